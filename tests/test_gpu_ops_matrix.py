"""Repair, verify, update, digest / locate and degraded read at every compiled
kernel shape, under residency caps, at random shapes, and queued back to back.

The per-operation files (test_gpu_repair, test_gpu_verify, test_gpu_update,
test_gpu_digest, test_gpu_read) share one small grid.  This file crosses what
that grid leaves out:

* every member count with_shape (csrc/xec_dispatch.h) compiles -- 1, 2, 4,
  8, 16, 32 -- and the generic loop below 8, at whole groups of 8 and at groups
  plus a tail;
* every (threads, unroll) pair at block sizes whose tiles come out full, cut
  inside granule row 0, and -- with two granules per lane -- "mixed": row 0
  whole and row 1 cut, where lanes of one wave take different paths;
* xec_set_occupancy, which none of these operations' own tests sets;
* random shapes, as test_gpu_fuzz does for encode and decode;
* long-list calls queued on a busy stream with no host synchronisation, which
  is what the pinned staging buffers of csrc/xec_api.cpp must survive.

Every expectation comes from outside the library: the oracle's encode, numpy
XOR (test_gpu_read.Batch), np_digest, and the pristine bytes.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re
import threading
from pathlib import Path

import numpy as np
import pytest

from test_digest_abi import np_digest
from test_gpu_digest import as_u64, expect_bitmap, ref_digests, run_locate, slots, stored
from test_gpu_fuzz import LAUNCH_SHAPES, _random_case
from test_gpu_read import Batch, Out, check_served, device_read, host_read
from test_gpu_repair import Case, pattern, run_repair, set_shape
from test_gpu_update import assert_state, expected, run_update, update_set
from test_gpu_verify import Flip, scrub

gpu_test = pytest.mark.gpu  # the shape arithmetic below runs without a device

CSRC = Path(__file__).resolve().parents[1] / "erasure-code-benchmark_amd" / "csrc"

SHAPES = [(64, 1), (64, 2), (256, 1), (256, 2)]  # (block_threads, unroll)
MEMBERS = [1, 2, 4, 8, 16, 32, 3, 9, 24, 40]     # k / m
MS = [1, 3]          # at m = 3 the class stride is not bs, so i % m matters
BSS = [8448, 14080]  # test_shape_arithmetic says why these two
S_MATRIX = 3
ENTRIES = ["host", "device"]
ROTATIONS = [0, -1, 1, 3, 129]

N_FUZZ_CASES = int(os.environ.get("XEC_FUZZ_CASES", "24"))
SEED_OFFSET = int(os.environ.get("XEC_FUZZ_SEED", "0"))


def _torch():
    import torch
    return torch


# --------------------------------------------------------------------------
# 1. Shape arithmetic: make_geometry (csrc/xec_kernels.h) and the fast-path
#    predicate of xor_members / reduce_members (csrc/xec_kernels.hip), restated.
# --------------------------------------------------------------------------
def tile_bytes(threads, unroll):
    return 16 * threads * unroll


def tiles_per_block(bs, threads, unroll):
    t = tile_bytes(threads, unroll)
    return (bs + t - 1) // t


def lanes_on_fast_path(bs, threads, unroll, tile):
    """Per lane of `tile`: does `off + (U - 1) * kStep < bs` hold?"""
    step = 16 * threads
    start = tile * tile_bytes(threads, unroll)
    return [start + lane * 16 + (unroll - 1) * step < bs for lane in range(threads)]


def tile_kind(bs, threads, unroll, tile):
    """'full': every lane takes the fast path.  'cut': the tile ends inside
    granule row 0.  'mixed': row 0 is whole and row 1 is partly or wholly past
    the block's end (two granules per lane only)."""
    if all(lanes_on_fast_path(bs, threads, unroll, tile)):
        return "full"
    if tile * tile_bytes(threads, unroll) + 16 * threads > bs:
        return "cut"
    return "mixed"


def tile_kinds(bs, threads, unroll):
    return {tile_kind(bs, threads, unroll, t) for t in range(tiles_per_block(bs, threads, unroll))}


def row1_probe(bs, threads):
    """(tile start, first byte of row 1) of the last two-granule tile that has
    a row 1 inside the block: the mixed tile where the block has one."""
    step = 16 * threads
    tile = 2 * step
    last = tiles_per_block(bs, threads, 2) - 1
    if last * tile + step >= bs:  # the last tile is cut: the one before it is full
        last -= 1
    assert last >= 0, "the block has no second granule row at this shape"
    return last * tile, last * tile + step


def verify_offsets(bs, threads):
    """The bytes xec_verify's flips go to: the first, the last, one in the
    middle of what row 1 of row1_probe's tile has inside the block, and the
    last byte of that tile's row 0 (in a mixed tile: a lane whose second
    granule is past the end)."""
    _, row1 = row1_probe(bs, threads)
    return 0, bs - 1, row1 + (min(bs, row1 + 16 * threads) - row1) // 2, row1 - 1


def read_ranges(bs, threads, unroll):
    """The whole block, all but 16 bytes at either end, and one tile plus 16
    bytes from 16 bytes before the first tile boundary of this shape (cut
    short where the block ends sooner: 8 KiB tiles do not fit twice)."""
    r = [(0, bs), (16, bs - 32)]
    tile = tile_bytes(threads, unroll)
    if tile < bs:
        r.append((tile - 16, min(tile + 16, bs - (tile - 16))))
    return r


def cell_index(members, m, bs):
    return (MEMBERS.index(members) * len(MS) + MS.index(m)) * len(BSS) + BSS.index(bs)


def overrides_for(ti, si):
    """(cache_policy, max_grid, rotation) of launch shape si in matrix cell ti."""
    q = ti + si
    return 1 + q % 2, (0, 2)[(q // 2) % 2], (0, 3)[(q // 4) % 2]


def compiled_member_counts():
    """The case labels of with_shape's member-count switch, from the source."""
    text = (CSRC / "xec_dispatch.h").read_text()
    body = text[text.index("switch (nm) {"):]
    body = body[: body.index("default:")]
    cases = [int(x) for x in re.findall(r"case (\d+):", body)]
    assert [int(x) for x in re.findall(r"with_shape<(\d+)>", body)] == cases
    return cases


def test_shape_arithmetic():
    """No device.  The matrix's block sizes give full and cut tiles at all four
    (threads, unroll) pairs and mixed tiles at both pairs with two granules per
    lane; its member counts are every compiled one and the three kinds of
    generic count; each override value meets each pair.  The restated formulas
    are the source's: a new switch case or another tile formula fails here."""
    norm = lambda s: " ".join(s.split())  # noqa: E731
    header = norm((CSRC / "xec_kernels.h").read_text())
    kernels = norm((CSRC / "xec_kernels.hip").read_text())
    assert "tile_bytes = 16ull * (uint64_t)ls.threads * (uint64_t)ls.unroll;" in header
    assert "g.tiles_per_block = (bs + tile_bytes - 1) / tile_bytes;" in header
    assert kernels.count("constexpr uint64_t kStep = (uint64_t)T * 16;") >= 3
    assert kernels.count("if (off + (U - 1) * kStep < bs) {") == 2  # xor_members, reduce_members
    assert kernels.count("if (off + (U - 1) * kStep < end) {") == 1  # xor_members_to
    assert kernels.count("(uint64_t)(T * U) + threadIdx.x) * 16;") >= 4  # a lane's first granule

    for threads, unroll in SHAPES:
        seen = set().union(*(tile_kinds(bs, threads, unroll) for bs in BSS))
        assert {"full", "cut"} <= seen, (threads, unroll, seen)
        assert ("mixed" in seen) == (unroll == 2), (threads, unroll, seen)
        # 8448 leaves 256 bytes past every tile size; 14080 leaves a whole row 0 and 768
        # or 1792 bytes of row 1 in its last two-granule tile
        assert tile_kinds(8448, threads, unroll) == {"full", "cut"}
        assert 8448 % tile_bytes(threads, unroll) == 256
        assert tile_kinds(14080, threads, unroll) == {"full", "mixed" if unroll == 2 else "cut"}
    assert [14080 % t for t in (1024, 2048, 4096, 8192)] == [768, 1792, 1792, 5888]
    # in the mixed tiles lanes of one wave diverge: some fast, some not
    for threads in (64, 256):
        last = tiles_per_block(14080, threads, 2) - 1
        lanes = lanes_on_fast_path(14080, threads, 2, last)
        waves = [lanes[w:w + 64] for w in range(0, threads, 64)]
        assert any(any(w) and not all(w) for w in waves), threads
    # the old grid's largest block is one ragged tile at 8 KiB and never mixed with full tiles
    assert tile_kinds(4352, 256, 2) == {"mixed"} and "mixed" not in tile_kinds(4352, 64, 2)

    # where the verify flips land
    for bs in BSS:
        for threads in (64, 256):
            first, last, row1, row0_end = verify_offsets(bs, threads)
            step, tile = 16 * threads, 32 * threads
            assert (first, last) == (0, bs - 1) and row1 < bs
            assert tile_kind(bs, threads, 2, first // tile) == "full"
            assert tile_kind(bs, threads, 2, last // tile) in ("cut", "mixed")
            assert (row1 % tile) // step == 1 and (row0_end % tile) // step == 0
            assert row1 // tile == row0_end // tile
            if "mixed" in tile_kinds(bs, threads, 2):
                t = row1 // tile
                assert tile_kind(bs, threads, 2, t) == "mixed"
                lanes = lanes_on_fast_path(bs, threads, 2, t)
                assert lanes[(row1 % step) // 16] and not lanes[(row0_end % step) // 16]
        for threads, unroll in SHAPES:  # the third read range crosses a tile boundary
            off, ln = read_ranges(bs, threads, unroll)[2]
            tile = tile_bytes(threads, unroll)
            assert off < tile < off + ln <= bs and off % 16 == 0 and ln % 16 == 0

    compiled = compiled_member_counts()
    assert compiled == [1, 2, 4, 8, 16, 32]
    assert set(compiled) <= set(MEMBERS), "a compiled member count the matrix does not run"
    generic = [n for n in MEMBERS if n not in compiled]
    assert any(n < 8 for n in generic)
    assert any(n >= 8 and n % 8 == 0 for n in generic)
    assert any(n > 8 and n % 8 != 0 for n in generic)
    assert any(8 < n < 16 for n in generic)  # one group plus a tail

    cells = [cell_index(n, m, bs) for n in MEMBERS for m in MS for bs in BSS]
    assert sorted(cells) == list(range(len(cells)))
    for si in range(len(SHAPES)):
        seen = {overrides_for(ti, si) for ti in cells}
        assert {v[0] for v in seen} == {1, 2} and {v[1] for v in seen} == {0, 2}
        assert {v[2] for v in seen} == {0, 3}


# --------------------------------------------------------------------------
# The five operation families on one encoded batch.
# --------------------------------------------------------------------------
def class_of(c: Case, cs, block):
    return cs * c.m + (block % c.m if block < c.k else block - c.k)


class Plan:
    """What one (S, k, m, bs) needs, computed once: the oracle's batch (Case),
    a repair bitmap, update sets with the oracle's re-encode, and a numpy batch
    for the reads.  The launch shapes are looped over it."""

    def __init__(self, gpu, oracle, S, k, m, bs, rng, sets=("third", "interleaved"),
                 loss="mixed"):
        self.c = c = Case.get(gpu, oracle, S, k, m, bs)
        self.repair_bm = pattern(rng, S, k, m, loss)
        ref_d = c.ref_d.cpu().numpy()
        self.updates = []
        for kind in sets:
            if kind == "random":
                pick = np.flatnonzero(rng.random(S * k) < rng.random())
                if pick.size == 0:
                    pick = np.array([int(rng.integers(S * k))])
                blocks = [divmod(int(q), k) for q in pick]
            else:
                blocks = update_set(rng, S, k, m, kind)
            fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
            self.updates.append((kind, blocks, fresh) + expected(oracle, c, ref_d, blocks, fresh))
        self.rb = Batch(S, k, m, bs, "classes")  # not cached: freed with the plan


def op_repair(gpu, c: Case, bm, what, entries=ENTRIES):
    for entry in entries:
        try:
            c.garbage(bm)
            st, verdict = run_repair(gpu, c, bm, entry)
            assert st == gpu.Status.SUCCESS and verdict == 0, (what, entry)
            c.assert_exact(f"after {entry} repair, {what}")
        finally:
            c.restore()


def op_verify(gpu, c: Case, rounds, what):
    """Zero flags on the intact batch; per round of (stripe, block, byte, bit)
    flips, each in a class of its own, exactly those flags and that count."""
    assert scrub(gpu, c) == ([], 0), f"intact batch flagged, {what}"
    for flips in rounds:
        want = sorted({class_of(c, cs, blk) for cs, blk, _, _ in flips})
        assert len(want) == len(flips)
        with contextlib.ExitStack() as es:
            for cs, blk, byte, bit in flips:
                es.enter_context(Flip(c, cs, blk, byte, bit))
            assert scrub(gpu, c) == (want, len(want)), (what, flips)
    c.assert_exact(f"the scrub changed data or parity, {what}")


def op_update(gpu, c: Case, updates, what, entries=ENTRIES):
    for kind, blocks, fresh, exp_d, exp_p in updates:
        for entry in entries:
            try:
                assert run_update(gpu, c, blocks, fresh, entry) == gpu.Status.SUCCESS, (what, kind)
                assert_state(c, exp_d, exp_p, f"after {entry} update '{kind}', {what}")
            finally:
                c.restore()


def op_read(gpu, b: Batch, items, ranges, what):
    for offset, length in ranges:
        w = f"{what} [{offset}, +{length})"
        out = Out(len(items), length)
        assert host_read(gpu, b, items, offset, length, out) == gpu.Status.SUCCESS, w
        check_served(b, items, offset, length, out, "xec_read " + w)
        out_d = Out(len(items), length)
        assert device_read(gpu, b, items, offset, length, out_d) == (gpu.Status.SUCCESS, 0), w
        check_served(b, items, offset, length, out_d, "xec_read_device " + w)


def op_digest(gpu, c: Case, what):
    dig = slots(c)
    assert gpu.digest(c.d, c.p, c.S, c.bs, c.k, c.m, dig, None, c.b.stream) == gpu.Status.SUCCESS
    _torch().cuda.synchronize()
    assert np.array_equal(as_u64(dig), ref_digests(c).reshape(-1)), f"digests != numpy, {what}"


def matrix_flips(c: Case, threads):
    """Round 1: the first byte (a full tile), the last byte (a cut or mixed
    tile) and a byte of row 1 of the last two-granule tile, in three classes,
    the second in a parity block.  Round 2: the last byte of that tile's row 0."""
    first, last, row1, row0_end = verify_offsets(c.bs, threads)
    k, m, nm = c.k, c.m, c.k // c.m
    j = m // 2
    return [[(0, 0, first, 0x01), (1, k + m - 1, last, 0x80), (2, j + m * (nm - 1), row1, 0x10)],
            [(0, k - 1, row0_end, 0x04)]]


def matrix_items(b: Batch):
    """A lost data block, a lost parity block, a present block of either
    stripe, and whatever else stripe 2 lost (the other classes at m = 3)."""
    k = b.k
    assert b.bm[2, 0] == 0 and b.bm[0, k] == 0 and b.bm[0, 0] != 0 and b.bm[2, k] != 0
    items = [(2 << 8) | 0, (0 << 8) | k, (0 << 8) | 0, (2 << 8) | k]
    items += [(2 << 8) | int(i) for i in np.flatnonzero(b.bm[2] == 0) if i != 0]
    return np.array(items, np.uint32)


def run_ops(gpu, plan: Plan, threads, unroll, what, digest=True):
    """The five families under whatever overrides the caller has set."""
    c = plan.c
    op_repair(gpu, c, plan.repair_bm, what)
    op_verify(gpu, c, matrix_flips(c, threads), what)
    op_update(gpu, c, plan.updates, what)
    op_read(gpu, plan.rb, matrix_items(plan.rb), read_ranges(c.bs, threads, unroll), what)
    if digest:
        op_digest(gpu, c, what)


def reset_overrides(gpu):
    set_shape(gpu)
    assert gpu.set_occupancy(0) == gpu.Status.SUCCESS


# --------------------------------------------------------------------------
# 2. Member counts x launch shapes
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("members", MEMBERS)
def test_member_count_by_launch_shape(gpu, oracle, members, m, bs):
    """Every compiled member count and the generic loop's three kinds, at
    (64,1), (64,2), (256,1) and (256,2) with full, cut and mixed tiles; cache
    policy, grid cap and rotation cycle through the cells.  The oracle encodes
    once per (k, m, bs); the digest kernel ignores unroll, so it runs with the
    one-granule shapes only."""
    k = members * m
    ti = cell_index(members, m, bs)
    rng = np.random.default_rng(members * 1000 + m * 10 + bs)
    plan = Plan(gpu, oracle, S_MATRIX, k, m, bs, rng)
    try:
        for si, (threads, unroll) in enumerate(SHAPES):
            cache_policy, max_grid, rotation = overrides_for(ti, si)
            set_shape(gpu, unroll=unroll, max_grid=max_grid, cache_policy=cache_policy,
                      block_threads=threads, rotation=rotation)
            what = (f"{k}+{m} x {bs} threads={threads} unroll={unroll} policy={cache_policy} "
                    f"max_grid={max_grid} rotation={rotation}")
            run_ops(gpu, plan, threads, unroll, what, digest=unroll == 1)
    finally:
        reset_overrides(gpu)
        plan.c.restore()


# --------------------------------------------------------------------------
# 3. Residency caps
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("k", [8, 16, 32])
def test_residency_caps(gpu, oracle, k):
    """xec_set_occupancy 1, 3 and 8 at 64 and 256 threads: an LDS reservation
    changes how many waves are resident and no byte.  Then the automatic
    setting, which at 8 members is verify_auto_occupancy's own branch."""
    m, bs = 1, 8448
    plan = Plan(gpu, oracle, S_MATRIX, k, m, bs, np.random.default_rng(k))
    try:
        for waves in (1, 3, 8):
            for threads in (64, 256):
                set_shape(gpu, block_threads=threads)
                assert gpu.set_occupancy(waves) == gpu.Status.SUCCESS
                run_ops(gpu, plan, threads, 1, f"{k}+{m} x {bs} waves={waves} threads={threads}")
        reset_overrides(gpu)
        run_ops(gpu, plan, 64, 1, f"{k}+{m} x {bs} automatic residency")
    finally:
        reset_overrides(gpu)
        plan.c.restore()


# --------------------------------------------------------------------------
# 4. Random shapes
# --------------------------------------------------------------------------
def fuzz_case(rng):
    """test_gpu_fuzz's shape, capped at k + m <= 256 (the host forms' packing),
    with blocks of up to 60 x 256 bytes: past the largest tile."""
    S, k, m, _ = _random_case(rng)
    if k + m > 256:
        k = m * ((256 - m) // m)
    bs = 256 * int(rng.integers(1, 61))
    S = max(1, min(S, (24 << 20) // (k * bs)))
    return S, k, m, bs


def test_fuzz_cases_stay_inside_the_host_forms():
    for case in range(200):
        S, k, m, bs = fuzz_case(np.random.default_rng(6161 + case))
        assert k % m == 0 and k >= m >= 1 and k + m <= 256 and S >= 1
        assert 256 <= bs <= 15360 and bs % 256 == 0 and S * k * bs <= 24 << 20
    assert max(fuzz_case(np.random.default_rng(6161 + c))[3] for c in range(200)) > 8192


@gpu_test
@pytest.mark.parametrize("case", range(N_FUZZ_CASES))
def test_random_shape_every_operation(gpu, oracle, case):
    """Random k, m, bs, S, launch shape, residency and rotation; random loss
    pattern, update set, corrupt bytes and read ranges; then xec_locate
    without flags against a bitmap built from the blocks damaged here."""
    case += SEED_OFFSET
    rng = np.random.default_rng(6161 + case)
    S, k, m, bs = fuzz_case(rng)
    unroll, max_grid, cache_policy, threads = LAUNCH_SHAPES[case % len(LAUNCH_SHAPES)]
    waves = int(rng.integers(0, 9))
    rotation = int(rng.choice(ROTATIONS))
    loss = ("parity", "data", "mixed")[int(rng.integers(3))]
    plan = Plan(gpu, oracle, S, k, m, bs, rng, sets=("random",), loss=loss)
    c, rb = plan.c, plan.rb
    what = (f"case {case}: {k}+{m} x {bs} x {S} launch={LAUNCH_SHAPES[case % len(LAUNCH_SHAPES)]} "
            f"waves={waves} rotation={rotation}")
    # corrupt bytes: one block in each of up to three classes, any byte, any nonzero change
    flips = []
    for cls in rng.permutation(S * m)[:3]:
        cs, j = divmod(int(cls), m)
        r = int(rng.integers(k // m + 1))
        block = k + j if r == k // m else j + m * r
        flips.append((cs, block, int(rng.integers(bs)), int(rng.integers(1, 256))))
    ranges = []
    for _ in range(3):
        offset = 16 * int(rng.integers(bs // 16))
        ranges.append((offset, 16 * int(rng.integers(1, (bs - offset) // 16 + 1))))
    items = rb.mixed_items(rng, int(rng.integers(4, 71)))
    try:
        assert gpu.set_launch(unroll, max_grid, cache_policy, threads) == gpu.Status.SUCCESS
        assert gpu.set_rotation(rotation) == gpu.Status.SUCCESS
        assert gpu.set_occupancy(waves) == gpu.Status.SUCCESS
        op_repair(gpu, c, plan.repair_bm, what)
        op_verify(gpu, c, [flips], what)
        op_update(gpu, c, plan.updates, what)
        op_read(gpu, rb, items, ranges, what)
        op_digest(gpu, c, what)
        dig = stored(c)  # numpy's digests of the oracle's bytes
        with contextlib.ExitStack() as es:
            for cs, blk, byte, bit in flips:
                es.enter_context(Flip(c, cs, blk, byte, bit))
            st, bm, cnt = run_locate(gpu, c, dig)
        assert st == gpu.Status.SUCCESS, what
        assert np.array_equal(bm, expect_bitmap(c, [(cs, blk) for cs, blk, _, _ in flips])), what
        assert cnt == len(flips), what
        c.assert_exact(f"at the end of {what}")
    finally:
        reset_overrides(gpu)
        c.restore()


# --------------------------------------------------------------------------
# 5. Sequences
# --------------------------------------------------------------------------
SEQ_S, SEQ_K, SEQ_M, SEQ_BS = 600, 8, 4, 256
SEQ_LOST = 1900  # more than the 1,800 entries a scratch of S*(k+m) bytes holds: two pieces


class StoreModel:
    """A numpy model of one parity store -- data, parity, bitmap, digests --
    and of what the queued sequence must leave in it.  Parity is the oracle's."""

    def __init__(self, oracle, seed):
        S, k, m, bs = SEQ_S, SEQ_K, SEQ_M, SEQ_BS
        rng = np.random.default_rng(seed)
        self.d0 = rng.integers(0, 256, size=S * k * bs, dtype=np.uint8)
        self.p0 = self.encode(oracle, self.d0)
        self.dig0 = np_digest(self.blocks(self.d0, self.p0))
        # step 1: two different long lists, then the digests of what they changed
        self.lists = []
        d1 = self.d0.copy()
        self.sel = np.zeros((S, k + m), np.uint8)
        for n in (1100, 1150):
            q = np.sort(rng.permutation(S * k)[:n])
            cs, i = q // k, q % k
            fresh = rng.integers(0, 256, size=(n, bs), dtype=np.uint8)
            d1.reshape(S, k, bs)[cs, i] = fresh
            self.sel[cs, i] = (1, 2, 255)[n % 3]
            self.sel[cs, k + i % m] = 1
            self.lists.append((((cs << 8) | i).astype(np.uint32), fresh))
        assert not np.array_equal(self.lists[0][0][:1100], self.lists[1][0][:1100])
        self.d1, self.p1 = d1, self.encode(oracle, d1)
        final = self.blocks(self.d1, self.p1)
        self.dig1 = np.where(self.sel != 0, np_digest(final), self.dig0)
        assert np.array_equal(self.dig1, np_digest(final))  # every changed block was selected
        # step 2: one block lost in each of SEQ_LOST classes, data or parity
        self.bm = np.ones((S, k + m), np.uint8)
        for cls in rng.permutation(S * m)[:SEQ_LOST]:
            c, j = divmod(int(cls), m)
            r = int(rng.integers(k // m + 1))
            self.bm[c, k + j if r == k // m else j + m * r] = 0
        lost, present = np.argwhere(self.bm == 0), np.argwhere(self.bm != 0)
        assert len(lost) == SEQ_LOST > S * (k + m) // 4
        assert (lost[:, 1] >= k).any() and (lost[:, 1] < k).any()
        pick = np.concatenate([lost[rng.integers(len(lost), size=550)],
                               present[rng.integers(len(present), size=550)]])
        pick = pick[rng.permutation(len(pick))]
        self.read_items = ((pick[:, 0] << 8) | pick[:, 1]).astype(np.uint32)
        self.read_range = (16, bs - 32)
        off, ln = self.read_range
        self.read_want = final[pick[:, 0], pick[:, 1], off:off + ln]

    @staticmethod
    def encode(oracle, d):
        S, k, m, bs = SEQ_S, SEQ_K, SEQ_M, SEQ_BS
        src, p = oracle.aligned(d.size), oracle.aligned(S * m * bs)
        src[:] = d
        assert oracle.encode_batch(src, p, S, bs, k, m) == 0
        return p.copy()

    @staticmethod
    def blocks(d, p):
        S, k, m, bs = SEQ_S, SEQ_K, SEQ_M, SEQ_BS
        return np.concatenate([d.reshape(S, k, bs), p.reshape(S, m, bs)], axis=1)


def same(got, want):
    if isinstance(want, list):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    return np.array_equal(got, want)


def run_sequence(gpu, model: StoreModel, errors, tag, sync_each=False):
    """Queue the whole sequence on one new stream behind a long fill; one
    synchronisation at the end (sync_each: one after every call instead).
    Mismatches with the model go to `errors`."""
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = SEQ_S, SEQ_K, SEQ_M, SEQ_BS
    n_blocks = S * (k + m)
    try:
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to("cuda")  # noqa: E731
            fill = lambda n, v, dt=torch.uint8: torch.full((n,), v, dtype=dt, device="cuda")  # noqa: E731
            d, p, dig = dev(model.d0), dev(model.p0), dev(model.dig0)
            news = [dev(fresh) for _, fresh in model.lists]
            up_scratch = [fill(gpu.update_scratch_bytes(len(it)), 0x3C) for it, _ in model.lists]
            d_sel, d_bm = dev(model.sel), dev(model.bm)
            h_bm = np.ascontiguousarray(model.bm.reshape(-1))
            n_read = len(model.read_items)
            out = Out(n_read, model.read_range[1])
            rd_bytes = gpu.read_scratch_bytes(n_read)
            rd_scratch = fill(rd_bytes, 0x3C)
            rp_scratch = fill(n_blocks, 0x3C)
            flags, vcount = fill(S * m, 0xFF), fill(1, 77, torch.int32)
            wb = gpu.locate_work_bytes(S, k, m)
            lbm = [fill(n_blocks, 0xA5) for _ in range(2)]
            lcount = [fill(1, 77, torch.int32) for _ in range(2)]
            work = [fill(wb, 0x3C) for _ in range(2)]
            busy = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
            s.synchronize()
            step = s.synchronize if sync_each else (lambda: None)
            # step 0: keep the stream busy, so that the copies below stay queued
            for v in range(24):
                busy.fill_(v)
            # step 1
            for (items, _), new, scratch in zip(model.lists, news, up_scratch):
                assert gpu.update(d, p, new, S, bs, k, m, items, len(items), scratch,
                                  scratch.numel(), s) == St.SUCCESS
                assert gpu.update_tiling_used() == 3
                step()
            assert gpu.digest(d, p, S, bs, k, m, dig, d_sel, s) == St.SUCCESS
            step()
            # step 2
            assert gpu.erase(d, p, S, bs, k, m, d_bm, s) == St.SUCCESS
            step()
            assert gpu.read(d, p, S, bs, k, m, h_bm, model.read_items, n_read, model.read_range[0],
                            model.read_range[1], out.ptr, rd_scratch, rd_bytes, s) == St.SUCCESS
            assert gpu.read_tiling_used() == 3
            step()
            assert gpu.repair(d, p, S, bs, k, m, h_bm, rp_scratch, s) == St.SUCCESS
            assert gpu.repair_tiling_used() == 3
            step()
            assert gpu.verify(d, p, S, bs, k, m, flags, vcount, s) == St.SUCCESS
            step()
            assert gpu.locate(d, p, S, bs, k, m, dig, flags, lbm[0], lcount[0], work[0], wb,
                              s) == St.SUCCESS
            step()
            # and every block against the refreshed digests, without the flags' gate
            assert gpu.locate(d, p, S, bs, k, m, dig, None, lbm[1], lcount[1], work[1], wb,
                              s) == St.SUCCESS
            still_busy = not s.query()
            s.synchronize()
            print(f"{tag}: stream still busy when the last call returned: {still_busy}")
            got = dict(data=d.cpu().numpy(), parity=p.cpu().numpy(), read=out.body(),
                       digests=as_u64(dig).reshape(S, k + m), flags=flags.cpu().numpy(),
                       verify_count=int(vcount.item()),
                       locate_bitmaps=[b.cpu().numpy() for b in lbm],
                       locate_counts=[int(x.item()) for x in lcount])
            guards = out.guards_intact()
        want = dict(data=model.d1, parity=model.p1, read=model.read_want, digests=model.dig1,
                    flags=np.zeros(S * m, np.uint8), verify_count=0,
                    locate_bitmaps=[np.ones(n_blocks, np.uint8)] * 2, locate_counts=[0, 0])
        for name, w in want.items():
            if not same(got[name], w):
                errors.append(f"{tag}: {name} differs from the model")
        if not guards:
            errors.append(f"{tag}: a guard byte of the read's output was written")
    except Exception as e:  # noqa: BLE001 - collected and asserted by the caller
        errors.append(f"{tag}: {e!r}")


@gpu_test
def test_queued_long_lists_against_a_model(gpu, oracle):
    """Two long xec_update lists, a selected xec_digest, xec_erase, a long
    xec_read, a two-piece xec_repair, xec_verify and xec_locate queued on one
    busy stream with no host synchronisation between them.  A staging buffer
    handed out while its copy is still queued shows as the wrong list applied."""
    errors: list[str] = []
    run_sequence(gpu, StoreModel(oracle, 50), errors, "one stream")
    assert not errors, errors


@gpu_test
def test_queued_long_lists_from_two_threads(gpu, oracle):
    """The same sequence from two threads at once, each on its own stream and
    batch: one pass each.  The staging pool is shared by the process."""
    errors: list[str] = []
    models = [StoreModel(oracle, 60 + t) for t in range(2)]
    threads = [threading.Thread(target=run_sequence, args=(gpu, models[t], errors, f"thread {t}"))
               for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=100)
    assert not any(th.is_alive() for th in threads), "a worker did not finish"
    assert not errors, errors


@gpu_test
def test_long_lists_synchronised_after_each_call(gpu, oracle):
    """The same sequence with a synchronisation after every call: the model
    holds whether or not the copies were still queued."""
    errors: list[str] = []
    run_sequence(gpu, StoreModel(oracle, 70), errors, "synchronised", sync_each=True)
    assert not errors, errors


def get_tuning(gpu):
    from xec._lib import Tuning
    t = Tuning()
    assert gpu.lib().xec_get_tuning(ctypes.byref(t)) == gpu.Status.SUCCESS
    return {name: int(getattr(t, name)) for name, _ in Tuning._fields_}


def tilings_used(gpu):
    return dict(decode=gpu.decode_tiling_used(), repair=gpu.repair_tiling_used(),
                update=gpu.update_tiling_used(), read=gpu.read_tiling_used())


@gpu_test
def test_overrides_change_between_synchronised_steps(gpu, oracle):
    """One operation per step, each under other launch overrides, synchronised
    after each: the bytes are the oracle's, xec_get_tuning returns what was
    set, and each *_tiling_used value moves with its own operation only."""
    S, k, m, bs = 3, 16, 2, 14080
    plan = Plan(gpu, oracle, S, k, m, bs, np.random.default_rng(81))
    c, rb = plan.c, plan.rb
    items = matrix_items(rb)
    intact = np.ones((S, k + m), np.uint8)
    what = "between synchronised steps"

    def read_step(reader, ok, offset, length):
        out = Out(len(items), length)
        assert reader(gpu, rb, items, offset, length, out) == ok
        check_served(rb, items, offset, length, out, what)

    # (launch overrides, waves per SIMD, the call, the *_tiling_used value it moves)
    steps = [
        (dict(unroll=2, max_grid=2, cache_policy=2, block_threads=256, rotation=3), 3,
         lambda: op_repair(gpu, c, plan.repair_bm, what, ["host"]), ("repair", 4)),
        (dict(unroll=1, block_threads=64), 1,
         lambda: op_verify(gpu, c, matrix_flips(c, 64), what), None),
        (dict(unroll=2, cache_policy=1, block_threads=64, rotation=1), 8,
         lambda: op_update(gpu, c, plan.updates[:1], what, ["device"]), ("update", 2)),
        (dict(unroll=1, max_grid=3, block_threads=256), 0,
         lambda: read_step(host_read, gpu.Status.SUCCESS, 16, bs - 32), ("read", 4)),
        (dict(cache_policy=2, max_grid=2, block_threads=256), 2,
         lambda: op_digest(gpu, c, what), None),
        (dict(unroll=2, block_threads=64, rotation=129), 4,
         lambda: op_repair(gpu, c, plan.repair_bm, what, ["device"]), ("repair", 2)),
        (dict(unroll=1, cache_policy=2, block_threads=256), 5,
         lambda: op_update(gpu, c, plan.updates[1:], what, ["host"]), ("update", 4)),
        (dict(unroll=2, max_grid=1, block_threads=256, rotation=-1), 7,
         lambda: read_step(device_read, (gpu.Status.SUCCESS, 0), 0, bs), ("read", 3)),
        (dict(), 0, lambda: op_repair(gpu, c, intact, what, ["host"]), ("repair", 0)),
    ]
    base = get_tuning(gpu)
    assert {base[n] for n in ("unroll", "max_grid", "cache_policy", "block_threads",
                              "waves_per_simd", "rotation")} == {0}
    try:
        for shape, waves, call, moved in steps:
            set_shape(gpu, **shape)
            assert gpu.set_occupancy(waves) == gpu.Status.SUCCESS
            want_tuning = dict(base, unroll=0, max_grid=0, cache_policy=0, block_threads=0,
                               rotation=0, waves_per_simd=waves)
            want_tuning.update(shape)
            assert get_tuning(gpu) == want_tuning
            before = tilings_used(gpu)
            call()
            _torch().cuda.synchronize()
            assert get_tuning(gpu) == want_tuning, "a call changed the overrides"
            want_used = dict(before)
            if moved is not None:
                want_used[moved[0]] = moved[1]
            assert tilings_used(gpu) == want_used, (shape, moved)
    finally:
        reset_overrides(gpu)
        c.restore()
    assert get_tuning(gpu) == base
