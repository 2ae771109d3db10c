"""Ranged update and degraded write at every compiled launch shape, under
residency caps, at k = 256, at random shapes, and queued back to back.

test_gpu_update_range and test_gpu_write share one small grid.  This file
crosses what that grid leaves out:

* every (threads, unroll) pair -- (256, 2) included -- over ranges whose tiles
  come out full, cut inside granule row 0 and "mixed" (row 0 whole, row 1 cut).
  The tiles of these two calls are chunks of the RANGE, so the kinds follow
  from `len`, not from the block size;
* the rebuild mode's grouped member loop: the lost written member at the first
  slot, at a group's last slot, as the first member of the second group and in
  the scalar tail, with present written members in a group and in the tail;
* xec_set_occupancy, which neither call's own tests set;
* k = 256, where block index 255 fills the item's low byte;
* random shapes, item sets, ranges and loss bitmaps built servable by
  construction;
* xec_write_device's verdict against a numpy restatement of the rule and
  against xec_check_write_items, three voices;
* long lists of both calls queued on a busy stream with no host
  synchronisation, which is what the pinned staging slots must survive.

Every expectation comes from outside the library, as in the two files above:
numpy patches of the ranges, oracle.encode_batch, GARBAGE in every lost block,
the state after xec_repair, xec.digest_host / np_digest for the slots with
sentinels in the untouched ones, and 0xA5 in whatever of d_new must not be read.
"""
from __future__ import annotations

import copy
import os
import threading
import types
from pathlib import Path

import numpy as np
import pytest

import test_gpu_update_range as R
import test_gpu_write as W
from test_digest_abi import np_digest
from test_gpu_fuzz import LAUNCH_SHAPES
from test_gpu_ops_matrix import (SHAPES, fuzz_case, overrides_for, reset_overrides, tile_bytes,
                                 tile_kind, tile_kinds, tiles_per_block, lanes_on_fast_path)
from test_gpu_repair import Case, run_repair, set_shape
from test_gpu_update import assert_state, expected, items_of, run_update, update_set

gpu_test = pytest.mark.gpu  # the coverage proof below runs without a device

CSRC = Path(__file__).resolve().parents[1] / "erasure-code-benchmark_amd" / "csrc"

MEMBERS = [1, 2, 7, 8, 9, 16, 17, 33]  # k / m: no group, one group, groups and a tail
MS = [1, 3]
BSS = [8448, 14080]
S_MATRIX = 3
ENTRIES = ["host", "device"]
# (offset, len) per block size; test_coverage_without_a_device says what each is for
RANGES = {
    8448: [(0, 8448), (1008, 5888), (32, 8416), (8432, 16)],
    14080: [(0, 14080), (16, 8448), (5632, 8448), (1008, 5888), (14064, 16)],
}
SETS = ["interleaved", "class"]
PATTERNS = ["mixed", "tail"]
# the member of the "tail" pattern's first rebuild class that is lost, by member count
TAIL_X = {1: 0, 2: 0, 7: 6, 8: 7, 9: 8, 16: 7, 17: 16, 33: 32}

N_FUZZ_CASES = int(os.environ.get("XEC_FUZZ_CASES", "24"))
SEED_OFFSET = int(os.environ.get("XEC_FUZZ_SEED", "0"))
FUZZ_SEED = 7171
N_VERDICT_CASES = 200
VERDICT_KM = [(4, 1), (6, 3), (8, 4), (9, 1), (16, 2)]
VERDICT_S, VERDICT_BS = 64, 256


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def tiling_diagnostics_left_at_zero():
    """As test_gpu_write: the cases here end with an xec_repair or an
    xec_update_range; a call with nothing to do puts those calls'
    *_tiling_used back to 0 for the ABI tests of the same process."""
    yield
    import xec
    xec.repair(0, 0, 0, 256, 1, 1, None, None)
    xec.update_range(0, 0, 0, 0, 256, 1, 1, None, 0, 0, 16)
    assert xec.repair_tiling_used() == 0 and xec.update_tiling_used() == 0


# --------------------------------------------------------------------------
# Restatements: the loss rule of include/xec.h, the loss bits of a list
# --------------------------------------------------------------------------
def np_servable(bm, blocks, k, m):
    """xec.h: an item is servable if its block is present, or if it is lost and
    every other block of its class (members and parity) is present."""
    lost = np.asarray(bm) == 0
    for cs, i in blocks:
        j = i % m
        in_class = int(lost[cs, j:k:m].sum()) + int(lost[cs, k + j])
        if lost[cs, i] and in_class > 1:
            return False
    return True


def np_write_verdict(bm, mask, k, m):
    """4 if a marked block is lost while another block of its class is lost."""
    lost = np.asarray(bm) == 0
    marked = np.asarray(mask) != 0
    bad = False
    for j in range(m):
        count = lost[:, j:k:m].sum(axis=1) + lost[:, k + j]
        marked_lost = (lost[:, j:k:m] & marked[:, j::m]).any(axis=1)
        bad |= bool((marked_lost & (count > 1)).any())
    return 4 if bad else 0


def np_write_bits(bm, items, k, m):
    """The 2-bit words that travel with a list: bit 0 = the item's block is
    lost, bit 1 = its class's parity block is lost; 16 items per word."""
    items = np.asarray(items, np.uint32)
    cs, i = (items >> 8).astype(np.int64), (items & 0xFF).astype(np.int64)
    b = (bm[cs, i] == 0).astype(np.uint32) | ((bm[cs, k + i % m] == 0).astype(np.uint32) << 1)
    words = np.zeros((len(items) + 15) // 16, np.uint32)
    t = np.arange(len(items))
    np.bitwise_or.at(words, t >> 4, b << (2 * (t & 15)).astype(np.uint32))
    return b, words


# --------------------------------------------------------------------------
# The matrix's cells, ranges and loss patterns
# --------------------------------------------------------------------------
def cell_index(members, m, bs):
    return (MEMBERS.index(members) * len(MS) + MS.index(m)) * len(BSS) + BSS.index(bs)


def tail_pattern(S, k, m):
    """(bitmap, sorted written (stripe, block) pairs, repairable), as
    test_gpu_write.pattern.  (stripe, class):
      (0, 0)    rebuild-write, the lost member at TAIL_X; written and present:
                members 0, 1, 7, the first of the tail and the last, where the
                class has them;
      (0, 1)    m > 1: delta, its items between those of (0, 0) in the list;
      (1, m-1)  delta beside a lost member nobody writes (one member per class:
                that member, and the class has no item);
      (2, 0)    m > 1 or one member: data-only, the first and last member;
      (2, m-1)  m > 1 or several members: rebuild-write, member 0 lost, the
                last member written and present."""
    assert S == 3
    nm = k // m
    j = m - 1
    bm = np.ones((S, k + m), np.uint8)
    x = TAIL_X[nm]
    w = {(0, r * m) for r in {x, 0, 1, 7, 8 * (nm // 8), nm - 1} if r < nm}
    bm[0, x * m] = 0
    if m > 1:
        w |= {(0, 1 + r * m) for r in {0, 1, nm - 1} if r < nm}
    if nm > 1:
        w.add((1, j))
        bm[1, j + (nm - 1) * m] = 0
    else:
        bm[1, j] = 0
    if m > 1 or nm == 1:
        w |= {(2, 0), (2, (nm - 1) * m)}
        bm[2, k] = 0
    if m > 1 or nm > 1:
        w |= {(2, j), (2, j + (nm - 1) * m)}
        bm[2, j] = 0
    return bm, sorted(w), True


def write_pattern(kind, S, k, m):
    return tail_pattern(S, k, m) if kind == "tail" else W.pattern(kind, S, k, m)


def rebuild_classes(S, k, m, bm, blocks):
    """[(member count, the lost written member r, the present written members)]
    of the rebuild-write classes of a pattern."""
    ns = types.SimpleNamespace(S=S, k=k, m=m)
    out = []
    for (cs, j), mode in W.modes_of(ns, bm, blocks).items():
        if mode != "rebuild":
            continue
        mine = [i // m for c2, i in blocks if c2 == cs and i % m == j]
        lost = [r for r in mine if bm[cs, j + r * m] == 0]
        assert len(lost) == 1
        out.append((k // m, lost[0], [r for r in mine if r != lost[0]]))
    return out


# --------------------------------------------------------------------------
# Random cases: servable by construction, nothing redrawn
# --------------------------------------------------------------------------
def random_write_case(rng, S, k, m, stats=None):
    """(bitmap, sorted written pairs, {(stripe, class): mode}, repairable).
    The mode of every (stripe, class) is drawn first -- none, delta, data-only
    or rebuild-write; one class, drawn beforehand, always writes -- then the
    written members, then the losses that give that mode, then losses nobody
    writes.  Nothing is rejected: what is drawn is what is returned."""
    nm = k // m
    bm = np.ones((S, k + m), np.uint8)
    blocks, modes = [], {}
    repairable = True
    forced = int(rng.integers(S * m))
    wild = bool(rng.integers(2))  # classes may lose two blocks: xec_repair refuses the batch
    for cs in range(S):
        for j in range(m):
            roll = int(rng.integers(4))
            if roll == 0 and cs * m + j == forced:
                roll = 1 + int(rng.integers(3))
            members = j + m * np.arange(nm)
            pick = np.zeros(nm, bool)
            if roll:
                pick = rng.random(nm) < rng.random()
                pick[int(rng.integers(nm))] = True
            written, rest = members[pick], members[~pick]
            blocks += [(cs, int(i)) for i in written]
            extra = int(rng.integers(3 if wild else 2))  # losses nobody writes
            if roll == 2 and not wild:
                extra = 0
            if roll == 0:    # no item: up to two of the class's blocks are lost
                pool = np.append(members, k + j)
                lose = rng.permutation(pool)[:extra]
            elif roll == 1:  # delta: the parity and every written member present
                modes[(cs, j)] = "delta"
                lose = rng.permutation(rest)[:extra]
            elif roll == 2:  # data-only: the parity lost, every written member present
                modes[(cs, j)] = "data"
                lose = np.append(rng.permutation(rest)[:extra % 2], k + j)
            else:            # rebuild-write: one written member lost and nothing else
                modes[(cs, j)] = "rebuild"
                lose = written[int(rng.integers(len(written)))]
            bm[cs, lose] = 0
            repairable &= np.size(lose) <= 1
    if stats is not None:
        stats["drawn"] = stats.get("drawn", 0) + 1
        stats["returned"] = stats.get("returned", 0) + 1
    return bm, sorted(blocks), modes, bool(repairable)


def fuzz_params(case, stats=None):
    rng = np.random.default_rng(FUZZ_SEED + case)
    S, k, m, bs = fuzz_case(rng)
    launch = LAUNCH_SHAPES[case % len(LAUNCH_SHAPES)]
    waves = int(rng.integers(0, 9))
    bm, blocks, modes, repairable = random_write_case(rng, S, k, m, stats)
    off = 16 * int(rng.integers(bs // 16))
    ln = 16 * int(rng.integers(1, (bs - off) // 16 + 1))
    return types.SimpleNamespace(S=S, k=k, m=m, bs=bs, launch=launch, waves=waves, bm=bm,
                                 blocks=blocks, modes=modes, repairable=repairable, off=off, ln=ln,
                                 rng=rng)


def verdict_case(case):
    """(k, m, S, bitmap, mask, offset, len) of one device-verdict case: a few
    lost blocks over a batch of 1 to 64 stripes, the mask from sparse to full."""
    rng = np.random.default_rng(9191 + case)
    k, m = VERDICT_KM[case % len(VERDICT_KM)]
    S = int(rng.integers(1, VERDICT_S + 1))
    n_lost = int(rng.integers(0, 9)) if case % 2 else int(rng.integers(0, 2 * S + 1))
    bm = np.ones(S * (k + m), np.uint8)
    bm[rng.permutation(bm.size)[:n_lost]] = 0
    marks = rng.choice(np.array([1, 2, 255], np.uint8), size=(S, k))
    mask = np.where(rng.random((S, k)) < (0.05, 0.3, 0.9)[int(rng.integers(3))], marks, 0)
    mask = mask.astype(np.uint8)
    if not mask.any():
        mask[int(rng.integers(S)), int(rng.integers(k))] = 1
    off = 16 * int(rng.integers(VERDICT_BS // 16))
    ln = 16 * int(rng.integers(1, (VERDICT_BS - off) // 16 + 1))
    return k, m, S, bm.reshape(S, k + m), mask, off, ln


# --------------------------------------------------------------------------
# The queued sequence's plan and model (section 7)
# --------------------------------------------------------------------------
SEQ_S, SEQ_K, SEQ_M, SEQ_BS = 600, 8, 4, 256
SEQ_LOST = 1900        # classes that lose one block: a repair list of two pieces
SEQ_RANGE = (16, 224)  # of the two xec_update_range lists
SEQ_WRITE = (112, 128)  # of the two xec_write lists


class SeqPlan:
    """What the sequence queues, without the oracle: two ranged-update lists,
    a bitmap that loses one block in SEQ_LOST classes, two write lists."""

    def __init__(self, seed):
        S, k, m = SEQ_S, SEQ_K, SEQ_M
        rng = self.rng = np.random.default_rng(seed)

        def one_list(n, ln):
            q = np.sort(rng.permutation(S * k)[:n])
            items = ((q // k) << 8 | (q % k)).astype(np.uint32)
            return items, rng.integers(0, 256, size=(n, ln), dtype=np.uint8)

        self.range_lists = [one_list(n, SEQ_RANGE[1]) for n in (1100, 1150)]
        self.bm = np.ones((S, k + m), np.uint8)
        for cls in rng.permutation(S * m)[:SEQ_LOST]:
            c, j = divmod(int(cls), m)
            r = int(rng.integers(k // m + 1))
            self.bm[c, k + j if r == k // m else j + m * r] = 0
        self.write_lists = [one_list(n, SEQ_WRITE[1]) for n in (1180, 1060)]
        self.bits = [np_write_bits(self.bm, items, k, m) for items, _ in self.write_lists]
        # the parity slots the writes leave stale: data-only classes with an item
        self.sel = np.zeros((S, k + m), np.uint8)
        for items, _ in self.write_lists:
            cs, i = (items >> 8).astype(np.int64), (items & 0xFF).astype(np.int64)
            stale = self.bm[cs, k + i % m] == 0
            self.sel[cs[stale], k + i[stale] % m] = 1


class RangeStoreModel(SeqPlan):
    """A numpy model of one parity store and of what the queued sequence must
    leave in it.  Parity is the oracle's, digests are np_digest's."""

    def __init__(self, oracle, seed):
        super().__init__(seed)
        S, k, m, bs = SEQ_S, SEQ_K, SEQ_M, SEQ_BS
        self.d0 = self.rng.integers(0, 256, size=S * k * bs, dtype=np.uint8)
        self.p0 = self.encode(oracle, self.d0)
        self.dig0 = np_digest(self.blocks(self.d0, self.p0))
        d = self.d0.copy()
        for lists, (off, ln) in ((self.range_lists, SEQ_RANGE), (self.write_lists, SEQ_WRITE)):
            for items, fresh in lists:
                cs, i = (items >> 8).astype(np.int64), (items & 0xFF).astype(np.int64)
                d.reshape(S, k, bs)[cs, i, off:off + ln] = fresh
        self.d1, self.p1 = d, self.encode(oracle, d)
        self.dig1 = np_digest(self.blocks(self.d1, self.p1))

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


# --------------------------------------------------------------------------
# 1. The coverage proof: no device
# --------------------------------------------------------------------------
def test_coverage_without_a_device():
    """The source formulas this file restates, the tile kinds of the chosen
    ranges, the positions of the lost member, and the generators' promises."""
    import xec
    norm = lambda s: " ".join(s.split())  # noqa: E731
    kernels = norm((CSRC / "xec_kernels.hip").read_text())
    # the ranged update's kernels and launcher; the degraded write's
    patch = kernels[kernels.index("constexpr int kPatchDataStoreAux"):
                    kernels.index("constexpr int kWriteDelta")]
    write = kernels[kernels.index("constexpr int kWriteDelta"):
                    kernels.index("hipError_t launch_write_check")]
    # both launchers count the chunks of the RANGE, through the one helper that does; a lane's
    # granule takes part while below `end`
    helper = kernels[kernels.index("Geometry range_geometry("):
                     kernels.index("hipError_t launch_encode(")]
    assert kernels.count("g.tiles_per_block = (len + tile_bytes - 1) / tile_bytes;") == 1
    assert helper.count("g.tiles_per_block = (len + tile_bytes - 1) / tile_bytes;") == 1
    assert helper.count("const uint64_t tile_bytes = 16ull * (uint64_t)ls.threads * "
                        "(uint64_t)ls.unroll;") == 1
    for part in (patch, write):
        assert part.count("const Geometry g = range_geometry(") == 1
        assert part.count("g.tiles_per_block =") == 0 and part.count("tile_bytes") == 0
    # every load, fold, digest term and store of a granule is guarded, and by nothing else
    assert patch.count("if (off + u * kStep < end)") == 9
    assert patch.count("for (int u = 0; u < U; ++u)") == 9
    assert write.count("if (w.off + u * kStep < w.end)") == 12
    assert write.count("for (int u = 0; u < U; ++u)") == 13  # the 12 and the zeroing of acc, oldx
    assert kernels.count("const uint64_t rel = (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;") == 2
    assert patch.count("rr.offset + (tc.chunk * (uint64_t)(T * U) + threadIdx.x) * 16;") == 1
    assert write.count("rr.offset + (tc.chunk * (uint64_t)(T * U) + threadIdx.x) * 16;") == 1
    # groups of 8 members, not with upkeep, then the scalar tail
    assert write.count("for (; !DIG && r + 8 <= nm; r += 8) {") == 1
    assert write.count("const uint8_t* from[8];") == 1 and write.count("u32x4 v[8][U];") == 1
    assert write.count("for (; r < nm; ++r) {") == 1

    # ---- ranges: tile kinds follow from len ----
    for bs in BSS:
        ranges = RANGES[bs]
        assert all(off % 16 == 0 and ln % 16 == 0 and ln > 0 and off + ln <= bs for off, ln in ranges)
        assert (0, bs) in ranges and (bs - 16, 16) in ranges
        assert any(off > 0 and off + ln < bs and ln > 16 for off, ln in ranges)
        assert any(off > 0 and off + ln == bs and ln > 16 for off, ln in ranges)
        for threads, unroll in SHAPES:
            tile = tile_bytes(threads, unroll)
            seen = set().union(*(tile_kinds(ln, threads, unroll) for _, ln in ranges))
            assert {"full", "cut"} <= seen, (bs, threads, unroll, seen)
            assert ("mixed" in seen) == (unroll == 2), (bs, threads, unroll, seen)
            # a full tile FOLLOWED by a ragged one in one range
            assert any(len(tile_kinds(ln, threads, unroll)) == 2 for _, ln in ranges)
            if unroll == 2:  # in some mixed tile the lanes of one wave diverge
                diverging = False
                for _, ln in ranges:
                    last = tiles_per_block(ln, threads, unroll) - 1
                    if tile_kind(ln, threads, unroll, last) != "mixed":
                        continue
                    lanes = lanes_on_fast_path(ln, threads, unroll, last)
                    waves = [lanes[q:q + 64] for q in range(0, threads, 64)]
                    diverging |= any(any(q) and not all(q) for q in waves)
                assert diverging, (bs, threads)
            if threads == 256:  # a cut tile with whole waves past the end: they add nothing
                assert any(0 < ln % tile <= 16 * (threads - 64) and
                           tile_kind(ln, threads, unroll, ln // tile) == "cut" for _, ln in ranges)
    assert RANGES[14080] == [(0, 14080), (16, 8448), (5632, 8448), (1008, 5888), (14064, 16)]
    assert [ln % 8192 for ln in (14080, 8448, 5888, 8416)] == [5888, 256, 5888, 224]

    # ---- cells: every override value meets every shape; max_grid=2 strides ----
    cells = [cell_index(n, m, bs) for n in MEMBERS for m in MS for bs in BSS]
    assert sorted(cells) == list(range(len(cells)))
    for si in range(len(SHAPES)):
        seen = {overrides_for(ti, si) for ti in cells}
        assert {v[0] for v in seen} == {1, 2} and {v[1] for v in seen} == {0, 2}
    for members in MEMBERS:
        for m in MS:
            k = members * m
            rng = np.random.default_rng(0)
            n_range = max(len(update_set(rng, S_MATRIX, k, m, kind)) for kind in SETS)
            n_write = max(len(write_pattern(kind, S_MATRIX, k, m)[1]) for kind in PATTERNS)
            for bs in BSS:
                # list tiles = items x chunks, class tiles = S x m x chunks: more than the two
                # workgroups of max_grid=2 at every shape, so they stride and run in reverse
                for threads, unroll in SHAPES:
                    most = max(tiles_per_block(ln, threads, unroll) for _, ln in RANGES[bs])
                    assert min(n_range, n_write, S_MATRIX * m) * most > 2, (members, m, bs, threads)

    # ---- member counts: where the lost written member stands ----
    assert sorted(TAIL_X) == MEMBERS
    for m in MS:
        x_seen, present_seen = set(), set()
        for members in MEMBERS:
            k = members * m
            cell_modes = set()
            for kind in PATTERNS:
                bm, blocks, repairable = write_pattern(kind, S_MATRIX, k, m)
                assert repairable and blocks == sorted(set(blocks)) and all(i < k for _, i in blocks)
                assert np_servable(bm, blocks, k, m)
                st, n_rebuild, _ = xec.check_write_items(bm.reshape(-1), S_MATRIX, k, m,
                                                         items_of(blocks), len(blocks))
                assert st == xec.Status.SUCCESS and n_rebuild >= 1
                ns = types.SimpleNamespace(S=S_MATRIX, k=k, m=m)
                cell_modes |= set(W.modes_of(ns, bm, blocks).values())
                lost = bm == 0
                if kind == "tail":  # an unwritten lost member, in a class other than a rebuild's
                    unwritten = [(cs, i) for cs, i in np.argwhere(lost[:, :k]) if (cs, i) not in blocks]
                    assert unwritten
                for nm, r, present in rebuild_classes(S_MATRIX, k, m, bm, blocks):
                    groups = nm // 8
                    if r == 0:
                        x_seen.add("first member")
                    if r == 7 and groups >= 1:
                        x_seen.add("a group's last slot")
                    if r == 8 and groups >= 2:
                        x_seen.add("first of the second group")
                    if r >= 8 * groups and groups >= 1:
                        x_seen.add("tail after a group")
                    if groups >= 1:
                        present_seen |= {"group" if q < 8 * groups else "tail" for q in present}
            assert cell_modes == {"delta", "data", "rebuild"}, (members, m, cell_modes)
        assert x_seen == {"first member", "a group's last slot", "first of the second group",
                          "tail after a group"}, (m, x_seen)
        assert present_seen == {"group", "tail"}, (m, present_seen)
    # what the older grid did: the lost member inside a full group, never at these slots
    for nm in (8, 9, 33):
        assert nm // 2 < 8 * (nm // 8) and nm // 2 not in (0, 7, 8)

    # ---- the random generators stay inside the ABI ----
    stats: dict = {}
    all_modes, refusals = set(), 0
    for case in range(200):
        f = fuzz_params(case, stats)
        S, k, m, bs = f.S, f.k, f.m, f.bs
        assert 1 <= m <= k <= 256 and k % m == 0 and S >= 1 and S * k * bs <= 24 << 20
        items = items_of(f.blocks)
        assert len(items) >= 1 and (np.diff(items.astype(np.int64)) > 0).all()
        assert all(0 <= cs < S and 0 <= i < k for cs, i in f.blocks)
        assert f.off % 16 == 0 and f.ln % 16 == 0 and f.ln >= 16 and f.off + f.ln <= bs
        assert len(items) * f.ln <= 24 << 20
        assert np_servable(f.bm, f.blocks, k, m), case
        assert W.modes_of(f, f.bm, f.blocks) == f.modes, case
        st, _, _ = xec.check_write_items(f.bm.reshape(-1), S, k, m, items, len(items))
        assert st == xec.Status.SUCCESS, case
        lost = f.bm == 0
        per_class = np.stack([lost[:, j:k:m].sum(axis=1) + lost[:, k + j] for j in range(m)], axis=1)
        assert f.repairable == bool((per_class <= 1).all()), case
        all_modes |= set(f.modes.values())
        refusals += not f.repairable
    assert stats == {"drawn": 200, "returned": 200}  # nothing rejected, nothing redrawn
    assert all_modes == {"delta", "data", "rebuild"} and 50 <= refusals <= 150

    # ---- the device-verdict cases: both outcomes common ----
    verdicts = []
    for case in range(N_VERDICT_CASES):
        k, m, S, bm, mask, off, ln = verdict_case(case)
        assert 1 <= S <= 64 and off + ln <= VERDICT_BS and off % 16 == 0 and ln % 16 == 0 and ln > 0
        verdicts.append(np_write_verdict(bm, mask, k, m))
        blocks = [(int(cs), int(i)) for cs, i in np.argwhere(mask != 0)]
        assert (verdicts[-1] == 0) == np_servable(bm, blocks, k, m)
    assert verdicts.count(4) * 4 >= N_VERDICT_CASES and verdicts.count(0) * 4 >= N_VERDICT_CASES

    # ---- the queued lists: long, ascending, all three modes, different bits ----
    for seed in (50, 60, 61, 70):
        plan = SeqPlan(seed)
        for items, _ in plan.range_lists + plan.write_lists:
            assert len(items) > 1024 and (np.diff(items.astype(np.int64)) > 0).all()
        assert not np.array_equal(plan.range_lists[0][0][:1100], plan.range_lists[1][0][:1100])
        lost = plan.bm == 0
        assert int(lost.sum()) == SEQ_LOST and lost[:, SEQ_K:].any() and lost[:, :SEQ_K].any()
        (b0, w0), (b1, w1) = plan.bits
        for b in (b0, b1):
            assert set(b.tolist()) == {0, 1, 2}  # delta, rebuild-write, data-only
        n = min(len(b0), len(b1))
        assert int((b0[:n] != b1[:n]).sum()) > n // 4
        assert int((w0[:n // 16] != w1[:n // 16]).sum()) > n // 32
        assert plan.sel.any() and not plan.sel[:, :SEQ_K].any()
        written = np.concatenate([items for items, _ in plan.write_lists])
        assert np_servable(plan.bm, [(int(q) >> 8, int(q) & 0xFF) for q in written], SEQ_K, SEQ_M)


# --------------------------------------------------------------------------
# 2. Launch shapes by member count and range
# --------------------------------------------------------------------------
def range_calls(gpu, oracle, c: Case, sets, ranges, rng, what, upkeeps=(False, True)):
    """xec_update_range and its device form over `sets` x `ranges`."""
    ref_d = c.ref_d.cpu().numpy()
    for off, ln in ranges:
        for kind, blocks in sets:
            fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
            exp = R.model(oracle, c, ref_d, blocks, fresh, off, ln)
            for entry in ENTRIES:
                for upkeep in upkeeps:
                    w = f"update_range {entry} '{kind}' [{off},+{ln}) upkeep={upkeep}, {what}"
                    try:
                        R.check_call(gpu, oracle, c, blocks, fresh, off, ln, entry, upkeep, w, exp)
                        want = 2 if entry == "device" else 4 if len(blocks) <= 1024 else 3
                        assert gpu.update_tiling_used() == want, w
                    finally:
                        c.restore()


def write_calls(gpu, oracle, c: Case, patterns, ranges, rng, what, upkeeps=(False, True)):
    """xec_write and its device form over `patterns` x `ranges`."""
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    for off, ln in ranges:
        for kind, (bm, blocks, repairable) in patterns:
            fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
            exp = W.model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
            for entry in ENTRIES:
                for upkeep in upkeeps:
                    w = f"write {entry} '{kind}' [{off},+{ln}) upkeep={upkeep}, {what}"
                    try:
                        W.check_call(gpu, oracle, c, bm, blocks, fresh, off, ln, entry, upkeep, w,
                                     exp, repairable)
                        want = 2 if entry == "device" else 4 if len(blocks) <= 1024 else 3
                        assert gpu.write_tiling_used() == want, w
                    finally:
                        c.restore()


@gpu_test
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("members", MEMBERS)
def test_member_count_by_launch_shape(gpu, oracle, members, m, bs):
    """(64,1), (64,2), (256,1) and (256,2) over ranges with full, cut and mixed
    tiles; cache policy, grid cap and rotation (which must not apply) cycle
    through the cells.  Both calls, both entries, with and without upkeep."""
    k = members * m
    ti = cell_index(members, m, bs)
    rng = np.random.default_rng(members * 1000 + m * 10 + bs)
    c = Case.get(gpu, oracle, S_MATRIX, k, m, bs)
    sets = [(kind, update_set(rng, S_MATRIX, k, m, kind)) for kind in SETS]
    patterns = [(kind, write_pattern(kind, S_MATRIX, k, m)) for kind in PATTERNS]
    try:
        for si, (threads, unroll) in enumerate(SHAPES):
            cache_policy, max_grid, rotation = overrides_for(ti, si)
            set_shape(gpu, unroll=unroll, max_grid=max_grid, cache_policy=cache_policy,
                      block_threads=threads, rotation=rotation)
            what = (f"{k}+{m} x {bs} threads={threads} unroll={unroll} policy={cache_policy} "
                    f"max_grid={max_grid} rotation={rotation}")
            range_calls(gpu, oracle, c, sets, RANGES[bs], rng, what)
            write_calls(gpu, oracle, c, patterns, RANGES[bs], rng, what)
    finally:
        reset_overrides(gpu)
        c.restore()


# --------------------------------------------------------------------------
# 3. Residency
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("k", [8, 33])
def test_residency_caps(gpu, oracle, k):
    """xec_set_occupancy 1, 3 and 8 at 64 and 256 threads, two granules per
    lane, then the automatic setting: an LDS reservation changes how many waves
    are resident and no byte and no slot.  The range ends in a mixed tile at
    both thread counts."""
    m, bs = 1, 8448
    ranges = [(1008, 5888)]
    assert all("mixed" in tile_kinds(5888, threads, 2) for threads in (64, 256))
    rng = np.random.default_rng(k)
    c = Case.get(gpu, oracle, S_MATRIX, k, m, bs)
    sets = [("interleaved", update_set(rng, S_MATRIX, k, m, "interleaved"))]
    patterns = [("tail", write_pattern("tail", S_MATRIX, k, m))]
    try:
        for waves, threads in [(w, t) for w in (1, 3, 8) for t in (64, 256)] + [(0, 64)]:
            set_shape(gpu, unroll=2, block_threads=threads)
            assert gpu.set_occupancy(waves) == gpu.Status.SUCCESS
            what = f"{k}+{m} x {bs} waves={waves} threads={threads}"
            range_calls(gpu, oracle, c, sets, ranges, rng, what, upkeeps=(True,))
            write_calls(gpu, oracle, c, patterns, ranges, rng, what, upkeeps=(True,))
    finally:
        reset_overrides(gpu)
        c.restore()


# --------------------------------------------------------------------------
# 4. k = 256
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("m", [1, 4])
def test_k_256_on_the_update_style_calls(gpu, oracle, m):
    """k = 256 is inside the limit of xec_update, xec_update_range and
    xec_write (k <= 256, not k + m <= 256): block index 255 fills the item's
    low byte.  xec_repair's own limit is k + m <= 256, so the state after the
    repair comes from xec_repair_device."""
    S, k, bs = 2, 256, 256
    blocks = [(0, 255), (1, 0), (1, 255)] + ([(1, 7)] if m == 4 else [])  # 7 and 255: class 3
    blocks.sort()
    assert [int(q) & 0xFF for q in items_of(blocks)].count(255) == 2
    rng = np.random.default_rng(256 + m)
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    St = gpu.Status
    try:
        # xec_update, xec_update_device
        fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
        exp_d, exp_p = expected(oracle, c, ref_d, blocks, fresh)
        for entry in ENTRIES:
            assert run_update(gpu, c, blocks, fresh, entry) == St.SUCCESS, entry
            assert gpu.update_tiling_used() == (4 if entry == "host" else 2)
            assert_state(c, exp_d, exp_p, f"xec_update {entry} at k=256, m={m}")
            c.restore()
        # xec_update_range and xec_write: a lost block 255 whose class rebuilds, a lost parity
        bm = np.ones((S, k + m), np.uint8)
        bm[0, 255] = 0
        bm[1, k] = 0
        md = W.modes_of(c, bm, blocks)
        assert md[(0, 255 % m)] == "rebuild" and md[(1, 0)] == "data"
        assert (md.get((1, 3)) == "delta") == (m == 4)
        for off, ln in ((0, bs), (112, 32)):
            range_calls(gpu, oracle, c, [("k256", blocks)], [(off, ln)], rng, f"k=256 m={m}")
            fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
            dev_d, dev_p, fin_d, fin_p = W.model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
            for entry in ENTRIES:
                for upkeep in (False, True):
                    what = f"xec_write {entry} [{off},+{ln}) upkeep={upkeep} at k=256, m={m}"
                    c.garbage(bm, W.GARBAGE)
                    dig = seeded = None
                    if upkeep:
                        seeded, dig = W.seed_slots(gpu, c, ref_d, ref_p, bm, blocks)
                    assert W.run_write(gpu, c, bm, blocks, fresh, off, ln, entry, dig) == (0, 0), what
                    assert gpu.write_tiling_used() == (4 if entry == "host" else 2), what
                    assert_state(c, dev_d, dev_p, what)
                    if upkeep:
                        want = W.want_slots(gpu, c, seeded, fin_d, fin_p, bm, blocks)
                        assert np.array_equal(R.as_u64(dig), want), what
                    assert run_repair(gpu, c, bm, "host")[0] == St.INVALID_SIZE  # k + m > 256
                    assert run_repair(gpu, c, bm, "device") == (St.SUCCESS, 0), what
                    assert_state(c, fin_d, fin_p, f"{what}, after the repair")
                    c.restore()
    finally:
        c.restore()


# --------------------------------------------------------------------------
# 5. Random shapes
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("case", range(N_FUZZ_CASES))
def test_random_shape_both_calls(gpu, oracle, case):
    """Random k, m, bs, S, launch shape and residency; a random item set, range
    and loss bitmap, every written item servable by construction.  Both calls,
    both entries, with and without upkeep; where the bitmap is one xec_repair
    refuses, the refusal is asserted in place of the state after it."""
    f = fuzz_params(case + SEED_OFFSET)
    what = (f"case {case + SEED_OFFSET}: {f.k}+{f.m} x {f.bs} x {f.S} launch={f.launch} "
            f"waves={f.waves} items={len(f.blocks)} repairable={f.repairable}")
    c = Case.get(gpu, oracle, f.S, f.k, f.m, f.bs)
    try:
        assert gpu.set_launch(*f.launch) == gpu.Status.SUCCESS
        assert gpu.set_occupancy(f.waves) == gpu.Status.SUCCESS
        range_calls(gpu, oracle, c, [("random", f.blocks)], [(f.off, f.ln)], f.rng, what)
        write_calls(gpu, oracle, c, [("random", (f.bm, f.blocks, f.repairable))], [(f.off, f.ln)],
                    f.rng, what)
    finally:
        reset_overrides(gpu)
        c.restore()


# --------------------------------------------------------------------------
# 6. The device verdict against the host scan and the rule
# --------------------------------------------------------------------------
@gpu_test
def test_device_verdict_against_the_host_scan(gpu, oracle):
    """200 random (bitmap, mask) pairs on the first S stripes of one batch per
    (k, m).  *d_status is 4 exactly when the numpy rule says so and exactly
    when xec_check_write_items refuses the marked blocks as items.  On a 4 no
    byte of data, parity or digests changes; on a 0 all three are the model's."""
    torch = _torch()
    St = gpu.Status
    bs = VERDICT_BS
    seen = []
    for case in range(N_VERDICT_CASES):
        k, m, S, bm, mask, off, ln = verdict_case(case)
        full = Case.get(gpu, oracle, VERDICT_S, k, m, bs)
        c = copy.copy(full)  # the first S stripes: the layout is stripe-major
        c.S = S
        c.d, c.p = full.d[: S * k * bs], full.p[: S * m * bs]
        c.ref_d, c.ref_p = full.ref_d[: S * k * bs], full.ref_p[: S * m * bs]
        ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
        blocks = [(int(cs), int(i)) for cs, i in np.argwhere(mask != 0)]
        rule = np_write_verdict(bm, mask, k, m)
        host, _, _ = gpu.check_write_items(bm.reshape(-1), S, k, m, items_of(blocks), len(blocks))
        assert host in (St.SUCCESS, St.DECODE_FAILURE)
        assert (rule == 4) == (host == St.DECODE_FAILURE), f"case {case}: the rule and the host scan"
        rng = np.random.default_rng(case)
        fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
        h_shadow = np.full((S, k, bs), 0xA5, np.uint8)
        for t, (cs, i) in enumerate(blocks):
            h_shadow[cs, i, off:off + ln] = fresh[t]
        try:
            c.garbage(bm, W.GARBAGE)
            d0, p0 = c.d.clone(), c.p.clone()
            seeded, dig = W.seed_slots(gpu, c, ref_d, ref_p, bm, blocks)
            status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
            st = gpu.write_device(c.d, c.p, torch.from_numpy(h_shadow.reshape(-1)).to("cuda"), S, bs,
                                  k, m, torch.from_numpy(bm.reshape(-1).copy()).to("cuda"),
                                  torch.from_numpy(mask.reshape(-1).copy()).to("cuda"), off, ln, dig,
                                  status, c.b.stream)
            torch.cuda.synchronize()
            assert st == St.SUCCESS
            verdict = int(status.item())
            assert verdict == rule, f"case {case}: {k}+{m} x {S}: device {verdict}, rule {rule}"
            if verdict == 4:
                assert torch.equal(c.d, d0) and torch.equal(c.p, p0), f"case {case}: bytes changed"
                assert np.array_equal(R.as_u64(dig), seeded), f"case {case}: slots changed"
            else:
                dev_d, dev_p, fin_d, fin_p = W.model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off,
                                                     ln)
                assert_state(c, dev_d, dev_p, f"case {case}")
                want = W.want_slots(gpu, c, seeded, fin_d, fin_p, bm, blocks)
                assert np.array_equal(R.as_u64(dig), want), f"case {case}: slots"
            seen.append(verdict)
        finally:
            full.restore()
    assert seen.count(4) * 4 >= len(seen) and seen.count(0) * 4 >= len(seen)


# --------------------------------------------------------------------------
# 7. Queued long lists
# --------------------------------------------------------------------------
def same(got, want):
    return np.array_equal(got, want)


def run_sequence(gpu, model: RangeStoreModel, errors, tag, sync_each=False):
    """Queue the whole sequence on one new stream behind a long fill; one
    synchronisation at the end (sync_each: one after every call instead).
    xec_erase zeroes the lost blocks before the writes, so a write that read
    one shows.  Mismatches with the model go to `errors`."""
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
            r_news = [dev(fresh) for _, fresh in model.range_lists]
            r_scratch = [fill(gpu.update_scratch_bytes(len(it)), 0x3C) for it, _ in model.range_lists]
            w_news = [dev(fresh) for _, fresh in model.write_lists]
            w_scratch = [fill(gpu.write_scratch_bytes(len(it)), 0x3C) for it, _ in model.write_lists]
            d_sel, d_bm = dev(model.sel), dev(model.bm)
            h_bm = np.ascontiguousarray(model.bm.reshape(-1))
            rp_scratch = fill(n_blocks, 0x3C)
            flags, vcount = fill(S * m, 0xFF), fill(1, 77, torch.int32)
            wb = gpu.locate_work_bytes(S, k, m)
            lbm, lcount, work = fill(n_blocks, 0xA5), fill(1, 77, torch.int32), fill(wb, 0x3C)
            busy = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
            s.synchronize()
            step = s.synchronize if sync_each else (lambda: None)
            for v in range(24):  # keep the stream busy, so that the copies below stay queued
                busy.fill_(v)
            off, ln = SEQ_RANGE
            for (items, _), new, scratch in zip(model.range_lists, r_news, r_scratch):
                assert gpu.update_range(d, p, new, S, bs, k, m, items, len(items), off, ln, dig,
                                        scratch, scratch.numel(), s) == St.SUCCESS
                assert gpu.update_tiling_used() == 3
                step()
            assert gpu.erase(d, p, S, bs, k, m, d_bm, s) == St.SUCCESS
            step()
            off, ln = SEQ_WRITE
            for (items, _), new, scratch in zip(model.write_lists, w_news, w_scratch):
                assert gpu.write(d, p, new, S, bs, k, m, h_bm, items, len(items), off, ln, dig,
                                 scratch, scratch.numel(), s) == St.SUCCESS
                assert gpu.write_tiling_used() == 3
                step()
            assert gpu.repair(d, p, S, bs, k, m, h_bm, rp_scratch, s) == St.SUCCESS
            assert gpu.repair_tiling_used() == 3
            step()
            assert gpu.digest(d, p, S, bs, k, m, dig, d_sel, s) == St.SUCCESS
            step()
            assert gpu.verify(d, p, S, bs, k, m, flags, vcount, s) == St.SUCCESS
            step()
            assert gpu.locate(d, p, S, bs, k, m, dig, None, lbm, lcount, work, wb, s) == St.SUCCESS
            still_busy = not s.query()
            s.synchronize()
            print(f"{tag}: stream still busy when the last call returned: {still_busy}")
            got = dict(data=d.cpu().numpy(), parity=p.cpu().numpy(),
                       digests=R.as_u64(dig).reshape(S, k + m), flags=flags.cpu().numpy(),
                       verify_count=int(vcount.item()), locate_bitmap=lbm.cpu().numpy(),
                       locate_count=int(lcount.item()))
        want = dict(data=model.d1, parity=model.p1, digests=model.dig1,
                    flags=np.zeros(S * m, np.uint8), verify_count=0,
                    locate_bitmap=np.ones(n_blocks, np.uint8), locate_count=0)
        for name, w in want.items():
            if not same(got[name], w):
                errors.append(f"{tag}: {name} differs from the model")
    except Exception as e:  # noqa: BLE001 - collected and asserted by the caller
        errors.append(f"{tag}: {e!r}")


@gpu_test
def test_queued_long_lists_against_a_model(gpu, oracle):
    """Two long xec_update_range lists and, after xec_erase, two long xec_write
    lists, all with upkeep, then xec_repair, a selected xec_digest, xec_verify
    and a full xec_locate, queued on one busy stream with no host
    synchronisation between them.  A staging slot handed out while its copy is
    still queued shows as the wrong list or the wrong loss bits applied."""
    errors: list[str] = []
    run_sequence(gpu, RangeStoreModel(oracle, 50), errors, "one stream")
    assert not errors, errors


@gpu_test
def test_queued_long_lists_from_two_threads(gpu, oracle):
    """The same sequence from two threads at once, each on its own stream and
    batch: one pass each.  The staging pool is shared by the process."""
    errors: list[str] = []
    models = [RangeStoreModel(oracle, 60 + t) for t in range(2)]
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
    run_sequence(gpu, RangeStoreModel(oracle, 70), errors, "synchronised", sync_each=True)
    assert not errors, errors
