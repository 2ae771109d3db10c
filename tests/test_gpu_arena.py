"""Every device call at its minimum alignment inside a guarded arena.

The other files check VALUES; this one checks WHERE the library writes and
that it works at the alignments include/xec.h accepts.  Every device buffer of
every call is a region of one arena (tests/arena.py), carved at exactly the
documented size and exactly the minimum alignment:

    data, parity, d_new            64 bytes (at 64 mod 128)
    d_out                          16
    digests, locate's work         8
    status, count, items, list
    scratch, d_bad                 4
    bitmaps, flags, masks, select  an odd address

After every library call the documented outputs equal the model -- the oracle's
data and parity, numpy's digests, the pristine bytes (test_gpu_read.Batch.want)
-- and `arena.check(writable=[...])` proves that no other byte of the arena
changed: not a guard band, and not a region the call only reads.  Outputs are
prefilled with a sentinel before each call, so a call that writes nothing fails
the value check.

Models and helpers come from the per-operation files; the calls themselves are
made here, because those files' helpers allocate the side buffers (status,
device bitmap, d_new ...) that must be arena regions here.  host_read,
check_served and run_repair take every buffer from the caller and run unchanged.
"""
from __future__ import annotations

import contextlib
import copy
import types

import numpy as np
import pytest

from arena import Arena
from test_gpu_digest import as_u64, expect_bitmap, ref_digests
from test_gpu_ops_matrix import class_of, reset_overrides
from test_gpu_parity import SEED
from test_gpu_read import GARBAGE, GUARD, SENTINEL, Batch, Out, check_served, host_read
from test_gpu_repair import Case, pattern, run_repair, set_shape
from test_gpu_update import assert_state, expected, items_of, update_set
from test_gpu_verify import Flip

gpu_test = pytest.mark.gpu  # the grid's bookkeeping below runs without a device

S_A = 3
KMS = [(4, 1), (6, 3), (32, 1), (33, 3)]  # members 4, 2 (m > 1), 32 (capped residency), 11 (generic)
BSS = [256, 1280, 8448]  # the minimum; one 1 KiB tile and a cut one; full + cut at every tile size
LIST, VALID_TILINGS = 3, range(1, 7)  # XEC_TILING_LIST; what xec_decode_tiling_used may report
B_S, B_K, B_M, B_BS = 1100, 4, 2, 256


def _torch():
    import torch
    return torch


def cell_index(k, m, bs):
    return KMS.index((k, m)) * len(BSS) + BSS.index(bs)


def cache_policy_for(ci):
    """1 (non-temporal: the buffer-store path) or 2 (plain stores) by cell index."""
    return 1 + ci % 2


def test_grid_assignment():
    """No device.  Half of the cells run the override launch with cache policy
    1 and half with 2, and every (k, m) meets both."""
    cells = [(k, m, bs) for k, m in KMS for bs in BSS]
    idx = [cell_index(*c) for c in cells]
    assert sorted(idx) == list(range(len(cells)))
    pol = [cache_policy_for(i) for i in idx]
    assert pol.count(1) == pol.count(2) == len(cells) // 2
    for k, m in KMS:
        assert {cache_policy_for(cell_index(k, m, bs)) for bs in BSS} == {1, 2}
    assert [k // m for k, m in KMS] == [4, 2, 32, 11]


# --------------------------------------------------------------------------
# Arena-backed stand-ins for the shared Case / Batch / Out
# --------------------------------------------------------------------------
def pinned(a):
    return _torch().from_numpy(np.ascontiguousarray(a).reshape(-1)).pin_memory()


def arena_case(gpu, oracle, a: Arena, S, k, m, bs, stream=None):
    """test_gpu_repair.Case (the oracle's batch, checked once against the
    library's encode) whose d / p are the arena's 'data' / 'parity' regions."""
    c = copy.copy(Case.get(gpu, oracle, S, k, m, bs))
    c.d, c.p = a["data"], a["parity"]
    assert c.d.numel() == S * k * bs and c.p.numel() == S * m * bs
    assert c.d.data_ptr() % 128 == 64 and c.p.data_ptr() % 64 == 0
    a.put("data", c.ref_d)
    a.put("parity", c.ref_p)
    if stream is not None:
        c.b = types.SimpleNamespace(stream=stream)
    return c


class ArenaBatch(Batch):
    """test_gpu_read.Batch over an arena case: the pristine blocks are the
    oracle's, the damaged copy is the case's data and parity with the lost
    blocks overwritten, the device bitmap is the arena's 'bitmap' region."""

    def __init__(self, a: Arena, c: Case, bm):
        self.S, self.k, self.m, self.bs = c.S, c.k, c.m, c.bs
        self.blocks = np.concatenate([c.ref_d.cpu().numpy().reshape(c.S, c.k, c.bs),
                                      c.ref_p.cpu().numpy().reshape(c.S, c.m, c.bs)], axis=1)
        self.bm = np.ascontiguousarray(bm)
        self.stream = c.b.stream
        c.garbage(self.bm, GARBAGE)
        a.adopt(["data", "parity"])
        a.put("bitmap", self.bm)
        self.d, self.p, self.d_bm = c.d, c.p, a["bitmap"]
        self.keep = (self.d.clone(), self.p.clone(), self.d_bm.clone(), self.bm.copy())


class ArenaOut(Out):
    """test_gpu_read.Out over an arena region of exactly n*length bytes; its
    'guards' are the 64 arena bytes either side, compared with the pristine copy."""

    def __init__(self, a: Arena, name, n, length, shift=0):
        start, end = a.regions[name]
        assert end - start == n * length, (name, end - start, n, length)
        self.a, self.n, self.length, self.span = a, n, length, (start - GUARD, end + GUARD)
        a.fill(name, SENTINEL)
        self.buf = a.buf[start - GUARD:end + GUARD]
        self.ptr = a.base + start + shift
        assert (a.base + start) % 16 == 0

    def guards_intact(self):
        torch = _torch()
        lo, hi = self.span
        p = self.a.pristine
        return (torch.equal(self.buf[:GUARD], p[lo:lo + GUARD]) and
                torch.equal(self.buf[-GUARD:], p[hi - GUARD:hi]))

    def all_sentinel(self):
        return bool((self.buf[GUARD:-GUARD] == SENTINEL).all())


def i32(t):
    return t.view(_torch().int32)


def arena_items(bm, k):
    """matrix_items' kinds from whatever the bitmap lost: a lost data block, a
    lost parity block, a present block of either kind, then every other lost
    block of the last stripe."""
    lost, pres = np.argwhere(bm == 0), np.argwhere(bm != 0)
    pick = [lost[lost[:, 1] < k][0], lost[lost[:, 1] >= k][0], pres[pres[:, 1] < k][0],
            pres[pres[:, 1] >= k][-1]]
    pick += [r for r in lost if r[0] == bm.shape[0] - 1]
    return np.array([(int(c) << 8) | int(i) for c, i in pick], np.uint32)


def arena_flips(c: Case):
    """matrix_flips at any block size.  Round 1: the first byte, the last byte
    (of a parity block) and one in the second half of a block, in three
    classes.  Round 2: a byte 17 from the end of the last data block."""
    k, m, nm, bs = c.k, c.m, c.k // c.m, c.bs
    j = m // 2
    return [[(0, 0, 0, 0x01), (1, k + m - 1, bs - 1, 0x80), (2, j + m * (nm - 1), bs // 2 + 5, 0x10)],
            [(0, k - 1, bs - 17, 0x04)]]


def unrecoverable(bm, k, m):
    """`bm` with class m-1 of stripe 1 having lost two data members."""
    bad = bm.copy()
    j = m - 1
    bad[1, :k][j::m] = 1
    bad[1, k + j] = 1
    bad[1, j] = bad[1, j + m] = 0
    return bad


# --------------------------------------------------------------------------
# Grid A: every call
# --------------------------------------------------------------------------
class Cell:
    """One (S, k, m, bs): the arena, the case in it and the plan of losses,
    updates, flips and read items, computed once; `run` is looped over the
    launch settings."""

    def __init__(self, gpu, oracle, S, k, m, bs, rng):
        torch = _torch()
        self.gpu, self.S, self.k, self.m, self.bs = gpu, S, k, m, bs
        nb = S * (k + m)
        self.bm = pattern(rng, S, k, m, "mixed")
        self.bad_bm = unrecoverable(self.bm, k, m)
        self.items = arena_items(self.bm, k)
        n = len(self.items)
        self.ranges = [("out_full", 0, bs), ("out_part", 16, bs - 32)]
        sets = [update_set(rng, S, k, m, kind) for kind in ("third", "interleaved")]
        self.list_bytes = gpu.device_list_bytes(S, k, m)
        self.work_bytes = gpu.locate_work_bytes(S, k, m)
        self.rscr_bytes = gpu.read_scratch_bytes(n)
        assert self.list_bytes == 4 * (1 + S * m) and self.work_bytes == 8 * nb
        sizes = [("data", S * k * bs, 64), ("parity", S * m * bs, 64), ("shadow", S * k * bs, 64)]
        sizes += [(f"new{t}", len(blocks) * bs, 64) for t, blocks in enumerate(sets)]
        sizes += [(f"uscr{t}", gpu.update_scratch_bytes(len(blocks)), 4)
                  for t, blocks in enumerate(sets)]
        sizes += [("scratch", nb, 1), ("bitmap", nb, 1), ("lbitmap", nb, 1), ("select", nb, 1),
                  ("flags", S * m, 1), ("mask", S * k, 1), ("status", 4, 4), ("count", 4, 4),
                  ("dwork", self.list_bytes, 4), ("digests", 8 * nb, 8), ("stored", 8 * nb, 8),
                  ("lwork", self.work_bytes, 8), ("items", 4 * n, 4),
                  ("out_full", n * bs, 16), ("out_part", n * (bs - 32), 16),
                  ("rscr", self.rscr_bytes, 4), ("bad", 4, 4)]
        edge = max(bs, 4096)
        self.a = a = Arena(Arena.room([(nbytes, al) for _, nbytes, al in sizes], edge), "cuda", edge)
        for name, nbytes, al in sizes:
            a.carve(name, nbytes, al)
        self.c = c = arena_case(gpu, oracle, a, S, k, m, bs)
        self.s = c.b.stream
        ref_d = c.ref_d.cpu().numpy()
        self.updates = []
        for t, blocks in enumerate(sets):
            fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
            self.updates.append((t, blocks, fresh) + expected(oracle, c, ref_d, blocks, fresh))
        self.ref_dig = ref_digests(c)
        a.put("stored", self.ref_dig)
        self.sel = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=(S, k + m))
        self.sel[0, 0], self.sel[S - 1, k + m - 1] = 1, 0
        lost = torch.from_numpy(self.bm == 0).to("cuda")
        self.erased_d = c.ref_d.clone()
        self.erased_d.view(S, k, bs)[lost[:, :k]] = 0
        self.erased_p = c.ref_p.clone()
        self.erased_p.view(S, m, bs)[lost[:, k:]] = 0
        self.payload = np.zeros((S * k, bs), np.uint8)  # the oracle's validation payload
        for q in range(S * k):
            oracle.write_validation_pattern(self.payload[q], bs, 77 + q)
        a.check(writable=[], what="after the setup")

    # ---- the test's own writes, adopted ----
    def damage(self, bm, value=0xA5):
        self.c.garbage(bm, value)
        self.a.adopt(["data", "parity"])

    def heal(self):
        self.c.restore()
        self.a.adopt(["data", "parity"])

    @contextlib.contextmanager
    def flipped(self, flips):
        with contextlib.ExitStack() as es:
            for cs, blk, byte, bit in flips:
                es.enter_context(Flip(self.c, cs, blk, byte, bit))
            self.a.adopt(["data", "parity"])
            yield
        self.a.adopt(["data", "parity"])

    def args(self):
        c = self.c
        return c.d, c.p, c.S, c.bs, c.k, c.m

    def status(self):
        return int(i32(self.a["status"]).item())

    # ---- the calls ----
    def fill_and_encode(self, what):
        torch, gpu, a, c = _torch(), self.gpu, self.a, self.c
        a.fill("data", 0x5A)
        assert gpu.fill_splitmix64(c.d, c.S, c.k * c.bs, SEED, self.s) == gpu.Status.SUCCESS
        assert torch.equal(c.d, c.ref_d), f"fill != oracle, {what}"
        a.check(writable=["data"], what=f"fill_splitmix64, {what}")
        a.fill("parity", 0xEE)
        assert gpu.encode(c.d, c.p, c.S, c.bs, c.k, c.m, self.s) == gpu.Status.SUCCESS
        assert torch.equal(c.p, c.ref_p), f"parity != oracle, {what}"
        a.check(writable=["parity"], what=f"encode, {what}")

    def decodes(self, what):
        """xec_decode under every tiling and xec_decode_per_stripe: lost data
        rebuilt, lost parity left as it was (parity is not writable)."""
        torch, gpu, a, c = _torch(), self.gpu, self.a, self.c
        h_bm = pinned(self.bm)
        for tiling in range(5):
            w = f"decode tiling {tiling}, {what}"
            assert gpu.set_decode_tiling(tiling) == gpu.Status.SUCCESS
            self.damage(self.bm)
            a.fill("scratch", 0x3C)
            assert gpu.decode(*self.args(), h_bm, a["scratch"], self.s) == gpu.Status.SUCCESS, w
            assert gpu.decode_tiling_used() in VALID_TILINGS, w
            assert torch.equal(c.d, c.ref_d), f"data != oracle, {w}"
            a.check(writable=["data", "scratch"], what=w)
        assert gpu.set_decode_tiling(0) == gpu.Status.SUCCESS
        self.damage(self.bm)
        a.fill("scratch", 0x3C)
        codes = np.full(c.S, 0xEE, np.uint8)
        assert gpu.decode_per_stripe(*self.args(), h_bm, a["scratch"], codes,
                                     self.s) == gpu.Status.SUCCESS, what
        assert not codes.any() and torch.equal(c.d, c.ref_d), f"decode_per_stripe, {what}"
        a.check(writable=["data", "scratch"], what=f"decode_per_stripe, {what}")
        self.heal()

    def device_decodes(self, what):
        torch, gpu, a, c = _torch(), self.gpu, self.a, self.c
        a.put("bitmap", self.bm)
        self.damage(self.bm)
        a.fill("status", 77)
        assert gpu.decode_device(*self.args(), a["bitmap"], a["status"], self.s) == gpu.Status.SUCCESS
        assert self.status() == 0 and torch.equal(c.d, c.ref_d), f"decode_device, {what}"
        a.check(writable=["data", "status"], what=f"decode_device, {what}")
        self.damage(self.bm)
        a.fill("status", 77)
        a.fill("dwork", 0x3C)
        assert gpu.decode_device_list(*self.args(), a["bitmap"], a["dwork"], self.list_bytes,
                                      a["status"], self.s) == gpu.Status.SUCCESS
        assert self.status() == 0 and torch.equal(c.d, c.ref_d), f"decode_device_list, {what}"
        a.check(writable=["data", "status", "dwork"], what=f"decode_device_list, {what}")
        self.heal()

    def repairs(self, what):
        gpu, a, c = self.gpu, self.a, self.c
        self.damage(self.bm)
        a.fill("scratch", 0x3C)
        st, _ = run_repair(gpu, c, self.bm, "host", scratch=a["scratch"])
        assert st == gpu.Status.SUCCESS, what
        c.assert_exact(f"after repair, {what}")
        a.check(writable=["data", "parity", "scratch"], what=f"repair, {what}")
        a.put("bitmap", self.bm)
        self.damage(self.bm)
        a.fill("status", 77)
        assert gpu.repair_device(*self.args(), a["bitmap"], a["status"], self.s) == gpu.Status.SUCCESS
        assert self.status() == 0, what
        c.assert_exact(f"after repair_device, {what}")
        a.check(writable=["data", "parity", "status"], what=f"repair_device, {what}")

    def scrub(self, what):
        """xec_verify into the arena's flags and count: (flagged classes, count)."""
        torch, gpu, a = _torch(), self.gpu, self.a
        a.fill("flags", 0xFF)
        a.fill("count", 77)
        assert gpu.verify(*self.args(), a["flags"], a["count"], self.s) == gpu.Status.SUCCESS, what
        flags = a["flags"]
        assert int(flags.max()) <= 1
        got = torch.nonzero(flags).flatten().tolist(), int(i32(a["count"]).item())
        a.check(writable=["flags", "count"], what=f"verify, {what}")
        return got

    def verifies(self, what):
        c = self.c
        assert self.scrub(what) == ([], 0), f"intact batch flagged, {what}"
        for flips in arena_flips(c):
            want = sorted({class_of(c, cs, blk) for cs, blk, _, _ in flips})
            assert len(want) == len(flips)
            with self.flipped(flips):
                assert self.scrub(what) == (want, len(want)), (what, flips)

    def updates_both(self, what):
        gpu, a, c = self.gpu, self.a, self.c
        S, k, bs = c.S, c.k, c.bs
        for t, blocks, fresh, exp_d, exp_p in self.updates:
            n = len(blocks)
            a.put(f"new{t}", fresh)
            a.fill(f"uscr{t}", 0x3C)
            assert gpu.update(c.d, c.p, a[f"new{t}"], S, bs, k, c.m, items_of(blocks), n,
                              a[f"uscr{t}"], a.size(f"uscr{t}"), self.s) == gpu.Status.SUCCESS, what
            assert_state(c, exp_d, exp_p, f"after update {t}, {what}")
            a.check(writable=["data", "parity", f"uscr{t}"], what=f"update {t}, {what}")
            self.heal()
            shadow = np.full((S, k, bs), 0xA5, np.uint8)
            mask = np.zeros((S, k), np.uint8)
            for q, (cs, i) in enumerate(blocks):
                shadow[cs, i] = fresh[q]
                mask[cs, i] = (1, 2, 255)[q % 3]
            a.put("shadow", shadow)
            a.put("mask", mask)
            assert gpu.update_device(c.d, c.p, a["shadow"], S, bs, k, c.m, a["mask"],
                                     self.s) == gpu.Status.SUCCESS, what
            assert_state(c, exp_d, exp_p, f"after update_device {t}, {what}")
            a.check(writable=["data", "parity"], what=f"update_device {t}, {what}")
            self.heal()

    def digests(self, what):
        gpu, a = self.gpu, self.a
        a.fill("digests", 0xA5)
        assert gpu.digest(*self.args(), a["digests"], None, self.s) == gpu.Status.SUCCESS
        assert np.array_equal(as_u64(a["digests"]), self.ref_dig.reshape(-1)), f"digests, {what}"
        a.check(writable=["digests"], what=f"digest of every block, {what}")
        a.put("select", self.sel)
        a.fill("digests", 0xA5)
        assert gpu.digest(*self.args(), a["digests"], a["select"], self.s) == gpu.Status.SUCCESS
        want = np.where(self.sel != 0, self.ref_dig, np.uint64(0xA5A5A5A5A5A5A5A5))
        assert np.array_equal(as_u64(a["digests"]), want.reshape(-1)), f"selected digests, {what}"
        a.check(writable=["digests"], what=f"digest of a selection, {what}")

    def locates(self, what):
        gpu, a, c = self.gpu, self.a, self.c
        flips = arena_flips(c)[0]
        want = expect_bitmap(c, [(cs, blk) for cs, blk, _, _ in flips])
        with self.flipped(flips):
            flagged = self.scrub(what)
            assert flagged[1] == len(flips)
            for flags in (None, a["flags"]):
                w = f"locate {'with' if flags is not None else 'without'} flags, {what}"
                a.fill("lbitmap", 0xA5)
                a.fill("count", 77)
                a.fill("lwork", 0x3C)
                assert gpu.locate(*self.args(), a["stored"], flags, a["lbitmap"], a["count"],
                                  a["lwork"], self.work_bytes, self.s) == gpu.Status.SUCCESS, w
                got = a["lbitmap"].cpu().numpy().reshape(c.S, c.k + c.m)
                assert np.array_equal(got, want), w
                assert int(i32(a["count"]).item()) == len(flips), w
                a.check(writable=["lbitmap", "count", "lwork"], what=w)

    def reads(self, what):
        gpu, a, c = self.gpu, self.a, self.c
        b = ArenaBatch(a, c, self.bm)
        items, n = self.items, len(self.items)
        a.put("items", items)
        for name, offset, length in self.ranges:
            w = f"{what} [{offset}, +{length})"
            out = ArenaOut(a, name, n, length)
            a.fill("rscr", 0x3C)
            assert host_read(gpu, b, items, offset, length, out,
                             scratch=(a["rscr"], self.rscr_bytes)) == gpu.Status.SUCCESS, w
            check_served(b, items, offset, length, out, "xec_read " + w)
            a.check(writable=[name, "rscr"], what="read " + w)
            out = ArenaOut(a, name, n, length)
            a.fill("status", 77)
            assert gpu.read_device(*self.args(), a["bitmap"], a["items"], n, offset, length,
                                   out.ptr, a["status"], self.s) == gpu.Status.SUCCESS, w
            assert self.status() == 0, w
            check_served(b, items, offset, length, out, "xec_read_device " + w)
            a.check(writable=[name, "status"], what="read_device " + w)
        self.heal()

    def erases(self, what):
        torch, gpu, a, c = _torch(), self.gpu, self.a, self.c
        a.put("bitmap", self.bm)
        assert gpu.erase(*self.args(), a["bitmap"], self.s) == gpu.Status.SUCCESS, what
        assert torch.equal(c.d, self.erased_d) and torch.equal(c.p, self.erased_p), f"erase, {what}"
        a.check(writable=["data", "parity"], what=f"erase, {what}")
        self.heal()

    def validations(self, what):
        """The validation payload over the data region's S*k blocks (its own
        shapes and alignments: test_validation_in_the_arena)."""
        gpu, a, c = self.gpu, self.a, self.c
        n = c.S * c.k
        a.fill("data", 0x5A)
        assert gpu.write_validation_pattern(c.d, n, c.bs, 77, self.s) == gpu.Status.SUCCESS, what
        assert np.array_equal(c.d.cpu().numpy().reshape(n, c.bs), self.payload), f"payload, {what}"
        a.check(writable=["data"], what=f"write_validation_pattern, {what}")
        a.fill("bad", 77)
        assert gpu.validate_blocks(c.d, n, c.bs, a["bad"], self.s) == gpu.Status.SUCCESS, what
        assert int(i32(a["bad"]).item()) == 0, what
        a.check(writable=["bad"], what=f"validate_blocks, {what}")
        self.heal()

    def refusals(self, what):
        """A batch no call may touch: the host forms return XEC_DECODE_FAILURE
        and write nothing; a device verdict of 3 or 4 leaves the status word
        (and the list scratch its check kernel fills) as the only change."""
        gpu, a, c = self.gpu, self.a, self.c
        St = gpu.Status
        bad, h_bad = self.bad_bm, pinned(self.bad_bm)
        self.damage(bad)
        a.put("bitmap", bad)
        for name in ("scratch", "dwork", "rscr"):
            a.fill(name, 0x3C)
        assert gpu.decode(*self.args(), h_bad, a["scratch"], self.s) == St.DECODE_FAILURE, what
        a.check(writable=[], what=f"decode refused, {what}")
        st, _ = run_repair(gpu, c, bad, "host", scratch=a["scratch"])
        assert st == St.DECODE_FAILURE, what
        a.check(writable=[], what=f"repair refused, {what}")
        a.fill("status", 77)
        assert gpu.decode_device(*self.args(), a["bitmap"], a["status"], self.s) == St.SUCCESS
        assert self.status() == 4, what
        a.check(writable=["status"], what=f"decode_device verdict 4, {what}")
        a.fill("status", 77)
        assert gpu.decode_device_list(*self.args(), a["bitmap"], a["dwork"], self.list_bytes,
                                      a["status"], self.s) == St.SUCCESS
        assert self.status() == 4, what
        a.check(writable=["status", "dwork"], what=f"decode_device_list verdict 4, {what}")
        a.fill("status", 77)
        assert gpu.repair_device(*self.args(), a["bitmap"], a["status"], self.s) == St.SUCCESS
        assert self.status() == 4, what
        a.check(writable=["status"], what=f"repair_device verdict 4, {what}")
        # reads: a lost block of the broken class is not servable, stripe S does not exist
        n, (name, offset, length) = len(self.items), self.ranges[1]
        for verdict, item in ((4, (1 << 8) | (c.m - 1)), (3, c.S << 8)):
            items = self.items.copy()
            items[n - 1] = item
            out = ArenaOut(a, name, n, length)
            refused = St.DECODE_FAILURE if verdict == 4 else St.INVALID_COUNTS
            assert gpu.read(*self.args(), bad.reshape(-1), items, n, offset, length, out.ptr,
                            a["rscr"], self.rscr_bytes, self.s) == refused, what
            a.check(writable=[], what=f"read refused ({verdict}), {what}")
            a.put("items", items)
            a.fill("status", 77)
            assert gpu.read_device(*self.args(), a["bitmap"], a["items"], n, offset, length,
                                   out.ptr, a["status"], self.s) == St.SUCCESS, what
            assert self.status() == verdict and out.all_sentinel(), what
            a.check(writable=["status"], what=f"read_device verdict {verdict}, {what}")
        self.heal()

    def run(self, what):
        self.fill_and_encode(what)
        self.decodes(what)
        self.device_decodes(what)
        self.repairs(what)
        self.verifies(what)
        self.updates_both(what)
        self.digests(what)
        self.locates(what)
        self.reads(what)
        self.erases(what)
        self.validations(what)
        self.refusals(what)
        self.c.assert_exact(f"at the end of {what}")
        self.a.check(writable=[], what=f"at the end of {what}")


@gpu_test
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", KMS)
def test_every_call_in_the_arena(gpu, oracle, k, m, bs):
    """Grid A: every entry point at the default launch and at unroll 2, a grid
    of 2 workgroups, 256 threads and the cell's cache policy; encode and the
    decodes once more under rotation 3."""
    ci = cell_index(k, m, bs)
    cell = Cell(gpu, oracle, S_A, k, m, bs, np.random.default_rng(4000 + ci))
    policy = cache_policy_for(ci)
    try:
        cell.run(f"{k}+{m} x {bs} default launch")
        set_shape(gpu, unroll=2, max_grid=2, cache_policy=policy, block_threads=256)
        cell.run(f"{k}+{m} x {bs} unroll=2 max_grid=2 policy={policy} threads=256")
        set_shape(gpu, rotation=3)
        what = f"{k}+{m} x {bs} rotation=3"
        cell.fill_and_encode(what)
        cell.decodes(what)
        cell.device_decodes(what)
        cell.a.check(writable=[], what=f"at the end of {what}")
    finally:
        reset_overrides(gpu)
        gpu.set_decode_tiling(0)


# --------------------------------------------------------------------------
# Validation payload
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("bs,align", [(256, 16), (4224, 16), (100, 1), (15, 1)])
def test_validation_in_the_arena(gpu, oracle, bs, align):
    """xec_write_validation_pattern may write the blocks, xec_validate_blocks
    *d_bad, under every xec_set_validate_kernel mode: at 16 mod 32 where the
    grouped kernel applies (bs % 128 == 0), at an odd address where no
    alignment is required."""
    nblocks, seed = 5, 77
    edge = max(bs, 4096)
    a = Arena(Arena.room([(nblocks * bs, align), (4, 4)], edge), "cuda", edge)
    buf, bad = a.carve("blocks", nblocks * bs, align), a.carve("bad", 4, 4)
    assert buf.data_ptr() % 32 == 16 if align == 16 else buf.data_ptr() % 2 == 1
    s = _torch().cuda.current_stream()
    want = np.zeros((nblocks, bs), np.uint8)
    for b in range(nblocks):
        oracle.write_validation_pattern(want[b], bs, seed + b)
    try:
        for mode in (0, 1, 2):
            what = f"{nblocks} x {bs} validate kernel mode {mode}"
            assert gpu.set_validate_kernel(mode) == gpu.Status.SUCCESS
            a.fill("blocks", 0x5A)
            assert gpu.write_validation_pattern(buf, nblocks, bs, seed, s) == gpu.Status.SUCCESS
            assert np.array_equal(buf.cpu().numpy().reshape(nblocks, bs), want), what
            a.check(writable=["blocks"], what="write_validation_pattern, " + what)
            a.fill("bad", 77)
            assert gpu.validate_blocks(buf, nblocks, bs, bad, s) == gpu.Status.SUCCESS
            assert int(i32(bad).item()) == 0, what
            a.check(writable=["bad"], what="validate_blocks, " + what)
            buf[3 * bs + bs - 1] ^= 0x40  # the last payload byte of block 3
            a.adopt(["blocks"])
            a.fill("bad", 77)
            assert gpu.validate_blocks(buf, nblocks, bs, bad, s) == gpu.Status.SUCCESS
            host = buf.cpu().numpy().reshape(nblocks, bs)
            n_bad = int(i32(bad).item())
            assert n_bad == sum(not oracle.validate_block(host[b], bs) for b in range(nblocks)), what
            assert n_bad == 1 or bs < 16, what  # under 16 bytes there is no checksum to fail
            buf[3 * bs + bs - 1] ^= 0x40
            a.adopt(["blocks"])
            a.check(writable=["bad"], what="validate_blocks of a damaged block, " + what)
    finally:
        gpu.set_validate_kernel(0)


# --------------------------------------------------------------------------
# Grid B: the scratch uploads
# --------------------------------------------------------------------------
def one_loss_per_class(rng, S, k, m, data_only):
    bm = np.ones((S, k + m), np.uint8)
    nm = k // m
    for cs in range(S):
        for j in range(m):
            r = int(rng.integers(nm if data_only else nm + 1))
            bm[cs, k + j if r == nm else j + m * r] = 0
    return bm


@gpu_test
def test_scratch_uploads_in_the_arena(gpu, oracle):
    """Grid B: 1,100 stripes of 4+2 x 256 -- past 1,024 list entries and past
    the 1,024 stripes whose loss masks travel in the kernel arguments -- with
    exact-size scratch at minimum alignment.  The host forms run on an idle
    stream, where the lists are uploaded into the caller's scratch, and behind
    queued work, where xec_decode and xec_decode_per_stripe upload into the
    library's own buffers instead; the arena holds as declared on either route.

    xec_decode under tiling 3 uploads its list whole: it reports
    XEC_TILING_LIST where the list fits the route's buffer (include/xec.h: 'where
    the list fits, else the automatic bitmap choice').  The 2,200 entries of one
    lost data block per class do not fit the 6,600-byte scratch of the idle
    route (1,649 entries past the pad: measured there, tiling 3 reports 2,
    XEC_TILING_CLASS) and fit the library's buffer on the busy one; the 1,100
    entries of one lost data block per stripe fit both (measured: 3 on either).
    So XEC_TILING_LIST is asserted wherever the list fits, and the batch that
    fits runs beside the one that does not."""
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = B_S, B_K, B_M, B_BS
    nb = S * (k + m)
    rng = np.random.default_rng(77)
    bm_repair = one_loss_per_class(rng, S, k, m, data_only=False)
    bm_class = one_loss_per_class(rng, S, k, m, data_only=True)   # 2,200 lost data blocks
    bm_stripe = bm_class.copy()                                   # 1,100: class 0 only
    bm_stripe[:, 1:k:m] = 1
    bm_bad = bm_class.copy()                                      # stripe 550 cannot be rebuilt
    bm_bad[550, :k] = (0, 1, 0, 1)
    bm_read = pattern(rng, S, k, m, "mixed")
    assert int((bm_repair == 0).sum()) == 2200 == int((bm_class == 0).sum())
    assert int((bm_stripe == 0).sum()) == 1100
    q = np.sort(rng.permutation(S * k)[:1200])
    blocks = [divmod(int(x), k) for x in q]
    fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
    n_up, n_rd, rd_off, rd_len = len(blocks), 1200, 16, bs - 32
    up_bytes, rd_bytes = gpu.update_scratch_bytes(n_up), gpu.read_scratch_bytes(n_rd)
    list_bytes = gpu.device_list_bytes(S, k, m)
    sizes = [("data", S * k * bs, 64), ("parity", S * m * bs, 64), ("scratch", nb, 1),
             ("bitmap", nb, 1), ("new", n_up * bs, 64), ("uscr", up_bytes, 4),
             ("out", n_rd * rd_len, 16), ("rscr", rd_bytes, 4), ("dwork", list_bytes, 4),
             ("status", 4, 4)]
    a = Arena(Arena.room([(nbytes, al) for _, nbytes, al in sizes]), "cuda")
    for name, nbytes, al in sizes:
        a.carve(name, nbytes, al)
    assert a.ptr("scratch") % 2 == 1 and a.size("scratch") == 6600  # pad != 0: 1,649 entries a piece
    assert a.ptr("uscr") % 8 == 4 and a.ptr("dwork") % 8 == 4
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    c = arena_case(gpu, oracle, a, S, k, m, bs, stream=s)
    exp_d, exp_p = expected(oracle, c, c.ref_d.cpu().numpy(), blocks, fresh)
    a.put("new", fresh)
    busy_t = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (c.d, c.p, S, bs, k, m)
    stayed_busy = []
    # pinned once and kept: a host bitmap must stay as it is until the stream has passed the call
    h_repair, h_class, h_stripe, h_bad = (pinned(x) for x in (bm_repair, bm_class, bm_stripe, bm_bad))

    def damage(bm, value=0xA5):
        c.garbage(bm, value)
        a.adopt(["data", "parity"])

    def heal():
        c.restore()
        a.adopt(["data", "parity"])

    def queue_work(route):
        """The busy route: the call finds fills of 1 GiB queued ahead of it."""
        if route == "busy":
            for v in range(12):
                busy_t.fill_(v)

    def returned(route, call):
        """Whether the stream was still working when the call returned."""
        still = not s.query()
        if route == "busy":
            stayed_busy.append(still)
            print(f"{call}: stream still busy when the call returned: {still}")
        return still

    with torch.cuda.stream(s):
        for route in ("idle", "busy"):
            # xec_repair: 2,200 items through 6,600 bytes at an odd address, in two pieces
            damage(bm_repair)
            a.fill("scratch", 0x3C)
            queue_work(route)
            assert gpu.repair(*args, h_repair, a["scratch"], s) == St.SUCCESS
            assert gpu.repair_tiling_used() == LIST
            returned(route, "repair")
            c.assert_exact(f"after repair, {route}")
            a.check(writable=["data", "parity", "scratch"], what=f"repair, {route}")
            # xec_update: 1,200 items through exactly update_scratch_bytes at 4 mod 8
            a.fill("uscr", 0x3C)
            queue_work(route)
            assert gpu.update(c.d, c.p, a["new"], S, bs, k, m, items_of(blocks), n_up, a["uscr"],
                              up_bytes, s) == St.SUCCESS
            assert gpu.update_tiling_used() == LIST
            returned(route, "update")
            assert_state(c, exp_d, exp_p, f"after update, {route}")
            a.check(writable=["data", "parity", "uscr"], what=f"update, {route}")
            heal()
            # xec_read: 1,200 items, half of them lost, through exactly read_scratch_bytes
            b = ArenaBatch(a, c, bm_read)
            items = b.mixed_items(rng, n_rd)
            assert (bm_read[items >> 8, items & 0xFF] == 0).sum() > 100
            out = ArenaOut(a, "out", n_rd, rd_len)
            a.fill("rscr", 0x3C)
            queue_work(route)
            assert gpu.read(*args, bm_read.reshape(-1), items, n_rd, rd_off, rd_len, out.ptr,
                            a["rscr"], rd_bytes, s) == St.SUCCESS
            assert gpu.read_tiling_used() == LIST
            returned(route, "read")
            s.synchronize()
            check_served(b, items, rd_off, rd_len, out, f"xec_read, {route}")
            a.check(writable=["out", "rscr"], what=f"read, {route}")
            heal()
            # xec_decode and xec_decode_per_stripe under every tiling
            pad = (4 - a.ptr("scratch") % 4) % 4
            try:
                for tiling in range(5):
                    assert gpu.set_decode_tiling(tiling) == St.SUCCESS
                    for losses, bm, h_bm in (("class", bm_class, h_class), ("stripe", bm_stripe, h_stripe)):
                        w = f"tiling {tiling}, one lost data block per {losses}, {route}"
                        n_lost = int((bm == 0).sum())
                        damage(bm)
                        a.fill("scratch", 0x3C)
                        queue_work(route)
                        assert gpu.decode(*args, h_bm, a["scratch"], s) == St.SUCCESS, w
                        used = gpu.decode_tiling_used()
                        still = returned(route, "decode " + w)
                        assert used in VALID_TILINGS, w
                        if tiling == 3 and (still or 4 * n_lost <= nb - pad):
                            assert used == LIST, w
                        c.assert_exact(f"after decode, {w}")
                        a.check(writable=["data", "scratch"], what="decode " + w)
                    w = f"tiling {tiling}, {route}"
                    damage(bm_class)
                    a.fill("scratch", 0x3C)
                    codes = np.full(S, 0xEE, np.uint8)
                    queue_work(route)
                    assert gpu.decode_per_stripe(*args, h_class, a["scratch"], codes,
                                                 s) == St.SUCCESS, w
                    assert gpu.decode_tiling_used() == LIST, w
                    returned(route, "decode_per_stripe " + w)
                    assert not codes.any(), w
                    c.assert_exact(f"after decode_per_stripe, {w}")
                    a.check(writable=["data", "scratch"], what="decode_per_stripe " + w)
            finally:
                gpu.set_decode_tiling(0)
            # one unrecoverable stripe: verdict 4, the others rebuilt, that one untouched
            damage(bm_bad)
            a.fill("scratch", 0x3C)
            codes = np.full(S, 0xEE, np.uint8)
            want_d = c.ref_d.clone()
            want_d.view(S, k, bs)[550] = c.d.view(S, k, bs)[550]
            want_codes = np.zeros(S, np.uint8)
            want_codes[550] = 4
            queue_work(route)
            assert gpu.decode_per_stripe(*args, h_bad, a["scratch"], codes,
                                         s) == St.DECODE_FAILURE
            assert gpu.decode_tiling_used() == LIST
            returned(route, "decode_per_stripe with a bad stripe")
            s.synchronize()
            assert np.array_equal(codes, want_codes), route
            assert torch.equal(c.d, want_d), f"decode_per_stripe with a bad stripe, {route}"
            a.check(writable=["data", "scratch"], what=f"decode_per_stripe, a bad stripe, {route}")
            heal()
        # xec_decode_device_list: d_work of exactly its bytes at 4 mod 8 (no host work: once)
        damage(bm_class)
        a.put("bitmap", bm_class)
        a.fill("dwork", 0x3C)
        a.fill("status", 77)
        assert gpu.decode_device_list(*args, a["bitmap"], a["dwork"], list_bytes, a["status"],
                                      s) == St.SUCCESS
        assert int(i32(a["status"]).item()) == 0
        c.assert_exact("after decode_device_list")
        a.check(writable=["data", "status", "dwork"], what="decode_device_list")
        a.check(writable=[], what="at the end")
    torch.cuda.synchronize()
    assert any(stayed_busy), "no call of the busy route found its stream busy"
    del busy_t
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------
# Grid C: touching is not overlapping
# --------------------------------------------------------------------------
@gpu_test
def test_touching_is_not_overlapping(gpu, oracle):
    """d_new flush after the end of data and flush before the start of parity,
    d_out flush after the end of parity and ending exactly where data starts:
    accepted, exact, nothing else written.  One alignment unit further -- 64
    bytes for d_new, 16 for d_out -- the ranges overlap: XEC_INVALID_SIZE and
    not a byte changes.  Layout, each flush against the next:
        out_b | data | new_a        new_b | parity | out_a"""
    St = gpu.Status
    S, (k, m), bs = S_A, KMS[1], BSS[1]
    n_rd, rd_off, rd_len = 7, 16, bs - 48  # 7 * 1232 = 48 mod 128: out_b ends at 64 mod 128
    rng = np.random.default_rng(9)
    blocks = update_set(rng, S, k, m, "interleaved")
    n_up = len(blocks)
    fresh = rng.integers(0, 256, size=(n_up, bs), dtype=np.uint8)
    bm = pattern(rng, S, k, m, "mixed")
    edge = max(bs, 4096)
    shadow_bytes = S * k * bs
    a = Arena(Arena.room([(n_rd * rd_len, 128), (S * k * bs, 64), (shadow_bytes, 64),
                          (shadow_bytes, 64), (S * m * bs, 64), (n_rd * rd_len, 16),
                          (S * (k + m), 1), (S * k, 1), (4 * n_rd, 4), (4, 4)], edge), "cuda", edge)
    a.carve("out_b", n_rd * rd_len, 16, modulus=128)
    a.carve("data", S * k * bs, 64, gap=0)
    a.carve("new_a", shadow_bytes, 64, gap=0)
    a.carve("new_b", shadow_bytes, 64)
    a.carve("parity", S * m * bs, 64, gap=0)
    a.carve("out_a", n_rd * rd_len, 16, gap=0)
    a.carve("bitmap", S * (k + m), 1)
    a.carve("mask", S * k, 1)
    a.carve("items", 4 * n_rd, 4)
    a.carve("status", 4, 4)
    assert a.ptr("out_b") + a.size("out_b") == a.ptr("data") and a.ptr("data") % 128 == 64
    assert a.ptr("data") + a.size("data") == a.ptr("new_a")
    assert a.ptr("new_b") + a.size("new_b") == a.ptr("parity")
    assert a.ptr("parity") + a.size("parity") == a.ptr("out_a")
    c = arena_case(gpu, oracle, a, S, k, m, bs)
    s = c.b.stream
    args = (c.d, c.p, S, bs, k, m)
    exp_d, exp_p = expected(oracle, c, c.ref_d.cpu().numpy(), blocks, fresh)
    shadow = np.full((S, k, bs), 0xA5, np.uint8)
    mask = np.zeros((S, k), np.uint8)
    for t, (cs, i) in enumerate(blocks):
        shadow[cs, i] = fresh[t]
        mask[cs, i] = 1
    a.put("mask", mask)
    packed = np.full(shadow_bytes, 0xA5, np.uint8)

    def heal():
        c.restore()
        a.adopt(["data", "parity"])

    # d_new: (region, where the host form's n_up packed blocks start in it, the step into the neighbour)
    for name, at, step in (("new_a", 0, -64), ("new_b", shadow_bytes - n_up * bs, 64)):
        packed[:] = 0xA5
        packed[at:at + n_up * bs] = fresh.reshape(-1)
        a.put(name, packed)
        d_new = a.ptr(name) + at
        assert d_new == a.ptr("data") + a.size("data") or d_new + n_up * bs == a.ptr("parity")
        w = f"update with d_new in {name}"
        assert gpu.update(c.d, c.p, d_new, S, bs, k, m, items_of(blocks), n_up, None, 0,
                          s) == St.SUCCESS, w
        assert_state(c, exp_d, exp_p, w)
        a.check(writable=["data", "parity"], what=w)
        heal()
        assert gpu.update(c.d, c.p, d_new + step, S, bs, k, m, items_of(blocks), n_up, None, 0,
                          s) == St.INVALID_SIZE, w
        assert gpu.update_tiling_used() == 0
        a.check(writable=[], what=w + ", one unit into the neighbour")
        a.put(name, shadow)
        w = f"update_device with d_new in {name}"
        assert gpu.update_device(c.d, c.p, a.ptr(name), S, bs, k, m, a["mask"], s) == St.SUCCESS, w
        assert_state(c, exp_d, exp_p, w)
        a.check(writable=["data", "parity"], what=w)
        heal()
        assert gpu.update_device(c.d, c.p, a.ptr(name) + step, S, bs, k, m, a["mask"],
                                 s) == St.INVALID_SIZE, w
        a.check(writable=[], what=w + ", one unit into the neighbour")
    # d_out
    b = ArenaBatch(a, c, bm)
    items = np.resize(arena_items(bm, k), n_rd).astype(np.uint32)
    a.put("items", items)
    for name, step in (("out_a", -16), ("out_b", 16)):
        out = ArenaOut(a, name, n_rd, rd_len)
        w = f"read with d_out in {name}"
        assert host_read(gpu, b, items, rd_off, rd_len, out, scratch=(None, 0)) == St.SUCCESS, w
        check_served(b, items, rd_off, rd_len, out, w)
        a.check(writable=[name], what=w)
        out = ArenaOut(a, name, n_rd, rd_len)
        a.fill("status", 77)
        w = f"read_device with d_out in {name}"
        assert gpu.read_device(*args, a["bitmap"], a["items"], n_rd, rd_off, rd_len, out.ptr,
                               a["status"], s) == St.SUCCESS, w
        assert int(i32(a["status"]).item()) == 0
        check_served(b, items, rd_off, rd_len, out, w)
        a.check(writable=[name, "status"], what=w)
        moved = ArenaOut(a, name, n_rd, rd_len, shift=step)
        a.fill("status", 77)
        assert host_read(gpu, b, items, rd_off, rd_len, moved, scratch=(None, 0)) == St.INVALID_SIZE
        assert gpu.read_device(*args, a["bitmap"], a["items"], n_rd, rd_off, rd_len, moved.ptr,
                               a["status"], s) == St.INVALID_SIZE
        assert gpu.read_tiling_used() == 0
        a.check(writable=[], what=f"d_out in {name}, one unit into the neighbour")
    heal()
    a.check(writable=[], what="at the end")


# --------------------------------------------------------------------------
# The host pipeline in a host arena
# --------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("S,k,m,bs,chunk,ns", [(10, 4, 2, 4096, 3, 2), (3, 4, 2, 1 << 20, 1, 2)],
                         ids=["4KiB", "1MiB"])
def test_pipeline_in_a_host_arena(gpu, oracle, S, k, m, bs, chunk, ns, pin):
    """xec_pipeline_encode may write h_parity only, xec_pipeline_decode h_data
    only (present blocks keep their bytes: the result is the oracle's data);
    h_parity and the bitmap stay as they were.  Blocks below and at
    kWholeCopyBelowBytes (csrc/xec_pipeline.cpp): both copy routes."""
    edge = max(bs, 4096)
    sizes = [("h_data", S * k * bs, 64), ("h_parity", S * m * bs, 64), ("h_bitmap", S * (k + m), 1)]
    a = Arena(Arena.room([(nbytes, al) for _, nbytes, al in sizes], edge), "cpu", edge, pin=pin)
    assert a.buf.is_pinned() == pin
    for name, nbytes, al in sizes:
        a.carve(name, nbytes, al)
    assert a.ptr("h_data") % 128 == 64 and a.ptr("h_parity") % 128 == 64
    ref_d, ref_p = oracle.batch(S, k, m, bs, seed_base=8800 + S)
    a.put("h_data", ref_d)
    bm = np.ones((S, k + m), np.uint8)
    for c in range(0, S, 2):  # two data blocks (one a class) in every other stripe
        bm[c, c % k] = bm[c, (c + 1) % k] = 0
    a.put("h_bitmap", bm)
    with gpu.Pipeline(chunk, bs, k, m, ns) as pl:
        a.fill("h_parity", 0xEE)
        assert pl.encode(a["h_data"], a["h_parity"], S) == gpu.Status.SUCCESS
        assert np.array_equal(a["h_parity"].numpy(), ref_p), "parity != oracle"
        a.check(writable=["h_parity"], what="pipeline encode")
        a["h_data"].numpy().reshape(S, k, bs)[bm[:, :k] == 0] = 0xA5
        a.adopt(["h_data"])
        assert pl.decode(a["h_data"], a["h_parity"], S, a["h_bitmap"]) == gpu.Status.SUCCESS
        assert np.array_equal(a["h_data"].numpy(), ref_d), "data != oracle"
        a.check(writable=["h_data"], what="pipeline decode")
        # an unrecoverable batch: nothing at all is written
        bad = bm.copy()
        bad[1, 0] = bad[1, m] = 0
        a.put("h_bitmap", bad)
        assert pl.decode(a["h_data"], a["h_parity"], S, a["h_bitmap"]) == gpu.Status.DECODE_FAILURE
        a.check(writable=[], what="pipeline decode refused")
