"""xec_write_shards_device on an MI355X: the degraded write over one buffer per
shard, list, bitmap and new bytes on the device.

Every expectation is built in numpy from the PRISTINE blocks of
test_gpu_read.Batch (parity by numpy): `final` is the pristine data with the
ranges patched and the parity re-encoded by numpy -- what the store holds once a
repair has run -- and `held` is what the write itself must leave: the written
present blocks patched, the parity range of every delta and rebuild-write class
taken from `final`, everything else as it was.  The loss patterns, the modes and
the digest slots a call may touch are test_gpu_write's (pattern, modes_of,
touched_slots, stale_parity_slots).  The store is one of the three placements of
tests/test_gpu_shards.py; lost blocks hold GARBAGE before a call and must hold it
afterwards, and after every call each allocation is compared as a whole with the
expected image -- blocks, gaps between blocks and guards.  d_new sits at its
minimum alignment (+16 in a 64-aligned buffer) between two guards of 0xA5 and is
compared as a whole too.  Digest slots the call may touch, and the parity slots
of data-only classes, start as the digests of the pristine blocks, every other
slot as a sentinel; afterwards a touched slot equals xec.digest_host of the
block in `final` and every other slot is bit-identical.
"""
from __future__ import annotations

import types

import numpy as np
import pytest

from test_gpu_read import GUARD, SENTINEL
from test_gpu_shards import (PLACEMENTS, POLICIES, SHAPES, Layout, Store, describe, device_bitmap,
                             poison, pristine)
from test_gpu_update import items_of
from test_gpu_update_range import ranges_of
from test_gpu_write import BS, KM, PATTERNS, modes_of, pattern, stale_parity_slots, touched_slots

pytestmark = pytest.mark.gpu

STRIPES = {(3, 3): 11, (6, 3): 7, (8, 1): 5, (9, 1): 4, (66, 2): 3}  # (k, m) -> S, 3 to 11
NEW_FILL = 0xA5


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def tiling_diagnostics_left_at_zero():
    """The batch-parity case runs xec_write, xec_update_range and xec_update; a
    call with nothing to do puts their *_tiling_used back to 0, which the ABI
    tests that run later in the same process ask of the main thread."""
    yield
    import xec
    xec.update_range(0, 0, 0, 0, 256, 1, 1, None, 0, 0, 16)
    xec.write(0, 0, 0, 0, 256, 1, 1, None, None, 0, 0, 16)
    assert xec.update_tiling_used() == 0 and xec.write_tiling_used() == 0


def ns(S, k, m):
    return types.SimpleNamespace(S=S, k=k, m=m)


def image_of(lay: Layout, blocks, bm=None):
    """lay.image without its cache, which is keyed by id(blocks): the arrays of
    this file are short-lived."""
    lay.images.clear()
    img = lay.image(blocks, bm)
    lay.images.clear()
    return img


def model(blocks, k, m, bm, written, fresh, off, ln):
    """(held, final) as the module docstring defines them; (S, k+m, bs) each."""
    S, _, bs = blocks.shape
    final = blocks.copy()
    for t, (c, i) in enumerate(written):
        final[c, i, off:off + ln] = fresh[t]
    final[:, k:] = np.bitwise_xor.reduce(final[:, :k].reshape(S, k // m, m, bs), axis=1)
    held = blocks.copy()
    for t, (c, i) in enumerate(written):
        held[c, i, off:off + ln] = fresh[t]
    for (c, j), mode in modes_of(ns(S, k, m), bm, written).items():
        if mode != "data":
            held[c, k + j, off:off + ln] = final[c, k + j, off:off + ln]
    return held, final


class New:
    """The new bytes packed in list order at +16 of a 64-aligned buffer, between
    two guards, NEW_FILL wherever the call must not read."""

    def __init__(self, fresh, pad=0):
        torch = _torch()
        body = np.ascontiguousarray(fresh).reshape(-1)
        self.host = np.full(GUARD + 16 + body.size + pad + GUARD, NEW_FILL, np.uint8)
        self.host[GUARD + 16:GUARD + 16 + body.size] = body
        self.buf = torch.from_numpy(self.host).to("cuda")
        assert self.buf.data_ptr() % 64 == 0
        self.ptr = self.buf.data_ptr() + GUARD + 16

    def intact(self):
        return np.array_equal(self.buf.cpu().numpy(), self.host)


def sentinel_slots(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(0x0101010101010101)) ^ np.uint64(
        0xA5A5A5A5A5A5A5A5)


def digests_of(xec, blocks, slots):
    row = blocks.shape[1]
    return {b: xec.digest_host(np.ascontiguousarray(blocks[b // row, b % row])) for b in slots}


def seed_slots(xec, blocks, k, m, bm, written):
    S = blocks.shape[0]
    c = ns(S, k, m)
    h = sentinel_slots(S * (k + m))
    which = touched_slots(c, bm, written) + stale_parity_slots(c, bm, written)
    for b, v in digests_of(xec, blocks, which).items():
        h[b] = np.uint64(v)
    return h


def want_slots(xec, seeded, final, k, m, bm, written):
    want = seeded.copy()
    c = ns(final.shape[0], k, m)
    for b, v in digests_of(xec, final, touched_slots(c, bm, written)).items():
        want[b] = np.uint64(v)
    return want


def d_u64(h):
    return _torch().from_numpy(h.view(np.uint8).copy()).to("cuda")


def as_u64(t):
    return t.cpu().numpy().view("<u8")


def d_u32(items):
    return _torch().from_numpy(np.ascontiguousarray(items, dtype=np.uint32).view(np.int32)).to("cuda")


def shard_write(xec, st: Store, d_bm, items, off, ln, new_ptr, d_dig=None, status=None,
                stream=None):
    """(status code, *d_status) of one xec_write_shards_device."""
    if status is None:
        status = poison()
    code = xec.write_shards_device(*st.args, d_bm, d_u32(items), len(items), off, ln, new_ptr,
                                   d_dig, status, stream)
    _torch().cuda.synchronize()
    return code, int(status.item())


def check_write(xec, st: Store, blocks, bm, written, fresh, off, ln, upkeep, what):
    """One call from the pristine store with the lost blocks garbled: every
    allocation, d_new, the bitmap and (with upkeep) every digest slot.  Returns
    (held, final, device digests or None)."""
    lay = st.lay
    k, m = lay.k, lay.m
    st.load(image_of(lay, blocks, bm))
    held, final = model(blocks, k, m, bm, written, fresh, off, ln)
    new = New(fresh)
    d_bm = None if bm is None else device_bitmap(bm)
    seeded = d_dig = None
    if upkeep:
        seeded = seed_slots(xec, blocks, k, m, bm, written)
        d_dig = d_u64(seeded)
    assert shard_write(xec, st, d_bm, items_of(written), off, ln, new.ptr,
                       d_dig) == (xec.Status.SUCCESS, 0), what
    assert xec.shards_arg_capacity_used() == (64 if k + m <= 64 else 256), what
    st.assert_image(image_of(lay, held, bm), what)
    assert new.intact(), f"{what}: d_new or its guards were written"
    if bm is not None:
        assert np.array_equal(d_bm.cpu().numpy(), bm.reshape(-1)), f"{what}: bitmap written"
    if upkeep:
        want = want_slots(xec, seeded, final, k, m, bm, written)
        bad = np.flatnonzero(as_u64(d_dig) != want)
        assert bad.size == 0, f"{what}: slots {bad[:8].tolist()}"
    return held, final, d_dig


# -- 1. three modes, bit exact ------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_three_modes_bit_exact(gpu, k, m, bs, placement):
    S = STRIPES[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, image_of(lay, blocks))
    rng = np.random.default_rng(k * 1000 + m * 10 + bs)
    seen = set()
    for off, ln in ranges_of(bs):
        for kind in PATTERNS:
            bm, written, _ = pattern(kind, S, k, m)
            seen |= set(modes_of(ns(S, k, m), bm, written).values())
            fresh = rng.integers(0, 256, size=(len(written), ln), dtype=np.uint8)
            for upkeep in (False, True):
                check_write(gpu, st, blocks, bm, written, fresh, off, ln, upkeep,
                            f"'{kind}' [{off},+{ln}) upkeep={upkeep} "
                            + describe(k, m, bs, S, placement))
    assert seen == {"delta", "data", "rebuild"}


# -- 2. batch parity of bytes ----------------------------------------------------------------
@pytest.mark.parametrize("k,m,bs", [(6, 3, 4352), (9, 1, 1280), (66, 2, 256)])
def test_aliased_into_a_batch_it_leaves_the_batch_calls_bytes_and_slots(gpu, k, m, bs):
    """Placement A: xec_write on a copy of the batch; with a NULL bitmap
    xec_update_range; with offset = 0, len = bs and no digests xec_update."""
    torch = _torch()
    S = STRIPES[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "A")
    st = Store(lay, image_of(lay, blocks))
    d_off, p_off = lay.batch_offsets
    rng = np.random.default_rng(k + m + bs)
    scratch = torch.empty(4096, dtype=torch.uint8, device="cuda")
    St = gpu.Status
    for off, ln in [(0, bs), (bs - 16, 16)] + ([(1008, 2064)] if bs >= 4352 else []):
        for kind in PATTERNS:
            bm, written, _ = pattern(kind, S, k, m)
            n = len(written)
            fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
            what = f"'{kind}' [{off},+{ln}) {k}+{m} x {bs}"
            for upkeep in (False, True):
                _, _, d_dig = check_write(gpu, st, blocks, bm, written, fresh, off, ln, upkeep, what)
                copy = torch.from_numpy(image_of(lay, blocks, bm)[0]).to("cuda")
                base = copy.data_ptr()
                assert base % 64 == 0
                dig2 = d_u64(seed_slots(gpu, blocks, k, m, bm, written)) if upkeep else None
                new = New(fresh)
                flat = None if bm is None else np.ascontiguousarray(bm.reshape(-1))
                assert gpu.write(base + d_off, base + p_off, new.ptr, S, bs, k, m, flat,
                                 items_of(written), n, off, ln, dig2, scratch, 4096) == St.SUCCESS
                torch.cuda.synchronize()
                assert torch.equal(copy, st.t[0]), "xec_write, " + what
                if upkeep:
                    assert torch.equal(dig2, d_dig), "xec_write's slots, " + what
                if bm is not None:
                    continue
                copy.copy_(torch.from_numpy(image_of(lay, blocks)[0]))
                dig3 = d_u64(seed_slots(gpu, blocks, k, m, bm, written)) if upkeep else None
                assert gpu.update_range(base + d_off, base + p_off, new.ptr, S, bs, k, m,
                                        items_of(written), n, off, ln, dig3, scratch,
                                        4096) == St.SUCCESS
                torch.cuda.synchronize()
                assert torch.equal(copy, st.t[0]), "xec_update_range, " + what
                if upkeep:
                    assert torch.equal(dig3, d_dig), "xec_update_range's slots, " + what
                if (off, ln) != (0, bs) or upkeep:
                    continue
                copy.copy_(torch.from_numpy(image_of(lay, blocks)[0]))
                whole = torch.from_numpy(np.ascontiguousarray(fresh).reshape(-1)).to("cuda")
                assert gpu.update(base + d_off, base + p_off, whole, S, bs, k, m, items_of(written),
                                  n, scratch, 4096) == St.SUCCESS
                torch.cuda.synchronize()
                assert torch.equal(copy, st.t[0]), "xec_update, " + what


# -- 3. list edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_list_edges(gpu, placement):
    S, k, m, bs = 5, 6, 2, 1280
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, image_of(lay, blocks))
    rng = np.random.default_rng(23)
    ones = np.ones((S, k + m), np.uint8)

    def lost(*at):
        bm = ones.copy()
        for c, x in at:
            bm[c, x] = 0
        return bm

    cases = [
        ("one item, present", lost((2, 1)), [(2, 3)]),
        ("one item, lost", lost((2, 3)), [(2, 3)]),
        ("one item, parity lost", lost((2, k + 1)), [(2, 3)]),
        ("one item, no bitmap", None, [(S - 1, k - 1)]),
        ("every member of a class, one lost", lost((1, 2)), [(1, 0), (1, 2), (1, 4)]),
        ("every member of both classes, one lost each", lost((1, 4), (1, 1)),
         [(1, i) for i in range(k)]),
        ("every member of a class, parity lost", lost((3, k)), [(3, 0), (3, 2), (3, 4)]),
        # the same class index in two consecutive stripes: (1, 0)'s item must not
        # be taken for an earlier owner of (2, 0)'s class, nor fold it
        ("one class in consecutive stripes", lost((2, 0)), [(1, 0), (2, 0)]),
        ("one class in consecutive stripes, modes apart", lost((1, k), (2, 2), (3, 4)),
         [(0, 4), (1, 0), (1, 4), (2, 0), (2, 2), (3, 2), (4, 0)]),
    ]
    for off, ln in [(0, bs), (1008, 48), (16, bs - 32)]:
        for name, bm, written in cases:
            fresh = rng.integers(0, 256, size=(len(written), ln), dtype=np.uint8)
            for upkeep in (False, True):
                check_write(gpu, st, blocks, bm, written, fresh, off, ln, upkeep,
                            f"{name} [{off},+{ln}) upkeep={upkeep} placement {placement}")


def test_a_list_past_every_argument_capacity(gpu):
    """About 1,100 items at 4+1 x 256 B x 300 stripes: the device list has no cap."""
    S, k, m, bs = 300, 4, 1, 256
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    st = Store(lay, image_of(lay, blocks))
    rng = np.random.default_rng(300)
    bm = np.ones((S, k + m), np.uint8)
    for c in range(S):
        r = int(rng.integers(8))
        if r <= k:  # one loss per stripe at most, data or parity: every item is servable
            bm[c, r] = 0
    written = [(c, i) for c in range(S) for i in range(k) if rng.random() < 0.92]
    assert len(written) > 1024
    md = set(modes_of(ns(S, k, m), bm, written).values())
    assert md == {"delta", "data", "rebuild"}
    for off, ln, upkeep in [(0, bs, True), (16, 224, False)]:
        fresh = rng.integers(0, 256, size=(len(written), ln), dtype=np.uint8)
        check_write(gpu, st, blocks, bm, written, fresh, off, ln, upkeep,
                    f"{len(written)} items [{off},+{ln})")


# -- 4. verdicts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_verdicts_leave_everything_as_it_was(gpu, placement):
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 5, 6, 2, 1280
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    bm = np.ones((S, k + m), np.uint8)
    bm[1, 1] = bm[1, k + 1] = 0  # class 1 of stripe 1 lost a member and its parity block
    bm[2, 0] = 0                 # a member lost alone: servable
    before = image_of(lay, blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    off, ln = 1008, 48
    far = (1 << 24) - 1
    good = [(0, 0), (1, 3), (2, 0), (4, 5)]  # (1, 3): a present member of the broken class
    lists = [
        (good[:1] + [(1, 1)] + good[1:], 4, "unservable"),
        ([(1, 1)], 4, "unservable alone"),
        ([(0, 0), (0, 0)], 3, "a repeat"),
        ([(2, 0), (0, 0)], 3, "disorder"),
        (good + [(4, 4)], 3, "disorder at the end"),
        ([(0, k)], 3, "i >= k"),
        ([(0, 0xFF)], 3, "i = 255"),
        ([(S, 0)], 3, "c >= S"),
        (good + [(far, 5)], 3, "c = 2^24 - 1"),
        ([(far, 0xFF)], 3, "the largest word"),
        ([(1, 1), (far, 0)], 4, "unservable and out of range"),
        ([(3, 0), (1, 1)], 4, "unservable and disorder in one item"),
        ([(1, 1), (1, 1), (0, 0)], 4, "unservable, a repeat and disorder"),
    ]
    for written, verdict, name in lists:
        n = len(written)
        new = New(np.full((n, ln), 0x11, np.uint8))
        seeded = sentinel_slots(S * (k + m))
        d_dig = d_u64(seeded)
        what = f"{name}, placement {placement}"
        assert shard_write(gpu, st, d_bm, items_of(written), off, ln, new.ptr,
                           d_dig) == (St.SUCCESS, verdict), what
        st.assert_image(before, what)
        assert new.intact() and np.array_equal(as_u64(d_dig), seeded), what
        assert np.array_equal(d_bm.cpu().numpy(), bm.reshape(-1)), what
    # without a bitmap the order rule and the ranges still hold, and nothing else
    for written, verdict in [([(2, 0), (0, 0)], 3), ([(far, 0)], 3), ([(0, 0), (0, 0)], 3)]:
        new = New(np.full((len(written), ln), 0x11, np.uint8))
        assert shard_write(gpu, st, None, items_of(written), off, ln, new.ptr) == (St.SUCCESS,
                                                                                  verdict)
        st.assert_image(before, f"no bitmap, verdict {verdict}, placement {placement}")
    torch.cuda.synchronize()


# -- 5. every launch shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(8, 1), (9, 1), (6, 3)])
def test_every_launch_shape(gpu, k, m):
    """Every (threads, unroll), both cache policies, the default grid and a grid of
    two workgroups striding over the tiles, in the placement with two different
    strides: the bytes and slots of the numpy model each time."""
    S, bs = STRIPES[(k, m)], 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    st = Store(lay, image_of(lay, blocks))
    rng = np.random.default_rng(k + m)
    work = []
    for kind in ("mixed", "lost_between"):
        bm, written, _ = pattern(kind, S, k, m)
        for off, ln in [(1008, 2064), (0, bs)]:
            work.append((kind, bm, written, off, ln,
                         rng.integers(0, 256, size=(len(written), ln), dtype=np.uint8)))
    try:
        for threads, unroll in SHAPES:
            for policy in POLICIES:
                for max_grid in (0, 2):
                    assert gpu.set_launch(unroll, max_grid, policy, threads) == gpu.Status.SUCCESS
                    for kind, bm, written, off, ln, fresh in work:
                        for upkeep in (False, True):
                            check_write(gpu, st, blocks, bm, written, fresh, off, ln, upkeep,
                                        f"{k}+{m} '{kind}' threads={threads} unroll={unroll} "
                                        f"policy={policy} max_grid={max_grid} [{off},+{ln}) "
                                        f"upkeep={upkeep}")
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(3) == gpu.Status.SUCCESS  # plays no part
        kind, bm, written, off, ln, fresh = work[0]
        check_write(gpu, st, blocks, bm, written, fresh, off, ln, True, "under a rotation")
    finally:
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(0) == gpu.Status.SUCCESS


# -- 6. the check order -------------------------------------------------------------------------------------
def test_every_check_in_order(gpu):
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 5, 4, 1, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    bm = np.ones((S, k + m), np.uint8)
    bm[0, 0] = bm[S - 1, k] = 0
    before = image_of(lay, blocks, bm)
    st = Store(lay, before)
    ptrs, ds, ps = st.ptrs, lay.ds, lay.ps
    d_bm, status = device_bitmap(bm), poison()
    written = [(0, 0), (1, 3), (S - 1, k - 1)]
    d_ok = d_u32(items_of(written))
    new = New(np.full((3, 256), 0x11, np.uint8))
    seeded = sentinel_slots(S * (k + m))
    d_dig = d_u64(seeded)
    bad_table = [ptrs[0]] * (k + m)  # breaks the overlap rule wherever the table is reached
    skew_table = ptrs[:2] + [ptrs[2] + 16] + ptrs[3:]  # XEC_INVALID_ALIGNMENT once it is reached
    r0, o0 = lay.at(0, 0)
    base = st.t[r0].data_ptr()
    in_gap = base + o0 + bs  # the 64 bytes between blocks 0 and 1 of shard 0

    def dev(t=ptrs, a=ds, b=ps, SS=S, bb=bs, kk=k, mm=m, items=d_ok, n=3, off=0, ln=256,
            nw=new.ptr, dig=d_dig, stt=status):
        code = gpu.write_shards_device(t, a, b, SS, bb, kk, mm, d_bm, items, n, off, ln, nw, dig,
                                       stt)
        assert gpu.shards_arg_capacity_used() == 0
        return code

    # 2. bs, then k and m, before everything that follows
    assert dev(t=None, bb=100, kk=6, mm=4, stt=None) == St.INVALID_SIZE
    assert dev(t=bad_table, kk=6, mm=4, stt=None, ln=0) == St.INVALID_COUNTS
    # 3. d_status
    assert dev(t=bad_table, stt=None, ln=0, nw=None) == St.INVALID_ALIGNMENT
    assert dev(t=None, stt=status.data_ptr() + 2, n=0) == St.INVALID_ALIGNMENT
    for t in (ptrs, bad_table, skew_table, None):
        # 5. the packing
        assert dev(t=t, kk=255, mm=5, ln=0) == St.INVALID_SIZE
        assert dev(t=t, SS=(1 << 24) + 1, ln=0) == St.INVALID_SIZE
        # 6. the range
        for off, ln in [(0, 0), (8, 256), (0, 24), (bs - 16, 32), (bs, 16), (bs + 16, 16)]:
            assert dev(t=t, off=off, ln=ln, nw=None) == St.INVALID_SIZE, (off, ln)
        # 7. the pointers
        assert dev(t=t, nw=None, items=d_ok.data_ptr() + 2) == St.INVALID_SIZE
        assert dev(t=t, items=None, nw=new.ptr + 8) == St.INVALID_SIZE
        # 8. their alignment
        assert dev(t=t, nw=new.ptr + 8, n=(1 << 64) // 256) == St.INVALID_ALIGNMENT
        assert dev(t=t, items=d_ok.data_ptr() + 2, n=(1 << 64) // 256) == St.INVALID_ALIGNMENT
        assert dev(t=t, dig=d_dig.data_ptr() + 4, n=(1 << 64) // 256) == St.INVALID_ALIGNMENT
        # 9. n_items * len, ahead of the table
        assert dev(t=t, n=(1 << 64) // 256) == St.INVALID_SIZE
    # 10. steps 3 to 7 of xec_check_shards, ahead of the overlaps
    tables = [
        ((None, ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:2] + [None] + ptrs[3:], ds, ps, k, m), St.INVALID_SIZE),
        ((skew_table, ds, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, ds + 32, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, bs - 64, ps, k, m), St.INVALID_SIZE),
        ((ptrs, ds, 1 << 62, k, m), St.INVALID_SIZE),
        ((ptrs[:3] + [ptrs[0]] + ptrs[4:], ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:-1] + [ptrs[1] + 64], ds, ps, k, m), St.INVALID_SIZE),
    ]
    for (t, a, b, kk, mm), code in tables:
        assert gpu.check_shards(t, a, b, S, bs, kk, mm) == code
        assert dev(t=t, a=a, b=b, kk=kk, mm=mm, nw=in_gap) == code
    # 11. d_new and d_digests against the hulls and each other
    assert dev(nw=in_gap, n=1, ln=16) == St.INVALID_SIZE       # a gap between two blocks of a shard
    assert dev(nw=base + o0) == St.INVALID_SIZE                # a block
    assert dev(nw=base + o0 - 3 * 256 + 16) == St.INVALID_SIZE     # ends 16 bytes inside the hull
    assert dev(nw=base + o0 + lay.hull(0) - 16) == St.INVALID_SIZE  # starts in its last 16 bytes
    assert dev(dig=in_gap) == St.INVALID_SIZE
    assert dev(dig=base + o0 - 8) == St.INVALID_SIZE           # its last slot reaches a block
    assert dev(nw=d_dig.data_ptr()) == St.INVALID_SIZE         # d_new on d_digests
    last16 = (8 * S * (k + m) - 1) // 16 * 16  # the 16 bytes that hold d_digests' last byte
    assert dev(nw=d_dig.data_ptr() + last16, n=1, ln=16) == St.INVALID_SIZE
    torch.cuda.synchronize()
    # nothing was queued: not a byte, not even *d_status = 0
    assert int(status.item()) == 77
    st.assert_image(before, "after rejected calls")
    assert new.intact() and np.array_equal(as_u64(d_dig), seeded)
    # nothing to do: only the verdict is queued, whatever the table and the range
    assert dev(t=bad_table, n=0, items=None, nw=None, ln=0) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    status.fill_(77)
    assert dev(t=None, SS=0, off=8, nw=None) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    st.assert_image(before, "after empty writes")
    assert np.array_equal(as_u64(d_dig), seeded)
    # d_new may touch a hull: the 48 bytes that end exactly where shard 0 begins (SENTINEL,
    # a guard or the gap behind the neighbour below) are the new bytes of three items
    off, ln = bs - 16, 16
    fresh = np.full((3, ln), SENTINEL, np.uint8)
    held, _ = model(blocks, k, m, bm, written, fresh, off, ln)
    assert (before[r0][o0 - 48:o0] == SENTINEL).all()
    code = gpu.write_shards_device(*st.args, d_bm, d_ok, 3, off, ln, base + o0 - 48, None, status)
    assert code == St.SUCCESS and gpu.shards_arg_capacity_used() == 64
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    st.assert_image(image_of(lay, held, bm), "d_new touching a hull")


# -- 7. write, repair, locate ---------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_write_then_repair_then_a_full_locate(gpu, placement):
    """Slots that held the digests of the blocks before the loss: after the write
    and xec_repair_shards_device under the same bitmap, on one stream with one
    synchronisation, the store holds `final` and a full xec_locate_shards counts
    exactly the parity blocks of the data-only classes."""
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 7, 6, 2, 1280
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    bm, written, repairable = pattern("mixed", S, k, m)
    assert repairable
    off, ln = 1008, 48
    rng = np.random.default_rng(7)
    fresh = rng.integers(0, 256, size=(len(written), ln), dtype=np.uint8)
    _, final = model(blocks, k, m, bm, written, fresh, off, ln)
    st = Store(lay, image_of(lay, blocks, bm))
    n_slots = S * (k + m)
    full = np.array([v for _, v in sorted(digests_of(gpu, blocks, range(n_slots)).items())],
                    dtype=np.uint64)
    d_dig, d_bm = d_u64(full), device_bitmap(bm)
    new = New(fresh)
    w_status, r_status, count = poison(), poison(), poison()
    located = torch.full((n_slots,), 0xA5, dtype=torch.uint8, device="cuda")
    wb = gpu.locate_work_bytes(S, k, m)
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert gpu.write_shards_device(*st.args, d_bm, d_u32(items_of(written)), len(written), off,
                                       ln, new.ptr, d_dig, w_status, s) == St.SUCCESS
        assert gpu.repair_shards_device(*st.args, d_bm, r_status, s) == St.SUCCESS
        assert gpu.locate_shards(*st.args, d_dig, None, located, count, work, wb, s) == St.SUCCESS
    s.synchronize()
    assert int(w_status.item()) == 0 and int(r_status.item()) == 0
    st.assert_image(image_of(lay, final), f"after the repair, placement {placement}")
    stale = stale_parity_slots(ns(S, k, m), bm, written)
    assert len(stale) > 0 and int(count.item()) == len(stale)
    assert np.flatnonzero(located.cpu().numpy() == 0).tolist() == stale


# -- 8. capture ------------------------------------------------------------------------------------------------
def test_graph_applies_the_items_bitmap_and_bytes_of_each_replay(gpu):
    """Captured once and replayed three times.  Every input is on the device
    before the capture; between the replays the store, the items, the bitmap, the
    new bytes and the slots are rewritten by device-to-device copies only.  The
    capture is linear: a memset, the check kernel, the write kernel."""
    torch = _torch()
    S, k, m, bs = 5, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    off, ln = 1008, 2064
    rng = np.random.default_rng(41)
    ones = np.ones((S, k + m), np.uint8)
    bm0, bm1 = ones.copy(), ones.copy()
    bm0[0, 2] = bm0[1, k + 1] = 0  # (0, 0) rebuild-write, (1, 1) data-only, the rest delta
    bm1[1, 2] = bm1[3, 0] = 0      # (1, 0) rebuild-write between two writes; (3, 0) lost, unwritten
    plans = [(bm0, [(0, 0), (0, 2), (1, 1), (2, 4), (3, 3), (4, 5)]),
             (bm1, [(0, 1), (1, 0), (1, 2), (1, 4), (2, 0), (4, 4)]),
             (ones, [(0, 0), (0, 2), (1, 1), (2, 4), (3, 3), (4, 5)])]
    n = 6
    rounds = []
    for bm, written in plans:
        fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
        held, final = model(blocks, k, m, bm, written, fresh, off, ln)
        seeded = seed_slots(gpu, blocks, k, m, bm, written)
        rounds.append(dict(
            bm=bm, start=[torch.from_numpy(a).to("cuda") for a in image_of(lay, blocks, bm)],
            want=image_of(lay, held, bm), items=d_u32(items_of(written)), d_bm=device_bitmap(bm),
            new=New(fresh), seeded=d_u64(seeded),
            slots=want_slots(gpu, seeded, final, k, m, bm, written)))
    st = Store(lay, image_of(lay, blocks, bm0))
    d_items, d_bm = rounds[0]["items"].clone(), rounds[0]["d_bm"].clone()
    new, d_dig = New(np.zeros((n, ln), np.uint8)), rounds[0]["seeded"].clone()
    status = poison()
    # what each replay left, kept on the device: nothing is allocated between the replays
    # (the constraint recorded at xec_verify), the comparisons come after the last one
    got = [[torch.empty_like(t) for t in st.t] for _ in rounds]
    got_new = [torch.empty_like(new.buf) for _ in rounds]
    got_dig = [torch.empty_like(d_dig) for _ in rounds]
    verdicts = torch.full((len(rounds),), 77, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.write_shards_device(*st.args, d_bm, d_items, n, off, ln, new.ptr, d_dig, status,
                                       cs) == gpu.Status.SUCCESS
        assert gpu.shards_arg_capacity_used() == 64
    for r, rd in enumerate(rounds):
        for t, a in zip(st.t, rd["start"]):
            t.copy_(a)
        d_items.copy_(rd["items"])
        d_bm.copy_(rd["d_bm"])
        new.buf.copy_(rd["new"].buf)
        d_dig.copy_(rd["seeded"])
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for dst, t in zip(got[r], st.t):
            dst.copy_(t)
        got_new[r].copy_(new.buf)
        got_dig[r].copy_(d_dig)
        verdicts[r:r + 1].copy_(status)
    torch.cuda.synchronize()
    del g
    assert verdicts.tolist() == [0, 0, 0]
    for r, rd in enumerate(rounds):
        for t, kept in zip(st.t, got[r]):
            t.copy_(kept)
        st.assert_image(rd["want"], f"replay {r}")
        assert torch.equal(got_new[r], rd["new"].buf), f"replay {r}: d_new written"
        assert np.array_equal(as_u64(got_dig[r]), rd["slots"]), f"replay {r}: slots"


# -- 9. kernel events ----------------------------------------------------------------------------------------------
def test_kernel_events_time_the_write_kernel_and_are_consumed(gpu):
    torch = _torch()
    S, k, m, bs = 5, 32, 4, 65536
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "C")
    bm = np.ones((S, k + m), np.uint8)
    bm[1, 4] = bm[2, k + 1] = 0
    written = [(c, i) for c in range(S) for i in (0, 4, 5, 9, k - 1)]
    n = len(written)
    fresh = np.random.default_rng(7).integers(0, 256, size=(n, bs), dtype=np.uint8)
    held, _ = model(blocks, k, m, bm, written, fresh, 0, bs)
    st = Store(lay, image_of(lay, blocks, bm))
    d_bm, status = device_bitmap(bm), poison()
    d_items, new = d_u32(items_of(written)), New(fresh)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)  # torch creates the HIP handle at the first record
    e1.record(s)
    torch.cuda.synchronize()

    def run(nn=n):
        return gpu.write_shards_device(*st.args, d_bm, d_items, nn, 0, bs, new.ptr, None, status, s)

    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert run() == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1)
    assert t > 0
    # reads and writes at least the n*bs new bytes: slower than HBM could, so it is the
    # write kernel's own interval
    assert 2 * n * bs / (t * 1e-3) / 1e9 < 8000.0
    assert int(status.item()) == 0
    st.assert_image(image_of(lay, held, bm), "timed write")
    # a call that launches nothing consumes the setting
    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert run(0) == gpu.Status.SUCCESS
    assert run() == gpu.Status.SUCCESS  # the same bytes again over what it wrote: not armed
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) == t
