"""xec_readv_shards_device on an MI355X: the device-resident vectored read over
one buffer per shard, a range per entry.

The expected bytes of every case are the PRISTINE blocks of test_gpu_read.Batch
(parity by numpy),

    want = concat over t of pristine[c_t, i_t][offset_t : offset_t + len_t]

never anything the library computed.  The store is one of the three placements
of tests/test_gpu_shards.py; every lost block holds GARBAGE before a call, so a
kernel that reads one delivers wrong bytes, and after every call each allocation
is compared as a whole with the image it held before -- blocks, gaps between
blocks and guards.  d_out and d_work sit between two guards each and d_out
starts as SENTINEL.
"""
from __future__ import annotations

import types

import numpy as np
import pytest

from test_gpu_read import BSS, GARBAGE, GUARD, KMS, SENTINEL
from test_gpu_readv import VOut, guarded, guards_of, make_iov, total_of, want_bytes
from test_gpu_shards import (PLACEMENTS, POLICIES, SHAPES, Layout, Store, describe, device_bitmap,
                             poison, pristine)
from test_gpu_shards_read import mixed_items, read_bitmap

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def mixed_iov(bm, k, m, bs, rng):
    """test_gpu_shards_read.mixed_items (present and lost, data and parity,
    repeats, any order), each with a range of its own as test_gpu_readv.mixed_iov
    draws them: below, at and just past one 1 KiB tile, ragged tails, starts off
    the tile boundaries, and the whole block."""
    items = mixed_items(bm, k, m, rng)
    n = len(items)
    lens = [x for x in (16, 1008, 1024, 1040, 2064, bs) if x <= bs]
    ln = rng.choice(lens, size=n)
    off = np.zeros(n, np.int64)
    for t in range(n):
        offs = [o for o in (0, 16, 1008, bs - ln[t]) if o + ln[t] <= bs]
        off[t] = offs[int(rng.integers(len(offs)))]
    # the item mixed_items repeats for certain, with two ranges of its own
    twice = np.flatnonzero(items == (((bm.shape[0] - 1) << 8) | (k - 1)))
    assert len(twice) >= 2
    ln[twice[0]], off[twice[0]], ln[twice[1]], off[twice[1]] = 16, bs - 16, lens[-1], 0
    iov = make_iov(items, off, ln)
    assert len(set(iov["len"].tolist())) > 1
    return iov


def d_iov_of(iov):
    return _torch().from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")


def shard_readv(xec, st: Store, d_bm, iov, out: VOut, out_bytes=None, status=None, stream=None):
    """(status code, *d_status) of one xec_readv_shards_device; d_work guarded."""
    torch = _torch()
    n = len(iov)
    if status is None:
        status = poison()
    wbytes = xec.readv_device_work_bytes(n)
    keep, d_work = guarded(wbytes)
    code = xec.readv_shards_device(*st.args, d_bm, d_iov_of(iov), n, out.ptr,
                                   out.total if out_bytes is None else out_bytes, d_work, wbytes,
                                   status, stream)
    torch.cuda.synchronize()
    assert guards_of(keep), "a guard byte of d_work was written"
    return code, int(status.item())


def check_served(blocks, iov, out: VOut, what):
    got, want = out.body(), want_bytes(types.SimpleNamespace(blocks=blocks), iov)
    if not np.array_equal(got, want):
        ends = np.cumsum(iov["len"].astype(np.int64))
        first = int(np.flatnonzero(got != want)[0])
        t = int(np.searchsorted(ends, first, side="right"))
        raise AssertionError(f"{what}: byte {first} differs from the pristine blocks, entry {t} = "
                             f"{iov[t]}")
    assert out.guards_intact(), f"{what}: a guard byte of d_out was written"


# -- 1. mixed entries, every shape and placement; batch parity of bytes in placement A ----
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_mixed_entries_are_the_pristine_slices_in_list_order(gpu, k, m, bs, placement):
    torch = _torch()
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    rng = np.random.default_rng(k * 13 + m + bs)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    iov = mixed_iov(bm, k, m, bs, rng)
    what = describe(k, m, bs, S, placement)
    total = total_of(iov)
    # 48 bytes past the total belong to d_out's buffer but not to the call's output
    out = VOut(total + 48)
    assert shard_readv(gpu, st, d_bm, iov, out) == (gpu.Status.SUCCESS, 0), what
    assert gpu.shards_arg_capacity_used() == (64 if k + m <= 64 else 256), what
    body = out.body()
    assert (body[total:] == SENTINEL).all(), f"{what}: bytes past the total were written"
    exact = VOut(total)
    assert shard_readv(gpu, st, d_bm, iov, exact) == (gpu.Status.SUCCESS, 0), what
    check_served(blocks, iov, exact, what)
    assert np.array_equal(body[:total], exact.body()) and out.guards_intact(), what
    st.assert_image(before, "readv, " + what)
    assert np.array_equal(d_bm.cpu().numpy(), bm.reshape(-1))
    if placement == "A":  # the batch call on the same bytes delivers the same bytes
        d_off, p_off = lay.batch_offsets
        base = st.t[0].data_ptr()
        second, status = VOut(total), poison()
        wbytes = gpu.readv_device_work_bytes(len(iov))
        _, d_work = guarded(wbytes)
        assert gpu.readv_device(base + d_off, base + p_off, S, bs, k, m, d_bm, d_iov_of(iov),
                                len(iov), second.ptr, total, d_work, wbytes,
                                status) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and torch.equal(second.buf, exact.buf), what


# -- 2. no bitmap: a pure gather -------------------------------------------------------
def test_a_null_bitmap_is_a_pure_gather(gpu):
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "C")
    rng = np.random.default_rng(3)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    iov = mixed_iov(bm, k, m, bs, rng)
    held = blocks.copy()
    held[bm == 0] = GARBAGE  # what the blocks hold, the garbage included
    out = VOut(total_of(iov))
    assert shard_readv(gpu, st, None, iov, out) == (gpu.Status.SUCCESS, 0)
    check_served(held, iov, out, "gather")
    st.assert_image(before, "gather")


# -- 3. verdicts ---------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_verdicts_and_their_maximum_write_nothing(gpu, placement):
    S, k, m, bs = 11, 6, 2, 4352
    St = gpu.Status
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    rng = np.random.default_rng(17)
    bm = read_bitmap(S, k, m, rng)
    bm[S - 2, 1] = 0  # class 1 of stripe S-2 now lost block 1 and its parity block
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    good = [(((S - 1) << 8) | (k - 1), 16, 1040), (((S - 2) << 8) | 3, 0, bs),
            (((S - 2) << 8) | 5, 1008, 2064), ((0 << 8) | 0, bs - 16, 16),
            (((S - 1) << 8) | (k + m - 1), 0, 1024), (((S - 1) << 8) | (k - 1), 0, 16)]
    far = [((S << 8) | 0, 0, 16), ((0xFFFFFF << 8) | 0xFF, 0, 16), ((0 << 8) | (k + m), 16, 32)]
    unserv = [(((S - 2) << 8) | 1, 0, 64), (((S - 2) << 8) | (k + m - 1), 16, 1024)]
    broken = [((0 << 8) | 1, 0, 0), ((0 << 8) | 1, 8, 16), ((0 << 8) | 1, 0, 24),
              ((0 << 8) | 1, bs - 16, 32)]
    cases = [(good, 0), (good + broken[:1], 1), (broken, 1), (good + far[:1], 3), (far, 3),
             (good + unserv[:1], 4), (unserv, 4), (broken + far, 3), (broken + far + unserv, 4),
             (far[:1] + good + unserv + broken[1:2], 4)]
    for entries, verdict in cases:
        iov = make_iov(*[np.array(x) for x in zip(*entries)])
        out = VOut(max(total_of(iov), 16))
        assert shard_readv(gpu, st, d_bm, iov, out) == (St.SUCCESS, verdict), entries
        if verdict == 0:
            check_served(blocks, iov, out, f"beside a doubly-lost class, {placement}")
        else:
            assert out.all_sentinel(), f"d_out written under verdict {verdict}"
        st.assert_image(before, f"verdict {verdict}, placement {placement}")
    # a total past out_bytes: verdict 1 and not a byte
    iov = make_iov(*[np.array(x) for x in zip(*good)])
    out = VOut(total_of(iov))
    assert shard_readv(gpu, st, d_bm, iov, out, out_bytes=total_of(iov) - 16) == (St.SUCCESS, 1)
    assert out.all_sentinel()
    st.assert_image(before, f"a short d_out, placement {placement}")


# -- 4. every launch shape --------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(4, 1), (16, 1), (6, 2)])
def test_every_launch_shape(gpu, k, m):
    S, bs = KMS[(k, m)], 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    rng = np.random.default_rng(k + m)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    iov = mixed_iov(bm, k, m, bs, rng)
    total = total_of(iov)
    try:
        for threads, unroll in SHAPES:
            for policy in POLICIES:
                for max_grid in (0, 2):
                    assert gpu.set_launch(unroll, max_grid, policy, threads) == gpu.Status.SUCCESS
                    what = (f"{k}+{m} threads={threads} unroll={unroll} policy={policy} "
                            f"max_grid={max_grid}")
                    out = VOut(total)
                    assert shard_readv(gpu, st, d_bm, iov, out) == (gpu.Status.SUCCESS, 0), what
                    check_served(blocks, iov, out, what)
        st.assert_image(before, f"{k}+{m} under every launch shape")
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(3) == gpu.Status.SUCCESS  # plays no part
        out = VOut(total)
        assert shard_readv(gpu, st, d_bm, iov, out) == (gpu.Status.SUCCESS, 0)
        check_served(blocks, iov, out, "under a rotation")
    finally:
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(0) == gpu.Status.SUCCESS


# -- 5. the check order, and where d_out may lie ------------------------------------------------
def test_every_check_in_order(gpu):
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 5, 4, 1, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    bm = read_bitmap(S, k, m, np.random.default_rng(3))
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    ptrs, ds, ps = st.ptrs, lay.ds, lay.ps
    d_bm, status = device_bitmap(bm), poison()
    ok = make_iov(np.array([((S - 1) << 8) | (k - 1), (0 << 8) | k, (1 << 8) | 3]),
                  np.array([0, 16, 1008]), np.array([256, 16, 496]))
    total = total_of(ok)
    d_ok = d_iov_of(ok)
    out = VOut(total)
    need = gpu.readv_device_work_bytes(3)
    keep, work = guarded(need + 8)
    bad_table = [ptrs[0]] * (k + m)  # breaks the overlap rule wherever the table is reached
    r0, o0 = lay.at(0, 0)
    base = st.t[r0].data_ptr()
    in_gap = base + o0 + bs  # the 64 bytes between blocks 0 and 1 of shard 0

    def dev(t=ptrs, a=ds, b=ps, SS=S, bb=bs, kk=k, mm=m, iov=d_ok, n=3, o=out.ptr, ob=total,
            w=work, wb=need, stt=status):
        code = gpu.readv_shards_device(t, a, b, SS, bb, kk, mm, d_bm, iov, n, o, ob, w, wb, stt)
        assert gpu.shards_arg_capacity_used() == 0
        return code

    # 2. bs, then k and m, before everything that follows
    assert dev(t=None, bb=100, kk=6, mm=4, stt=None) == St.INVALID_SIZE
    assert dev(t=bad_table, kk=6, mm=4, stt=None) == St.INVALID_COUNTS
    # 3. d_status first, then xec_readv_device's own checks, all ahead of the table
    assert dev(t=bad_table, stt=None, o=None) == St.INVALID_ALIGNMENT
    assert dev(t=None, stt=status.data_ptr() + 2, n=0) == St.INVALID_ALIGNMENT
    for t in (ptrs, bad_table, None):
        assert dev(t=t, kk=255, mm=5, o=None) == St.INVALID_SIZE
        assert dev(t=t, SS=(1 << 24) + 1, o=None) == St.INVALID_SIZE
        assert dev(t=t, bb=1 << 32, o=None) == St.INVALID_SIZE
        assert dev(t=t, o=None, iov=d_ok.data_ptr() + 2) == St.INVALID_SIZE
        assert dev(t=t, iov=None, o=out.ptr + 8) == St.INVALID_SIZE
        assert dev(t=t, w=None, o=out.ptr + 8) == St.INVALID_SIZE
        assert dev(t=t, wb=need - 1, o=out.ptr + 8) == St.INVALID_SIZE
        assert dev(t=t, o=out.ptr + 8) == St.INVALID_ALIGNMENT
        assert dev(t=t, iov=d_ok.data_ptr() + 2, o=in_gap) == St.INVALID_ALIGNMENT
        assert dev(t=t, w=work + 4, o=in_gap) == St.INVALID_ALIGNMENT
    # 4. steps 3 to 7 of xec_check_shards, ahead of d_out's place
    tables = [
        ((None, ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:2] + [None] + ptrs[3:], ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:2] + [ptrs[2] + 16] + ptrs[3:], ds, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, ds + 32, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, bs - 64, ps, k, m), St.INVALID_SIZE),
        ((ptrs, ds, 1 << 62, k, m), St.INVALID_SIZE),
        ((ptrs[:3] + [ptrs[0]] + ptrs[4:], ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:-1] + [ptrs[1] + 64], ds, ps, k, m), St.INVALID_SIZE),
    ]
    for (t, a, b, kk, mm), code in tables:
        assert gpu.check_shards(t, a, b, S, bs, kk, mm) == code
        assert dev(t=t, a=a, b=b, kk=kk, mm=mm, o=in_gap) == code
    # 5. d_out on the hull of a shard
    assert dev(o=in_gap, ob=16) == St.INVALID_SIZE         # a gap between two blocks of one shard
    assert dev(o=base + o0) == St.INVALID_SIZE             # a block
    assert dev(o=base + o0 - total + 16) == St.INVALID_SIZE    # ends 16 bytes inside the hull
    assert dev(o=base + o0 + lay.hull(0) - 16) == St.INVALID_SIZE  # starts in its last 16 bytes
    # 6. a 32-bit tile count that could overflow
    assert dev(n=(1 << 32) // 5 + 1, wb=1 << 40) == St.INVALID_SIZE
    torch.cuda.synchronize()
    # nothing was queued: no byte of d_out or d_work, not even *d_status = 0
    assert out.all_sentinel() and int(status.item()) == 77 and bool((keep == SENTINEL).all())
    st.assert_image(before, "after rejected calls")
    # nothing to do: only the verdict is queued, whatever the table
    assert dev(t=bad_table, n=0, iov=None, o=None, w=None, wb=0) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    status.fill_(77)
    assert dev(t=None, SS=0, o=None) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and out.all_sentinel()
    st.assert_image(before, "after empty reads")
    # d_out may touch a hull: the bytes that end exactly where shard 0 begins are written
    iov = make_iov(np.array([((S - 1) << 8) | (k - 1), (0 << 8) | k, (1 << 8) | 3, (0 << 8) | 0]),
                   np.array([bs - 16, 0, 16, 1008]), np.array([16, 16, 16, 16]))
    assert bm[S - 1, k - 1] == 0 and bm[0, 0] == 0
    need4 = gpu.readv_device_work_bytes(4)
    keep4, work4 = guarded(need4)
    code = gpu.readv_shards_device(*st.args, d_bm, d_iov_of(iov), 4, base + o0 - 64, 64, work4,
                                   need4, status)
    assert code == St.SUCCESS and gpu.shards_arg_capacity_used() == 64
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    after = [a.copy() for a in before]
    assert (after[r0][o0 - 64:o0] == SENTINEL).all()
    after[r0][o0 - 64:o0] = want_bytes(types.SimpleNamespace(blocks=blocks), iov)
    st.assert_image(after, "d_out touching a hull")
    assert guards_of(keep4)


# -- 6. capture ----------------------------------------------------------------------------------
def test_graph_serves_the_entries_of_each_replay(gpu):
    """Captured once and replayed three times.  Every input is on the device
    before the capture; between the replays entries (their lengths too) and bitmap
    are rewritten by device-to-device copies only.  Each replay serves what they
    hold then."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    rng = np.random.default_rng(41)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    sel = [mixed_iov(bm, k, m, bs, rng) for _ in range(2)]
    n = len(sel[0])
    cap = max(total_of(x) for x in sel)
    held = blocks.copy()
    held[bm == 0] = GARBAGE  # a third round under a bitmap of no losses
    d_sel = [d_iov_of(x) for x in sel + [sel[0]]]
    d_bms = [device_bitmap(bm), device_bitmap(bm),
             torch.ones(S * (k + m), dtype=torch.uint8, device="cuda")]
    ns = types.SimpleNamespace
    wants = [want_bytes(ns(blocks=blocks), sel[0]), want_bytes(ns(blocks=blocks), sel[1]),
             want_bytes(ns(blocks=held), sel[0])]
    assert len(wants[0]) != len(wants[1]) or not np.array_equal(wants[0], wants[1])
    d_wants = [torch.from_numpy(np.ascontiguousarray(w)).to("cuda") for w in wants]
    d_iov, d_bm = d_sel[0].clone(), d_bms[0].clone()
    status = poison()
    out = VOut(cap)
    wbytes = gpu.readv_device_work_bytes(n)
    keep, d_work = guarded(wbytes)
    # what each replay left, kept on the device: nothing is allocated between the replays
    # (the constraint recorded at xec_verify), the comparisons come after the last one
    got = [torch.empty_like(out.buf) for _ in range(3)]
    verdicts = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.readv_shards_device(*st.args, d_bm, d_iov, n, out.ptr, cap, d_work, wbytes,
                                       status, cs) == gpu.Status.SUCCESS
        assert gpu.shards_arg_capacity_used() == 64
    for r in range(3):
        d_iov.copy_(d_sel[r])
        d_bm.copy_(d_bms[r])
        out.buf.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got[r].copy_(out.buf)
        verdicts[r:r + 1].copy_(status)
    torch.cuda.synchronize()
    del g
    assert verdicts.tolist() == [0, 0, 0]
    for r in range(3):
        t = len(wants[r])
        assert torch.equal(got[r][GUARD:GUARD + t], d_wants[r]), f"replay {r}"
        assert bool((got[r][GUARD + t:] == SENTINEL).all()), f"replay {r}: past the total"
        assert bool((got[r][:GUARD] == SENTINEL).all()), f"replay {r}: the guard"
    assert guards_of(keep)
    st.assert_image(before, "after the replays")


# -- 7. kernel events ------------------------------------------------------------------------------
def test_kernel_events_time_the_read_kernel_and_are_consumed(gpu):
    torch = _torch()
    S, k, m, bs = 5, 32, 4, 65536
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "C")
    rng = np.random.default_rng(7)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm, status = device_bitmap(bm), poison()
    items = mixed_items(bm, k, m, rng, extra=40)
    iov = make_iov(items, 0, bs)
    d_iov = d_iov_of(iov)
    n, total = len(iov), total_of(iov)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)  # torch creates the HIP handle at the first record
    e1.record(s)
    torch.cuda.synchronize()
    out = VOut(total)
    wbytes = gpu.readv_device_work_bytes(n)
    _, d_work = guarded(wbytes)

    def run(nn=n):
        return gpu.readv_shards_device(*st.args, d_bm, d_iov, nn, out.ptr, total, d_work, wbytes,
                                       status, s)

    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert run() == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1)
    assert t > 0
    # delivers `total` bytes: slower than HBM could, so it is the read kernel's own
    # interval and not the check's or the scan's
    assert total / (t * 1e-3) / 1e9 < 8000.0
    assert run() == gpu.Status.SUCCESS  # not armed any more
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) == t
    check_served(blocks, iov, out, "timed readv")
    # a call that launches nothing consumes the setting
    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert run(0) == gpu.Status.SUCCESS
    assert run() == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) == t
    st.assert_image(before, "timed readv")
