"""xec_read_shards_device on an MI355X: the device-resident degraded read over
one buffer per shard.

The expected bytes of every case are the PRISTINE blocks of test_gpu_read.Batch
(parity by numpy),

    want[t] = pristine[c, i][offset : offset + len]

never anything the library computed.  The store is one of the three placements
of tests/test_gpu_shards.py; every lost block holds GARBAGE before a call, so a
kernel that reads one delivers wrong bytes, and after every call each allocation
is compared as a whole with the image it held before -- blocks, gaps between
blocks and guards -- so a kernel that writes the store shows too.  d_out sits
between two guards and starts as SENTINEL.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_read import BSS, GARBAGE, GUARD, KMS, SENTINEL, Out, ranges_for
from test_gpu_shards import (PLACEMENTS, POLICIES, SHAPES, Layout, Store, describe, device_bitmap,
                             loss_bitmap, poison, pristine)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def read_bitmap(S, k, m, rng):
    """One loss per class at most.  Certain: (0, 0) a lost data block, (S-1, k-1)
    a lost data block of the last stripe, (S-2, k+m-1) a lost parity block; every
    other block of stripes S-1 and S-2 is present."""
    assert S >= 3
    bm = loss_bitmap("mixed", S, k, m, rng)
    bm[S - 2:] = 1
    bm[S - 1, k - 1] = 0
    bm[S - 2, k + m - 1] = 0
    assert bm[0, 0] == 0
    return np.ascontiguousarray(bm)


def mixed_items(bm, k, m, rng, extra=24):
    """Present and lost, data and parity, shuffled, with repeats; stripe S-1 and
    shards k-1, k and k+m-1 always among them (a swapped pair of strides then
    reads another block in every placement with two strides)."""
    S = bm.shape[0]
    must = [(S - 1, k - 1), (S - 1, k), (S - 1, k + m - 1), (S - 2, k + m - 1), (S - 2, k - 1),
            (0, 0), (S - 1, 0), (1, k)]
    lost, pres = np.argwhere(bm == 0), np.argwhere(bm != 0)
    more = np.concatenate([lost[rng.integers(len(lost), size=extra // 2)],
                           pres[rng.integers(len(pres), size=extra // 2)]])
    ci = np.concatenate([np.array(must), more, np.array(must[:3])])  # and repeats for certain
    ci = ci[rng.permutation(len(ci))]
    items = ((ci[:, 0] << 8) | ci[:, 1]).astype(np.uint32)
    is_lost = bm[ci[:, 0], ci[:, 1]] == 0
    par = ci[:, 1] >= k
    assert (is_lost & par).any() and (is_lost & ~par).any()
    assert (~is_lost & par).any() and (~is_lost & ~par).any()
    assert len(set(items.tolist())) < len(items) and np.any(np.diff(items.astype(np.int64)) < 0)
    return items


def d_u32(items):
    return _torch().from_numpy(np.ascontiguousarray(items, dtype=np.uint32).view(np.int32)).to("cuda")


def shard_read(xec, st: Store, d_bm, items, offset, length, out_ptr, status=None, stream=None):
    """(status code, *d_status) of one xec_read_shards_device."""
    torch = _torch()
    if status is None:
        status = poison()
    code = xec.read_shards_device(*st.args, d_bm, d_u32(items), len(items), offset, length,
                                  out_ptr, status, stream)
    torch.cuda.synchronize()
    return code, int(status.item())


def want_bytes(blocks, items, offset, length):
    it = np.asarray(items, dtype=np.int64)
    return blocks[it >> 8, it & 0xFF, offset:offset + length]


def check_served(blocks, items, offset, length, out: Out, what):
    got, want = out.body(), want_bytes(blocks, items, offset, length)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(items)} items differ from the pristine "
                           f"blocks, first t={bad[0]} item={int(items[bad[0]]):#x}")
    assert out.guards_intact(), f"{what}: a guard byte of d_out was written"


# -- 1. mixed items, every shape, range and placement -----------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_ranges_of_mixed_items_are_the_pristine_bytes(gpu, k, m, bs, placement):
    torch = _torch()
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    rng = np.random.default_rng(k * 13 + m + bs)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    items = mixed_items(bm, k, m, rng)
    for offset, length in ranges_for(bs):
        what = f"{describe(k, m, bs, S, placement)} [{offset}, +{length})"
        out = Out(len(items), length)
        assert shard_read(gpu, st, d_bm, items, offset, length, out.ptr) == (gpu.Status.SUCCESS,
                                                                             0), what
        assert gpu.shards_arg_capacity_used() == (64 if k + m <= 64 else 256), what
        check_served(blocks, items, offset, length, out, what)
        st.assert_image(before, "read, " + what)
        if placement == "A":  # the batch call on the same bytes delivers the same bytes
            d_off, p_off = lay.batch_offsets
            base = st.t[0].data_ptr()
            second, status = Out(len(items), length), poison()
            assert gpu.read_device(base + d_off, base + p_off, S, bs, k, m, d_bm, d_u32(items),
                                   len(items), offset, length, second.ptr,
                                   status) == gpu.Status.SUCCESS
            torch.cuda.synchronize()
            assert int(status.item()) == 0 and torch.equal(second.buf, out.buf), what
    assert np.array_equal(d_bm.cpu().numpy(), bm.reshape(-1))


# -- 2. no bitmap: a pure gather ----------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_a_null_bitmap_is_a_pure_gather(gpu, placement):
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    rng = np.random.default_rng(3)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    items = mixed_items(bm, k, m, rng)
    held = blocks.copy()
    held[bm == 0] = GARBAGE  # what the blocks hold, the garbage included
    for offset, length in [(1008, 2064), (0, bs)]:
        want = want_bytes(held, items, offset, length)
        assert (want == GARBAGE).all(axis=1).any()
        out = Out(len(items), length)
        assert shard_read(gpu, st, None, items, offset, length, out.ptr) == (gpu.Status.SUCCESS, 0)
        assert np.array_equal(out.body(), want) and out.guards_intact(), placement
        st.assert_image(before, f"gather, placement {placement}")


# -- 3. verdicts -----------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_reads_are_served_where_repair_refuses(gpu, placement):
    """Stripe S-2 gets a doubly-lost class: xec_repair_shards_device refuses the
    store, the read serves every item that is not a LOST block of that class --
    its present blocks included."""
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
    status = poison()
    assert gpu.repair_shards_device(*st.args, d_bm, status) == St.SUCCESS
    _torch().cuda.synchronize()
    assert int(status.item()) == 4
    st.assert_image(before, "after the refused repair")
    good = [((S - 1) << 8) | (k - 1), ((S - 2) << 8) | 3, ((S - 2) << 8) | 5,  # present, broken class
            ((S - 2) << 8) | 0, (0 << 8) | 0, ((S - 1) << 8) | (k + m - 1), ((S - 1) << 8) | (k - 1)]
    far = [(S << 8) | 0, (0xFFFFFF << 8) | 0xFF, (0 << 8) | (k + m)]  # never dereferenced
    unserv = [((S - 2) << 8) | 1, ((S - 2) << 8) | (k + m - 1)]
    offset, length = 1008, 2064
    for items, verdict in [(good, 0), (good + unserv[:1], 4), (unserv, 4), (good + far[:1], 3),
                           (far, 3), (far[:1] + good + unserv + far[1:], 4)]:
        items = np.array(items, np.uint32)
        out = Out(len(items), length)
        assert shard_read(gpu, st, d_bm, items, offset, length, out.ptr) == (St.SUCCESS, verdict)
        if verdict == 0:
            check_served(blocks, items, offset, length, out, f"beside a doubly-lost class, {placement}")
        else:
            assert out.all_sentinel(), f"d_out written under verdict {verdict}"
        st.assert_image(before, f"verdict {verdict}, placement {placement}")
    # without a bitmap only the range of an item can be wrong
    out = Out(len(far), length)
    assert shard_read(gpu, st, None, np.array(far, np.uint32), offset, length,
                      out.ptr) == (St.SUCCESS, 3)
    assert out.all_sentinel()


# -- 4. every launch shape ------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(4, 1), (16, 1), (6, 2)])
def test_every_launch_shape(gpu, k, m):
    """One shape per compiled member-count class, in the placement with two
    different strides, under every (threads, unroll), both cache policies, the
    default grid and a grid of two workgroups striding over the tiles."""
    S, bs = KMS[(k, m)], 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    rng = np.random.default_rng(k + m)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    d_bm = device_bitmap(bm)
    items = mixed_items(bm, k, m, rng)
    try:
        for threads, unroll in SHAPES:
            for policy in POLICIES:
                for max_grid in (0, 2):
                    assert gpu.set_launch(unroll, max_grid, policy, threads) == gpu.Status.SUCCESS
                    for offset, length in [(1008, 2064), (0, bs), (bs - 16, 16)]:
                        what = (f"{k}+{m} threads={threads} unroll={unroll} policy={policy} "
                                f"max_grid={max_grid} [{offset}, +{length})")
                        out = Out(len(items), length)
                        assert shard_read(gpu, st, d_bm, items, offset, length,
                                          out.ptr) == (gpu.Status.SUCCESS, 0), what
                        check_served(blocks, items, offset, length, out, what)
        st.assert_image(before, f"{k}+{m} under every launch shape")
        # rotation plays no part
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(3) == gpu.Status.SUCCESS
        out = Out(len(items), bs)
        assert shard_read(gpu, st, d_bm, items, 0, bs, out.ptr) == (gpu.Status.SUCCESS, 0)
        check_served(blocks, items, 0, bs, out, "under a rotation")
    finally:
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(0) == gpu.Status.SUCCESS


# -- 5. the check order, and where d_out may lie ----------------------------------------
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
    ok = np.array([((S - 1) << 8) | (k - 1), (0 << 8) | k, (1 << 8) | 3], np.uint32)
    d_ok = d_u32(ok)
    out = Out(3, 256)
    bad_table = [ptrs[0]] * (k + m)  # breaks the overlap rule wherever the table is reached
    r0, o0 = lay.at(0, 0)
    in_gap = st.t[r0].data_ptr() + o0 + bs  # the 64 bytes between blocks 0 and 1 of shard 0

    def dev(t=ptrs, a=ds, b=ps, SS=S, bb=bs, kk=k, mm=m, items=d_ok, n=3, off=0, ln=256,
            o=out.ptr, stt=status):
        code = gpu.read_shards_device(t, a, b, SS, bb, kk, mm, d_bm, items, n, off, ln, o, stt)
        assert gpu.shards_arg_capacity_used() == 0
        return code

    # 2. bs, then k and m, before everything that follows
    assert dev(t=None, bb=100, kk=6, mm=4, stt=None) == St.INVALID_SIZE
    assert dev(t=bad_table, kk=6, mm=4, stt=None, ln=0) == St.INVALID_COUNTS
    # 3. d_status first
    assert dev(t=bad_table, stt=None, ln=0, o=None) == St.INVALID_ALIGNMENT
    assert dev(t=None, stt=status.data_ptr() + 2, n=0) == St.INVALID_ALIGNMENT
    # ... then the packing, the range, the pointers and their alignment, ahead of the table
    for t in (ptrs, bad_table, None):
        assert dev(t=t, kk=255, mm=5, ln=0) == St.INVALID_SIZE
        assert dev(t=t, SS=(1 << 24) + 1, ln=0) == St.INVALID_SIZE
        for off, ln in [(0, 0), (8, 256), (0, 24), (bs - 16, 32), (bs, 16), (bs + 16, 16)]:
            assert dev(t=t, off=off, ln=ln, o=None) == St.INVALID_SIZE, (off, ln)
        assert dev(t=t, o=None, items=d_ok.data_ptr() + 2) == St.INVALID_SIZE
        assert dev(t=t, items=None, o=out.ptr + 8) == St.INVALID_SIZE
        assert dev(t=t, o=out.ptr + 8, items=d_ok.data_ptr() + 2) == St.INVALID_ALIGNMENT
        assert dev(t=t, items=d_ok.data_ptr() + 2, o=in_gap) == St.INVALID_ALIGNMENT
    # 5. steps 3 to 7 of xec_check_shards, ahead of d_out's place
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
    # 6. d_out on the hull of a shard
    base = st.t[r0].data_ptr()
    assert dev(o=in_gap, ln=16) == St.INVALID_SIZE          # a gap between two blocks of one shard
    assert dev(o=base + o0) == St.INVALID_SIZE              # a block
    assert dev(o=base + o0 - 2 * 256 - 16) == St.INVALID_SIZE  # ends 16 bytes inside the hull
    assert dev(o=base + o0 + lay.hull(0) - 16) == St.INVALID_SIZE  # starts in its last 16 bytes
    assert dev(o=out.ptr, n=(1 << 64) // 256) == St.INVALID_SIZE    # n_items * len wraps
    torch.cuda.synchronize()
    # nothing was queued: no byte of d_out, not even *d_status = 0
    assert out.all_sentinel() and int(status.item()) == 77
    st.assert_image(before, "after rejected calls")
    # nothing to do: only the verdict is queued, whatever the table and the range
    assert dev(t=bad_table, n=0, items=None, o=None, ln=0) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    status.fill_(77)
    assert dev(t=None, SS=0, off=8, o=None) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and out.all_sentinel()
    st.assert_image(before, "after empty reads")
    # d_out may touch a hull: 64 bytes that end exactly where shard 0 begins (a guard or
    # the gap behind the neighbour below, whose hull they touch as well) are written
    items = np.array([((S - 1) << 8) | (k - 1), (0 << 8) | k, (1 << 8) | 3, (0 << 8) | 0], np.uint32)
    assert bm[S - 1, k - 1] == 0 and bm[0, 0] == 0
    code = gpu.read_shards_device(*st.args, d_bm, d_u32(items), 4, bs - 16, 16, base + o0 - 64,
                                  status)
    assert code == St.SUCCESS and gpu.shards_arg_capacity_used() == 64
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    after = [a.copy() for a in before]
    assert (after[r0][o0 - 64:o0] == SENTINEL).all()
    after[r0][o0 - 64:o0] = want_bytes(blocks, items, bs - 16, 16).reshape(-1)
    st.assert_image(after, "d_out touching a hull")


# -- 6. capture -----------------------------------------------------------------------------
def test_graph_of_read_shards_device_serves_the_selection_of_each_replay(gpu):
    """Captured once and replayed three times.  Every input is on the device
    before the capture; between the replays items and bitmap are rewritten by
    device-to-device copies only (the constraint recorded at xec_verify).  Each
    replay serves what they hold then."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    rng = np.random.default_rng(41)
    bm = read_bitmap(S, k, m, rng)
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    offset, length = 1008, 2064
    sel = [mixed_items(bm, k, m, rng) for _ in range(2)]
    n = len(sel[0])
    held = blocks.copy()
    held[bm == 0] = GARBAGE  # a third selection under a bitmap of no losses
    d_sel = [d_u32(x) for x in sel + [sel[0]]]
    d_bms = [device_bitmap(bm), device_bitmap(bm), torch.ones(S * (k + m), dtype=torch.uint8,
                                                              device="cuda")]
    wants = [want_bytes(blocks, sel[0], offset, length), want_bytes(blocks, sel[1], offset, length),
             want_bytes(held, sel[0], offset, length)]
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[0], wants[2])
    d_wants = [torch.from_numpy(np.ascontiguousarray(w)).to("cuda") for w in wants]
    d_items, d_bm = d_sel[0].clone(), d_bms[0].clone()
    status = poison()
    out = Out(n, length)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.read_shards_device(*st.args, d_bm, d_items, n, offset, length, out.ptr, status,
                                      cs) == gpu.Status.SUCCESS
        assert gpu.shards_arg_capacity_used() == 64
    for r in range(3):
        d_items.copy_(d_sel[r])
        d_bm.copy_(d_bms[r])
        out.buf.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == 0, r
        assert torch.equal(out.buf[GUARD:-GUARD].view(n, length), d_wants[r]), f"replay {r}"
        assert out.guards_intact()
    del g
    st.assert_image(before, "after the replays")


# -- 7. kernel events ------------------------------------------------------------------------
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
    d_items = d_u32(items)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)  # torch creates the HIP handle at the first record
    e1.record(s)
    torch.cuda.synchronize()
    out = Out(len(items), bs)

    def run():
        return gpu.read_shards_device(*st.args, d_bm, d_items, len(items), 0, bs, out.ptr, status, s)

    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert run() == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1)
    assert t > 0
    # delivers len(items)*bs bytes: slower than HBM could, so it is the kernel's own interval
    assert len(items) * bs / (t * 1e-3) / 1e9 < 8000.0
    assert run() == gpu.Status.SUCCESS  # not armed any more
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) == t
    check_served(blocks, items, 0, bs, out, "timed read")
    st.assert_image(before, "timed read")
