"""xec_digest_shards and xec_locate_shards on an MI355X: block digests and the
locate over one buffer per shard, and the chain scrub -> locate -> repair on
that memory.

Every expected digest is the numpy restatement of the formula
(tests/test_digest_abi.py np_digest, spot-checked against xec_digest_host) over
the PRISTINE blocks of test_gpu_read.Batch; every expected bitmap is built here
from the blocks the test damaged.  The store is one of the three placements of
tests/test_gpu_shards.py (A aliased into a batch, B one arena with two strides
and 64-byte gaps, C interleaved and separate allocations), and after every call
each allocation is compared as a whole with the image it held before: blocks,
gaps and guards at once.  Slots, bitmaps and counts start from a fill, so one
that was never written shows.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_digest_abi import np_digest
from test_gpu_read import BSS, KMS, SENTINEL
from test_gpu_shards import (PLACEMENTS, POISON, Layout, Store, describe, device_bitmap, poison,
                             pristine, scrub)

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")
BIG = 2 * (64 << 10) + 256  # two digest segments and a ragged quarter tile
OVERRIDES = [dict(), dict(block_threads=256), dict(cache_policy=2), dict(max_grid=2)]
_REF: dict = {}


def _torch():
    import torch
    return torch


def ref_digests(S, k, m, bs) -> np.ndarray:
    """(S, k+m) uint64 of the pristine blocks, computed once per shape."""
    key = (S, k, m, bs)
    if key not in _REF:
        _REF[key] = np_digest(pristine(S, k, m, bs))
        _REF[key].setflags(write=False)
    return _REF[key]


def slots(n):
    """n u64 of device memory as bytes, prefilled."""
    return _torch().full((8 * n,), FILL, dtype=_torch().uint8, device="cuda")


def as_u64(t) -> np.ndarray:
    return t.cpu().numpy().view("<u8")


def stored(ref):
    return _torch().from_numpy(np.ascontiguousarray(ref).reshape(-1).view(np.uint8).copy()).to("cuda")


def damaged(lay: Layout, clean, flips):
    """A copy of the image `clean` with bit `bit` of byte `byte` of block x of
    stripe c flipped, for every (c, x, byte, bit)."""
    bad = [a.copy() for a in clean]
    for c, x, byte, bit in flips:
        r, o = lay.at(x, c)
        bad[r][o + byte] ^= bit
    return bad


def expect_bitmap(lay: Layout, bad):
    bm = np.ones((lay.S, lay.k + lay.m), np.uint8)
    for c, x in bad:
        bm[c, x] = 0
    return bm


def run_locate(xec, st: Store, dig, flags=None, stream=None):
    """(bitmap (S, k+m), count) of one xec_locate_shards over the store."""
    torch = _torch()
    lay = st.lay
    n = lay.S * (lay.k + lay.m)
    bitmap = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    count = poison()
    wb = xec.locate_work_bytes(lay.S, lay.k, lay.m)
    work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
    assert xec.locate_shards(*st.args, dig, flags, bitmap, count, work, wb,
                             stream) == xec.Status.SUCCESS
    assert xec.shards_arg_capacity_used() == (64 if lay.k + lay.m <= 64 else 256)
    torch.cuda.synchronize()
    return bitmap.cpu().numpy().reshape(lay.S, lay.k + lay.m), int(count.item())


def batch_locate(xec, st: Store, dig, flags=None):
    """xec_locate on the batch that placement A's table is aliased into."""
    torch = _torch()
    lay = st.lay
    d_off, p_off = lay.batch_offsets
    base = st.t[0].data_ptr()
    n = lay.S * (lay.k + lay.m)
    bitmap = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    count = poison()
    wb = xec.locate_work_bytes(lay.S, lay.k, lay.m)
    work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
    assert xec.locate(base + d_off, base + p_off, lay.S, lay.bs, lay.k, lay.m, dig, flags, bitmap,
                      count, work, wb) == xec.Status.SUCCESS
    torch.cuda.synchronize()
    return bitmap.cpu().numpy().reshape(lay.S, lay.k + lay.m), int(count.item())


# -- 1. the digest of every block ---------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_digest_of_every_block_is_the_host_digest(gpu, k, m, bs, placement):
    torch = _torch()
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    ref = ref_digests(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    clean = lay.image(blocks)
    st = Store(lay, clean)
    what = describe(k, m, bs, S, placement)
    dig = slots(S * (k + m))
    assert gpu.digest_shards(*st.args, dig) == gpu.Status.SUCCESS, what
    assert gpu.shards_arg_capacity_used() == (64 if k + m <= 64 else 256), what
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(dig), ref.reshape(-1)), what
    for c, x in ((0, 0), (S - 1, k + m - 1)):  # the host digest is the same sum
        assert gpu.digest_host(blocks[c, x]) == int(ref[c, x]), what
    st.assert_image(clean, "digest, " + what)
    if placement == "A":  # the batch call on the same bytes leaves the same slots
        d_off, p_off = lay.batch_offsets
        second = slots(S * (k + m))
        base = st.t[0].data_ptr()
        assert gpu.digest(base + d_off, base + p_off, S, bs, k, m, second) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(second, dig), what


# -- 2. segment boundaries ------------------------------------------------------
@pytest.mark.parametrize("shape", OVERRIDES,
                         ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()) or "default")
def test_three_segments_meet_in_every_slot(gpu, shape):
    """bs = two 64 KiB segments and 256 bytes: three workgroups add into one
    slot, under the default launch, 256 threads, the default cache policy and a
    grid of two workgroups striding over the tiles; two different strides."""
    torch = _torch()
    S, k, m, bs = 3, 4, 1, BIG
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    clean = lay.image(blocks)
    st = Store(lay, clean)
    dig = slots(S * (k + m))
    try:
        assert gpu.set_launch(**shape) == gpu.Status.SUCCESS
        assert gpu.digest_shards(*st.args, dig) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
    finally:
        gpu.set_launch()
    assert np.array_equal(as_u64(dig), ref_digests(S, k, m, bs).reshape(-1)), shape
    st.assert_image(clean, f"digest under {shape}")


# -- 3. selection -----------------------------------------------------------------
@pytest.mark.parametrize("k,m,bs", [(6, 2, 4352), (66, 2, 256), (4, 1, BIG)])
def test_selection_reads_and_writes_the_selected_only(gpu, k, m, bs):
    torch = _torch()
    S = 3 if bs == BIG else KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    ref = ref_digests(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    clean = lay.image(blocks)
    st = Store(lay, clean)
    rng = np.random.default_rng(k * 31 + m + bs)
    sel = (rng.random((S, k + m)) < 0.4).astype(np.uint8) * rng.choice(
        np.array([1, 2, 255], np.uint8), size=(S, k + m))
    sel[S - 1, k + m - 1] = 7  # the last block of the last shard
    sel[0, 0], sel[0, 1], sel[0, k] = 1, 0, 0
    assert sel[:, :k].any() and sel[:, k:].any() and (sel[:, :k] == 0).any()
    d_sel = device_bitmap(sel)
    dig = slots(S * (k + m))
    assert gpu.digest_shards(*st.args, dig, d_sel) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    want = np.where(sel != 0, ref, np.uint64(FILL64)).reshape(-1)
    assert np.array_equal(as_u64(dig), want)
    assert np.array_equal(d_sel.cpu().numpy(), sel.reshape(-1))
    st.assert_image(clean, "selected digest")
    # a byte of an unselected block, and one of the gap behind block 0 of shard 0:
    # the selected slots do not move, so neither was read
    bad = damaged(lay, clean, [(0, 1, bs // 2, 0x40), (0, k, 3, 0x01)])
    r, o = lay.at(0, 0)
    assert bad[r][o + bs + 9] == SENTINEL
    bad[r][o + bs + 9] ^= 0xFF
    st.load(bad)
    again = slots(S * (k + m))
    assert gpu.digest_shards(*st.args, again, d_sel) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(again), want)
    st.assert_image(bad, "selected digest of a damaged store")


# -- 4. full locate ---------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("k,m,bs", [(4, 1, 4352), (6, 2, 256), (66, 2, 4352), (16, 1, 65536)])
def test_full_locate_names_the_damaged_blocks(gpu, k, m, bs, placement):
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    clean = lay.image(blocks)
    st = Store(lay, clean)
    dig = stored(ref_digests(S, k, m, bs))
    what = describe(k, m, bs, S, placement)
    bm, count = run_locate(gpu, st, dig)
    assert count == 0 and np.array_equal(bm, expect_bitmap(lay, [])), what
    # one bit in the last 16 bytes of a data block, one in a parity block of another stripe
    flips = [(0, k - 1, bs - 5, 0x10), (S - 1, k + m - 1, bs // 2, 0x01)]
    bad = damaged(lay, clean, flips)
    st.load(bad)
    bm, count = run_locate(gpu, st, dig)
    assert count == 2, what
    assert np.array_equal(bm, expect_bitmap(lay, [(0, k - 1), (S - 1, k + m - 1)])), what
    st.assert_image(bad, "locate, " + what)
    if placement == "A":
        bm_b, count_b = batch_locate(gpu, st, dig)
        assert count_b == count and np.array_equal(bm_b, bm), what
    # the same bit at the same offset of two blocks of one class cancels in the XOR
    pair = [(1, m - 1, 40, 0x08), (1, k + m - 1, 40, 0x08)]
    bad = damaged(lay, clean, pair)
    st.load(bad)
    assert scrub(gpu, st)[:2] == ([], 0), f"the scrub saw a cancelling pair, {what}"
    bm, count = run_locate(gpu, st, dig)
    assert count == 2, what
    assert np.array_equal(bm, expect_bitmap(lay, [(1, m - 1), (1, k + m - 1)])), what
    st.assert_image(bad, "locate of a cancelling pair, " + what)


# -- 5. locate with flags -----------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("k,m,bs", [(6, 2, 4352), (32, 4, 256), (4, 1, BIG)])
def test_locate_with_flags_checks_the_flagged_classes_only(gpu, k, m, bs, placement):
    S = 3 if bs == BIG else KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    ref = ref_digests(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    clean = lay.image(blocks)
    what = describe(k, m, bs, S, placement)
    # damage in class m - 1 of stripe S - 1 (a data block) and class 0 of stripe 0 (parity)
    hit = [(S - 1, k - 1), (0, k)]
    bad = damaged(lay, clean, [(S - 1, k - 1, bs - 1, 0x80), (0, k, 0, 0x01)])
    st = Store(lay, bad)
    flagged, n_flagged, flags = scrub(gpu, st)
    assert flagged == sorted([(S - 1) * m + m - 1, 0]) and n_flagged == 2, what
    d_flags = _torch().from_numpy(flags).to("cuda")
    # spoiled stored digests: one in an unflagged class (must read 1), one in a
    # flagged class of an undamaged block (must read 0: it was checked)
    spoiled = ref.copy()
    unflagged = (1, 0) if S > 1 else None
    assert unflagged is not None and flags[1 * m + 0] == 0
    spoiled[unflagged] ^= np.uint64(1)
    also = (0, 0)  # class 0 of stripe 0 is flagged
    spoiled[also] ^= np.uint64(1 << 63)
    bm, count = run_locate(gpu, st, stored(spoiled), d_flags)
    want = expect_bitmap(lay, hit + [also])
    assert want[unflagged] == 1
    assert count == 3 and np.array_equal(bm, want), what
    st.assert_image(bad, "locate with flags, " + what)
    assert np.array_equal(d_flags.cpu().numpy(), flags), what
    if placement == "A":
        bm_b, count_b = batch_locate(gpu, st, stored(spoiled), d_flags)
        assert count_b == count and np.array_equal(bm_b, bm), what
    # the gate reads nothing of an unflagged class: damage there, and in a gap, changes nothing
    if placement == "B":
        worse = damaged(lay, bad, [(1, 0, 17, 0x02)])  # would differ from its (unspoiled) digest
        r, o = lay.at(0, 0)
        worse[r][o + bs + 5] ^= 0xFF
        st.load(worse)
        bm, count = run_locate(gpu, st, stored(ref), d_flags)
        assert count == 2 and np.array_equal(bm, expect_bitmap(lay, hit)), what
        st.assert_image(worse, "gated locate, " + what)


# -- 6. the heal chain ----------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_verify_locate_repair_on_one_stream(gpu, placement):
    """xec_verify_shards -> xec_locate_shards(flags) -> xec_repair_shards_device
    queued back to back on a side stream, one synchronisation at the end."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    clean = lay.image(blocks)
    dig = stored(ref_digests(S, k, m, bs))
    one_each = [(0, k - 1, bs - 5, 0x10), (S - 1, k + m - 1, bs // 2, 0x01), (4, 2, 0, 0xFF)]
    two_in_a_class = one_each + [(4, 4, 100, 0x01)]  # blocks 2 and 4 of stripe 4: class 0
    st = Store(lay, clean)
    n = S * (k + m)
    wb = gpu.locate_work_bytes(S, k, m)
    for flips, want_status in ((one_each, 0), (two_in_a_class, 4)):
        bad = damaged(lay, clean, flips)
        st.load(bad)
        flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
        bitmap = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
        n_flags, n_bad, status = poison(), poison(), poison()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            assert gpu.verify_shards(*st.args, flags, n_flags, s) == gpu.Status.SUCCESS
            assert gpu.locate_shards(*st.args, dig, flags, bitmap, n_bad, work, wb,
                                     s) == gpu.Status.SUCCESS
            assert gpu.repair_shards_device(*st.args, bitmap, status, s) == gpu.Status.SUCCESS
        s.synchronize()
        what = f"{len(flips)} damaged blocks, placement {placement}"
        assert int(n_flags.item()) == 3 and int(n_bad.item()) == len(flips), what
        want_bm = expect_bitmap(lay, [(c, x) for c, x, _, _ in flips])
        assert np.array_equal(bitmap.cpu().numpy().reshape(S, k + m), want_bm), what
        assert int(status.item()) == want_status, what
        if want_status == 0:
            st.assert_image(clean, "healed, " + what)
            assert scrub(gpu, st)[:2] == ([], 0), what
        else:  # repair is all-or-nothing: the damage stays
            st.assert_image(bad, "refused, " + what)


# -- 7. rejected calls ------------------------------------------------------------------
def test_rejected_calls_queue_nothing(gpu):
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 5, 4, 1, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    before = lay.image(blocks)
    st = Store(lay, before)
    ptrs, ds, ps = st.ptrs, lay.ds, lay.ps
    wide_n = S * 257
    dig, bitmap = slots(wide_n), torch.full((wide_n,), 0xFF, dtype=torch.uint8, device="cuda")
    work = torch.full((8 * wide_n,), 0xFF, dtype=torch.uint8, device="cuda")
    flags = torch.zeros((S * m,), dtype=torch.uint8, device="cuda")
    count = poison()
    wb = gpu.locate_work_bytes(S, k, m)
    bad_table = [ptrs[0]] * (k + m)  # breaks step 5 (overlap) wherever it is reached

    def digest(t=ptrs, a=ds, b=ps, SS=S, bb=bs, kk=k, mm=m, d=dig, sel=None):
        code = gpu.digest_shards(t, a, b, SS, bb, kk, mm, d, sel)
        assert gpu.shards_arg_capacity_used() == 0
        return code

    def locate(t=ptrs, a=ds, b=ps, SS=S, bb=bs, kk=k, mm=m, d=dig, f=flags, bmp=bitmap, cnt=count,
               w=work, wbytes=None):
        code = gpu.locate_shards(t, a, b, SS, bb, kk, mm, d, f, bmp, cnt, w,
                                 gpu.locate_work_bytes(SS, kk, mm) if wbytes is None else wbytes)
        assert gpu.shards_arg_capacity_used() == 0
        return code

    # 2. bs, then k and m, before the call's own pointers and the table
    assert digest(t=None, bb=100, kk=6, mm=4, d=None) == St.INVALID_SIZE
    assert digest(t=None, kk=6, mm=4, d=None) == St.INVALID_COUNTS
    assert locate(t=None, bb=100, kk=6, mm=4, d=None, w=None) == St.INVALID_SIZE
    assert locate(t=bad_table, kk=6, mm=4, w=None, wbytes=0) == St.INVALID_COUNTS
    # 3. the call's own pointers and sizes, in the batch call's order, before the table
    for t in (ptrs, bad_table, None):
        assert digest(t=t, d=None) == St.INVALID_SIZE
        assert digest(t=t, d=dig.data_ptr() + 4) == St.INVALID_ALIGNMENT
        assert locate(t=t, d=None, w=work.data_ptr() + 4) == St.INVALID_SIZE
        assert locate(t=t, w=None, d=dig.data_ptr() + 4) == St.INVALID_SIZE
        assert locate(t=t, wbytes=wb - 1, cnt=count.data_ptr() + 2) == St.INVALID_SIZE
        assert locate(t=t, d=dig.data_ptr() + 4, bmp=None) == St.INVALID_ALIGNMENT
        assert locate(t=t, w=work.data_ptr() + 4, bmp=None) == St.INVALID_ALIGNMENT
        assert locate(t=t, cnt=count.data_ptr() + 2, bmp=None) == St.INVALID_ALIGNMENT
        assert locate(t=t, bmp=None) == St.INVALID_SIZE
    # ... and with no stripes the alignment is still asked, ahead of step 4
    assert digest(t=None, SS=0, d=dig.data_ptr() + 4) == St.INVALID_ALIGNMENT
    assert locate(t=None, SS=0, cnt=count.data_ptr() + 2) == St.INVALID_ALIGNMENT
    # 5. steps 3 to 7 of xec_check_shards
    wide = (ptrs * 52)[:257]
    tables = [
        ((wide, ds, ps, 256, 1), St.INVALID_SIZE),
        ((None, ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:2] + [None] + ptrs[3:], ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:2] + [ptrs[2] + 16] + ptrs[3:], ds, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, ds + 32, ps, k, m), St.INVALID_ALIGNMENT),
        ((ptrs, bs - 64, ps, k, m), St.INVALID_SIZE),
        ((ptrs, ds, 1 << 62, k, m), St.INVALID_SIZE),
        ((ptrs[:3] + [ptrs[0]] + ptrs[4:], ds, ps, k, m), St.INVALID_SIZE),
        ((ptrs[:-1] + [ptrs[1] + 64], ds, ps, k, m), St.INVALID_SIZE),  # parity inside a data hull
    ]
    for (t, a, b, kk, mm), code in tables:
        assert gpu.check_shards(t, a, b, S, bs, kk, mm) == code
        assert digest(t=t, a=a, b=b, kk=kk, mm=mm) == code
        assert locate(t=t, a=a, b=b, kk=kk, mm=mm, f=None) == code
    torch.cuda.synchronize()
    st.assert_image(before, "after rejected calls")
    assert int(count.item()) == POISON
    assert bool((dig == FILL).all()) and bool((bitmap == 0xFF).all()) and bool((work == 0xFF).all())
    # 4. no stripes: success; the digest queues nothing, the locate its count alone
    assert digest(t=None, SS=0) == St.SUCCESS and digest(t=None, SS=0, d=None) == St.SUCCESS
    torch.cuda.synchronize()
    assert bool((dig == FILL).all()) and int(count.item()) == POISON
    assert locate(t=None, SS=0, d=None, bmp=None, w=None, cnt=None) == St.SUCCESS
    assert locate(t=bad_table, SS=0) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    assert bool((dig == FILL).all()) and bool((bitmap == 0xFF).all()) and bool((work == 0xFF).all())
    st.assert_image(before, "after calls without stripes")
    # and the accepted calls work from this state
    bm, n_bad = run_locate(gpu, st, stored(ref_digests(S, k, m, bs)))
    assert n_bad == 0 and np.array_equal(bm, expect_bitmap(lay, []))


# -- 8. kernel events -------------------------------------------------------------------
def test_kernel_events_time_the_digest_kernel_of_both_calls(gpu):
    torch = _torch()
    S, k, m, bs = 7, 16, 1, 65536
    blocks = pristine(S, k, m, bs)
    ref = ref_digests(S, k, m, bs)
    lay = Layout(S, k, m, bs, "C")
    clean = lay.image(blocks)
    st = Store(lay, clean)
    s = torch.cuda.current_stream()
    n = S * (k + m)
    wb = gpu.locate_work_bytes(S, k, m)
    work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
    bitmap = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    count = poison()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for call in ("digest", "locate"):
        e0.record(s)  # torch creates the HIP handle at the first record
        e1.record(s)
        torch.cuda.synchronize()
        dig = slots(n)

        def run():
            if call == "digest":
                return gpu.digest_shards(*st.args, dig, None, s)
            return gpu.locate_shards(*st.args, stored(ref), None, bitmap, count, work, wb, s)

        assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
        assert run() == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        assert t > 0, call
        # reads S*(k+m)*bs bytes: slower than HBM could, so it is the kernel's own interval
        assert S * (k + m) * bs / (t * 1e-3) / 1e9 < 8000.0, call
        assert run() == gpu.Status.SUCCESS  # not armed any more
        torch.cuda.synchronize()
        assert e0.elapsed_time(e1) == t, call
        if call == "digest":
            assert np.array_equal(as_u64(dig), ref.reshape(-1))
        else:
            assert int(count.item()) == 0 and bool((bitmap == 1).all())
    st.assert_image(clean, "timed digest and locate")
