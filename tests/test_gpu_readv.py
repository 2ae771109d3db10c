"""Vectored degraded read on an MI355X: xec_readv (host bitmap and entries) and
xec_readv_device (both on the device), a range per entry.

The expected bytes of every case are the PRISTINE batch before erasure,

    want = concat over t of original[c_t, i_t][offset_t : offset_t + len_t]

with the parity computed by numpy (tests/test_gpu_read.py's Batch); the library
is never the source of an expectation.  Before a call every lost block holds
0xEE on the device, so a kernel that reads a lost block delivers wrong bytes.
d_out sits between two 64-byte guards of a sentinel.  After every accepted call
data, parity and the bitmaps are byte-identical to copies taken before it and
the guards are intact; after every rejected or failed call d_out holds its
sentinel throughout.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_read import (ARG_LIST, BSS, GARBAGE, GUARD, KMS, LIST, SENTINEL, Batch, Out,
                           host_read)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _xec():
    import xec
    return xec


def make_iov(items, offsets, lengths):
    a = np.zeros(len(items), dtype=_xec().IOV)
    a["item"], a["offset"], a["len"] = items, offsets, lengths
    return a


def mixed_iov(b: Batch, rng, n):
    """n entries over Batch.mixed_items (unordered, data and parity, present and
    lost, duplicates), each with a range drawn from lengths below, at and just
    past one 1 KiB tile, with ragged tails and starts off the tile boundaries."""
    bs = b.bs
    lens = [x for x in (16, 1008, 1024, 1040, 2064, bs) if x <= bs]
    items = b.mixed_items(rng, n)
    if n >= 8:  # stripe 1 is intact in the batch's pattern: a present parity and a present data block
        items[2], items[3] = (1 << 8) | b.k, (1 << 8) | 0
    ln = rng.choice(lens, size=n)
    off = np.zeros(n, np.int64)
    for t in range(n):
        offs = [o for o in (0, 16, 1008, bs - ln[t]) if 0 <= o and o + ln[t] <= bs]
        off[t] = offs[int(rng.integers(len(offs)))]
    if n >= 4:  # the duplicates (mixed_items: n-1 of 0, n-2 of n//2) with ranges of their own
        ln[0], off[0], ln[n - 1], off[n - 1] = 16, 0, lens[-1], 0
        ln[n // 2], off[n // 2], ln[n - 2], off[n - 2] = lens[-1], 0, 16, bs - 16
        ln[1] = lens[1]  # a neighbour of entry 0 with another length
        off[1] = min(off[1], bs - ln[1])
    return make_iov(items, off, ln)


def want_bytes(b: Batch, iov):
    return np.concatenate([b.blocks[int(e["item"]) >> 8, int(e["item"]) & 0xFF,
                                    int(e["offset"]):int(e["offset"]) + int(e["len"])] for e in iov])


class VOut:
    """total bytes of d_out between two guards, all SENTINEL."""

    def __init__(self, total):
        torch = _torch()
        self.total = int(total)
        self.buf = torch.full((GUARD + self.total + GUARD,), SENTINEL, dtype=torch.uint8,
                              device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def body(self):
        return self.buf[GUARD:GUARD + self.total].cpu().numpy()

    def guards_intact(self):
        b = self.buf
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())

    def all_sentinel(self):
        return bool((self.buf == SENTINEL).all())


def total_of(iov):
    return int(iov["len"].astype(np.int64).sum())


def guarded(nbytes):
    """nbytes of device memory between two sentinel guards: (buffer, pointer)."""
    torch = _torch()
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def guards_of(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def host_readv(xec, b: Batch, iov, out: VOut, bm="own", scratch="auto", out_bytes=None, stream=None):
    torch = _torch()
    n = len(iov)
    h_bm = b.bm.reshape(-1) if isinstance(bm, str) else bm
    d_scratch, sbytes, keep = None, 0, None
    if scratch == "auto" and n > 256:
        sbytes = xec.readv_scratch_bytes(n)
        keep, d_scratch = guarded(sbytes)
    elif scratch != "auto":
        d_scratch, sbytes = scratch
    st = xec.readv(b.d, b.p, b.S, b.bs, b.k, b.m, h_bm, iov, n, out.ptr,
                   out.total if out_bytes is None else out_bytes, d_scratch, sbytes,
                   b.stream if stream is None else stream)
    torch.cuda.synchronize()
    if keep is not None:
        assert guards_of(keep), "a guard byte of d_scratch was written"
    return st


def device_readv(xec, b: Batch, iov, out: VOut, bm="own", out_bytes=None, status=None):
    torch = _torch()
    n = len(iov)
    d_iov = torch.from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")
    d_bm = b.d_bm if isinstance(bm, str) else bm
    if status is None:
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wbytes = xec.readv_device_work_bytes(n)
    keep, d_work = guarded(wbytes)
    st = xec.readv_device(b.d, b.p, b.S, b.bs, b.k, b.m, d_bm, d_iov, n, out.ptr,
                          out.total if out_bytes is None else out_bytes, d_work, wbytes, status,
                          b.stream)
    torch.cuda.synchronize()
    assert guards_of(keep), "a guard byte of d_work was written"
    return st, int(status.item())


def check_served(b: Batch, iov, out: VOut, what):
    got, want = out.body(), want_bytes(b, iov)
    if not np.array_equal(got, want):
        ends = np.cumsum(iov["len"].astype(np.int64))
        first = int(np.flatnonzero(got != want)[0])
        t = int(np.searchsorted(ends, first, side="right"))
        raise AssertionError(f"{what}: byte {first} differs from the pristine batch, entry {t} = "
                             f"{iov[t]}")
    assert out.guards_intact(), f"{what}: a guard byte of d_out was written"
    b.assert_untouched(what)


# -------------------------------------------------------------------------- 1
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_mixed_lists_are_the_pristine_slices_in_list_order(gpu, k, m, bs):
    S = KMS[(k, m)]
    b = Batch.get(S, k, m, bs)
    iov = mixed_iov(b, np.random.default_rng(k + m + bs), 37)
    items = iov["item"]
    lost = b.bm[items >> 8, items & 0xFF] == 0
    assert (lost & ((items & 0xFF) >= k)).any() and (lost & ((items & 0xFF) < k)).any()
    assert (~lost & ((items & 0xFF) >= k)).any() and (~lost & ((items & 0xFF) < k)).any()
    for t, u in ((0, 36), (18, 35)):  # two duplicates with different ranges
        assert iov[t]["item"] == iov[u]["item"]
        assert (iov[t]["offset"], iov[t]["len"]) != (iov[u]["offset"], iov[u]["len"])
    assert iov[0]["len"] != iov[1]["len"]  # neighbours whose lengths differ
    assert ((iov["offset"].astype(np.int64) + iov["len"]) <= bs).all() and len(set(iov["len"])) > 1
    total = total_of(iov)
    assert gpu.check_readv(b.bm.reshape(-1), S, bs, k, m, iov, len(iov)) == (0, int(lost.sum()), total)
    what = f"{k}+{m} x {bs} x {S}"
    out = VOut(total)
    assert host_readv(gpu, b, iov, out) == gpu.Status.SUCCESS, what
    assert gpu.readv_tiling_used() == ARG_LIST
    check_served(b, iov, out, "xec_readv " + what)
    out_d = VOut(total)
    assert device_readv(gpu, b, iov, out_d) == (gpu.Status.SUCCESS, 0), what
    assert gpu.readv_tiling_used() == LIST
    check_served(b, iov, out_d, "xec_readv_device " + what)


# -------------------------------------------------------------------------- 2
def test_equal_ranges_are_byte_identical_to_xec_read(gpu):
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    items = b.mixed_items(np.random.default_rng(21), 70)
    for offset, length in [(1008, 2064), (0, bs), (bs - 16, 16)]:
        ref = Out(len(items), length)
        assert host_read(gpu, b, items, offset, length, ref) == gpu.Status.SUCCESS
        iov = make_iov(items, offset, length)
        out = VOut(len(items) * length)
        assert host_readv(gpu, b, iov, out) == gpu.Status.SUCCESS
        check_served(b, iov, out, f"equal ranges [{offset}, +{length})")
        assert np.array_equal(out.body(), ref.body().reshape(-1))
        out_d = VOut(len(items) * length)
        assert device_readv(gpu, b, iov, out_d) == (gpu.Status.SUCCESS, 0)
        assert np.array_equal(out_d.body(), ref.body().reshape(-1))


# -------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1025])
def test_host_entry_counts_at_the_capacity_boundaries(gpu, n):
    """64 and 256 are the kernel-argument capacities; past 256 the table is
    uploaded into d_scratch."""
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    iov = mixed_iov(b, np.random.default_rng(n), n)
    if n == 1:
        iov[0] = ((2 << 8) | 0, 1008, 2064)  # the one entry is a lost data block
    out = VOut(total_of(iov))
    assert host_readv(gpu, b, iov, out) == gpu.Status.SUCCESS
    assert gpu.readv_tiling_used() == (ARG_LIST if n <= 256 else LIST)
    check_served(b, iov, out, f"xec_readv n={n}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_device_entry_counts_across_the_scan_passes(gpu, n):
    """The scan kernel walks the list in passes of 256 entries."""
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    iov = mixed_iov(b, np.random.default_rng(1000 + n), n)
    if n == 1:
        iov[0] = ((0 << 8) | k, 16, 1040)  # the one entry is a lost parity block
    out = VOut(total_of(iov))
    assert device_readv(gpu, b, iov, out) == (gpu.Status.SUCCESS, 0)
    assert gpu.readv_tiling_used() == LIST
    check_served(b, iov, out, f"xec_readv_device n={n}")


# -------------------------------------------------------------------------- 4
def test_upload_path_needs_its_scratch_and_the_device_form_its_work(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St = gpu.Status
    n = 257
    iov = mixed_iov(b, np.random.default_rng(5), n)
    out = VOut(total_of(iov))
    need = gpu.readv_scratch_bytes(n)
    keep, ptr = guarded(need + 8)
    assert host_readv(gpu, b, iov, out, scratch=(ptr + 2, need)) == St.INVALID_ALIGNMENT
    assert host_readv(gpu, b, iov, out, scratch=(None, need)) == St.INVALID_SIZE
    assert host_readv(gpu, b, iov, out, scratch=(ptr, need - 1)) == St.INVALID_SIZE
    assert gpu.readv_tiling_used() == 0 and out.all_sentinel()
    # the entries are judged first: one out of range outranks a missing scratch
    bad = iov.copy()
    bad[n - 1]["item"] = S << 8
    assert host_readv(gpu, b, bad, out, scratch=(None, 0)) == St.INVALID_COUNTS
    assert out.all_sentinel() and bool((keep == SENTINEL).all())
    # exactly the contract's bytes, at a 4-byte offset, inside the guards
    keep2, ptr2 = guarded(need + 4)
    assert host_readv(gpu, b, iov, out, scratch=(ptr2 + 4, need)) == St.SUCCESS
    assert gpu.readv_tiling_used() == LIST
    check_served(b, iov, out, "exact scratch at a 4-byte offset")
    assert bool((keep2[:GUARD + 4] == SENTINEL).all()) and bool((keep2[-GUARD:] == SENTINEL).all())
    # at 256 entries the scratch is not looked at
    out2 = VOut(total_of(iov[:256]))
    assert host_readv(gpu, b, iov[:256], out2, scratch=(1, 0)) == St.SUCCESS
    check_served(b, iov[:256], out2, "256 entries without scratch")

    # d_work of the device form: NULL, short, misaligned; exact inside guards is device_readv's
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    d_iov = torch.from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")
    wneed = gpu.readv_device_work_bytes(n)
    wkeep, wptr = guarded(wneed + 8)
    out3 = VOut(total_of(iov))

    def dev(work, wbytes):
        return gpu.readv_device(b.d, b.p, S, bs, k, m, b.d_bm, d_iov, n, out3.ptr, out3.total, work,
                                wbytes, status, b.stream)

    assert dev(None, wneed) == St.INVALID_SIZE
    assert dev(wptr, wneed - 1) == St.INVALID_SIZE
    assert dev(wptr + 4, wneed) == St.INVALID_ALIGNMENT
    torch.cuda.synchronize()
    assert gpu.readv_tiling_used() == 0 and out3.all_sentinel() and int(status.item()) == 77
    assert bool((wkeep == SENTINEL).all())
    assert device_readv(gpu, b, iov, out3) == (St.SUCCESS, 0)  # exactly wneed bytes, guarded
    check_served(b, iov, out3, "exact d_work")


# -------------------------------------------------------------------------- 5, 6
def test_every_check_in_order(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St, s = gpu.Status, b.stream
    ok = make_iov([(2 << 8) | 0, (0 << 8) | k, (1 << 8) | 3], [0, 16, 1008], [256, 1040, 2064])
    total = total_of(ok)
    out = VOut(total)
    flat = b.bm.reshape(-1)

    def host(d=None, p=None, SS=S, bb=bs, kk=k, mm=m, bm=flat, iov=ok, n=3, o=out.ptr, ob=total):
        st = gpu.readv(b.d if d is None else d, b.p if p is None else p, SS, bb, kk, mm, bm, iov, n,
                       o, ob, None, 0, s)
        assert gpu.readv_tiling_used() == 0
        return st

    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    d_ok = torch.from_numpy(ok.view(np.uint8).reshape(-1).copy()).to("cuda")
    wbytes = gpu.readv_device_work_bytes(3)
    work = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")

    def dev(SS=S, bb=bs, kk=k, mm=m, iov=d_ok, n=3, o=out.ptr, ob=total, stt=status, d=None,
            w=work, wb=wbytes):
        st = gpu.readv_device(b.d if d is None else d, b.p, SS, bb, kk, mm, b.d_bm, iov, n, o, ob,
                              w, wb, stt, s)
        assert gpu.readv_tiling_used() == 0
        return st

    def with_range(off, ln):
        e = ok.copy()
        e[1]["offset"], e[1]["len"] = off, ln
        return e

    # 2. xec_check_args, before everything that follows
    assert host(d=b.d.data_ptr() + 16, iov=None) == St.INVALID_ALIGNMENT
    assert host(bb=100, n=0) == St.INVALID_SIZE
    assert host(kk=6, mm=4, iov=None) == St.INVALID_COUNTS
    assert dev(d=b.d.data_ptr() + 16, stt=None) == St.INVALID_ALIGNMENT
    # 3. nothing to do, before the pointers are looked at
    assert host(n=0, o=None, iov=None) == St.SUCCESS
    assert host(SS=0, o=None, iov=with_range(8, 0)) == St.SUCCESS
    # 4. the packing and the 32-bit ranges
    assert host(kk=255, mm=5, o=None) == St.INVALID_SIZE
    assert host(SS=(1 << 24) + 1, o=None) == St.INVALID_SIZE
    assert host(bb=1 << 32, o=None) == St.INVALID_SIZE
    assert dev(kk=255, mm=5, o=None) == St.INVALID_SIZE
    assert dev(bb=1 << 32, o=None) == St.INVALID_SIZE
    # 5. NULL d_out or entries, before 6. d_out's alignment
    assert host(o=None) == St.INVALID_SIZE
    assert host(iov=None, o=out.ptr + 8) == St.INVALID_SIZE
    assert host(o=out.ptr + 8, iov=with_range(8, 0)) == St.INVALID_ALIGNMENT
    # 7. a broken range, before 8. the totals and the overlap
    for off, ln in [(0, 0), (8, 256), (0, 24), (bs - 16, 32), (bs, 16), (bs + 16, 16),
                    (0xFFFFFFF0, 32)]:
        assert host(iov=with_range(off, ln), ob=0) == St.INVALID_SIZE, (off, ln)
    # 8. capacity and overlap, before 9. the entries are judged
    far = ok.copy()
    far[2]["item"] = S << 8
    assert host(ob=total - 16, iov=far) == St.INVALID_SIZE
    assert host(o=b.d.data_ptr() + bs, iov=far) == St.INVALID_SIZE
    assert host(o=b.p.data_ptr() + S * m * bs - 16) == St.INVALID_SIZE
    assert host(o=b.d.data_ptr() - total + 16) == St.INVALID_SIZE  # ends inside the data
    # 9. an entry out of range outranks 10. an entry that is not servable
    dbl = flat.copy().reshape(S, k + m)
    dbl[1, 1] = dbl[1, 3] = 0  # stripe 1, class 1
    unserv = ok.copy()
    unserv[0]["item"] = (1 << 8) | 1
    assert host(bm=dbl.reshape(-1), iov=unserv) == St.DECODE_FAILURE
    both = unserv.copy()
    both[1]["item"] = k + m
    assert host(bm=dbl.reshape(-1), iov=both) == St.INVALID_COUNTS
    assert host(iov=far) == St.INVALID_COUNTS
    # the device form: d_status, then NULLs, work_bytes, alignments, overlap, the tile count
    assert dev(stt=None) == St.INVALID_ALIGNMENT
    assert dev(stt=status.data_ptr() + 2) == St.INVALID_ALIGNMENT
    assert dev(o=None) == St.INVALID_SIZE and dev(iov=None) == St.INVALID_SIZE
    assert dev(w=None, o=out.ptr + 8) == St.INVALID_SIZE
    assert dev(wb=wbytes - 1, o=out.ptr + 8) == St.INVALID_SIZE
    assert dev(o=out.ptr + 8) == St.INVALID_ALIGNMENT
    assert dev(iov=d_ok.data_ptr() + 2) == St.INVALID_ALIGNMENT
    assert dev(w=work.data_ptr() + 4, wb=wbytes - 4, o=b.p.data_ptr()) == St.INVALID_SIZE  # 6 before 7
    assert dev(o=b.p.data_ptr()) == St.INVALID_SIZE
    assert dev(o=b.d.data_ptr() - total + 16) == St.INVALID_SIZE
    assert dev(n=1 << 30, wb=1 << 40) == St.INVALID_SIZE  # 2^30 entries x 5 tiles of 1 KiB
    torch.cuda.synchronize()
    # nothing was queued: no byte of d_out, and not even *d_status = 0
    assert out.all_sentinel() and int(status.item()) == 77
    b.assert_untouched("after rejected calls")
    # an empty device read queues the verdict alone
    assert dev(n=0, iov=None, o=None, w=None, wb=0) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and out.all_sentinel()
    # and the accepted call works from this state, out_bytes exactly sum len
    assert host_readv(gpu, b, ok, out) == St.SUCCESS
    check_served(b, ok, out, "after the rejected calls")


def test_device_verdicts_their_maximum_and_the_capacity(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St = gpu.Status
    bm = b.bm.copy()
    bm[1] = 1
    bm[1, 1] = bm[1, k + 1] = 0  # stripe 1, class 1: a member and the parity
    d_bm = torch.from_numpy(np.ascontiguousarray(bm.reshape(-1))).to("cuda")
    good = [((2 << 8) | 0, 1008, 2064), ((0 << 8) | k, 0, 16), ((1 << 8) | 0, 16, 1024),
            ((1 << 8) | 3, bs - 1040, 1040)]
    far = [((S << 8) | 0, 0, 16), ((0xFFFFFF << 8) | 0xFF, 16, 32), (k + m, 0, 16)]  # never dereferenced
    unserv = [((1 << 8) | 1, 0, 16), ((1 << 8) | (k + 1), 16, 1040)]
    ranges = [((2 << 8) | 0, 8, 16), (5, 0, 0), (5, 0, 24), (5, bs - 16, 32), (5, 0xFFFFFFF0, 32),
              ((S << 8) | 0, 0, 0)]  # the last one breaks both rules: 3, the larger
    cases = [(good, 0), (good + ranges[:1], 1), (ranges[:5], 1), (good + ranges[5:], 3),
             (good + far[:1], 3), (far, 3), (good + ranges[:2] + far[:1], 3),
             (good + unserv[:1], 4), (unserv, 4), (far[:1] + good + unserv + ranges[:3] + far[1:], 4)]
    for entries, verdict in cases:
        iov = make_iov(*zip(*entries))
        valid = [e for e in entries if e[2] and e[2] % 16 == 0 and e[1] + e[2] <= bs]
        out = VOut(sum(e[2] for e in valid) + 64)
        assert device_readv(gpu, b, iov, out, bm=d_bm) == (St.SUCCESS, verdict), entries
        if verdict == 0:
            check = VOut(total_of(iov))
            assert device_readv(gpu, b, iov, check, bm=d_bm) == (St.SUCCESS, 0)
            check_served(b, iov, check, "verdict 0")
            assert bool((out.buf[GUARD + total_of(iov):] == SENTINEL).all())  # nothing past the total
        else:
            assert out.all_sentinel(), f"d_out written under verdict {verdict}"
    # sum len > out_bytes: 1, whatever the entries; exactly sum len is served
    iov = make_iov(*zip(*good))
    total = total_of(iov)
    out = VOut(total)
    assert device_readv(gpu, b, iov, out, bm=d_bm, out_bytes=total - 16) == (St.SUCCESS, 1)
    assert device_readv(gpu, b, iov, out, bm=d_bm, out_bytes=0) == (St.SUCCESS, 1)
    assert out.all_sentinel()
    assert device_readv(gpu, b, iov, out, bm=d_bm, out_bytes=total) == (St.SUCCESS, 0)
    check_served(b, iov, out, "out_bytes exactly the total")
    # the host form: the same capacity rule, and the bytes past the total keep their sentinel
    roomy = VOut(total + 4096)
    assert host_readv(gpu, b, iov, roomy, bm=np.ascontiguousarray(bm.reshape(-1))) == St.SUCCESS
    assert np.array_equal(roomy.body()[:total], want_bytes(b, iov))
    assert bool((roomy.buf[GUARD + total:] == SENTINEL).all())
    b.assert_untouched("after failed device reads")


# -------------------------------------------------------------------------- 7
def test_reads_are_served_where_repair_refuses(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    bm = b.bm.copy()
    bm[1] = 1
    bm[1, 0] = bm[1, 2] = 0  # stripe 1, class 0 doubly lost
    flat = np.ascontiguousarray(bm.reshape(-1))
    St = gpu.Status
    scratch = torch.empty(flat.size, dtype=torch.uint8, device="cuda")
    assert gpu.repair(b.d, b.p, S, bs, k, m, flat, scratch, b.stream) == St.DECODE_FAILURE
    torch.cuda.synchronize()
    b.assert_untouched("after the refused repair")
    iov = make_iov([(2 << 8) | 0, (1 << 8) | 4, (1 << 8) | k, (0 << 8) | k, (1 << 8) | 1, (2 << 8) | 0],
                   [1008, 0, 16, bs - 1040, 0, 0], [2064, 16, 1024, 1040, bs, 1008])
    out = VOut(total_of(iov))
    assert host_readv(gpu, b, iov, out, bm=flat) == St.SUCCESS
    check_served(b, iov, out, "beside a doubly-lost class")
    d_bm = torch.from_numpy(flat).to("cuda")
    out_d = VOut(total_of(iov))
    assert device_readv(gpu, b, iov, out_d, bm=d_bm) == (St.SUCCESS, 0)
    check_served(b, iov, out_d, "beside a doubly-lost class (device)")
    # its lost blocks are not servable, and then nothing is written at all
    worse = np.append(iov, make_iov([(1 << 8) | 2], [0], [16]))
    out2 = VOut(total_of(worse))
    assert host_readv(gpu, b, worse, out2, bm=flat) == St.DECODE_FAILURE
    assert gpu.readv_tiling_used() == 0 and out2.all_sentinel()
    assert device_readv(gpu, b, worse, out2, bm=d_bm) == (St.SUCCESS, 4)
    assert out2.all_sentinel()


# -------------------------------------------------------------------------- 8
@pytest.mark.parametrize("launch", [dict(block_threads=64), dict(block_threads=256),
                                    dict(unroll=1), dict(unroll=2), dict(cache_policy=1),
                                    dict(cache_policy=2), dict(max_grid=3),
                                    dict(block_threads=256, unroll=2, max_grid=3)],
                         ids=lambda d: "-".join(f"{a}{v}" for a, v in d.items()))
def test_launch_overrides_give_identical_bytes(gpu, launch):
    """Tile bytes from 1 KiB (64 x 1) to 8 KiB (256 x 2); max_grid = 3 strides
    three workgroups over every tile."""
    b = Batch.get(11, 6, 2, 4352)
    b66 = Batch.get(3, 66, 2, 4352)  # a member count without a compiled unroll
    b64k = Batch.get(5, 32, 4, 65536)  # entries of many tiles
    try:
        assert gpu.set_launch(**launch) == gpu.Status.SUCCESS
        for bb, n in ((b, 70), (b66, 70), (b64k, 300)):
            iov = mixed_iov(bb, np.random.default_rng(9), n)
            out = VOut(total_of(iov))
            assert host_readv(gpu, bb, iov, out) == gpu.Status.SUCCESS
            check_served(bb, iov, out, f"xec_readv under {launch}")
            out_d = VOut(total_of(iov))
            assert device_readv(gpu, bb, iov, out_d) == (0, 0)
            check_served(bb, iov, out_d, f"xec_readv_device under {launch}")
    finally:
        gpu.set_launch()
    try:  # rotation plays no part
        assert gpu.set_rotation(3) == gpu.Status.SUCCESS
        iov = mixed_iov(b, np.random.default_rng(10), 20)
        out = VOut(total_of(iov))
        assert host_readv(gpu, b, iov, out) == gpu.Status.SUCCESS
        check_served(b, iov, out, "under a rotation")
    finally:
        gpu.set_rotation(0)


# -------------------------------------------------------------------------- 9
def test_host_form_refuses_graph_capture(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    iov = make_iov([(2 << 8) | 0, 1], [0, 16], [256, 1024])
    out = VOut(total_of(iov))
    St = gpu.Status
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.readv(b.d, b.p, S, bs, k, m, b.bm.reshape(-1), iov, 2, out.ptr, out.total, None,
                         0, cs) == St.DEVICE_ERROR
        assert gpu.readv_tiling_used() == 0
        assert gpu.readv(b.d, b.p, S, bs, k, m, b.bm.reshape(-1), iov, 0, out.ptr, out.total, None,
                         0, cs) == St.SUCCESS
    g.replay()  # an empty graph
    torch.cuda.synchronize()
    del g
    assert out.all_sentinel()
    b.assert_untouched("after a refused capture")


def test_graph_of_readv_device_serves_the_entries_of_each_replay(gpu):
    """xec_readv_device captured once and replayed three times.  Every input is
    on the device before the capture; between the replays entries and bitmap
    are rewritten by device-to-device copies only (the constraint recorded at
    xec_verify).  The lengths change from replay to replay, and the totals with
    them; each replay serves what the buffers hold then."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    n = 300
    sel = [mixed_iov(b, np.random.default_rng(41 + r), n) for r in range(2)]
    held = np.concatenate([b.keep[0].cpu().numpy().reshape(S, k, bs),
                           b.keep[1].cpu().numpy().reshape(S, m, bs)], axis=1)
    third = sel[0].copy()
    third["len"][::2], third["offset"][::2] = 16, 0  # other lengths again, under a bitmap of no losses
    sels = sel + [third]
    totals = [total_of(x) for x in sels]
    assert len(set(totals)) == 3
    wants = [want_bytes(b, sels[0]), want_bytes(b, sels[1]),
             np.concatenate([held[int(e["item"]) >> 8, int(e["item"]) & 0xFF,
                                  int(e["offset"]):int(e["offset"]) + int(e["len"])] for e in third])]
    assert (wants[2] == GARBAGE).any()
    d_wants = [torch.from_numpy(np.ascontiguousarray(w)).to("cuda") for w in wants]
    d_sel = [torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to("cuda") for x in sels]
    d_bms = [b.d_bm.clone(), b.d_bm.clone(), torch.ones_like(b.d_bm)]
    d_iov, d_bm = d_sel[0].clone(), d_bms[0].clone()
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wbytes = gpu.readv_device_work_bytes(n)
    wkeep, wptr = guarded(wbytes)
    out = VOut(max(totals))
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.readv_device(b.d, b.p, S, bs, k, m, d_bm, d_iov, n, out.ptr, out.total, wptr,
                                wbytes, status, cs) == gpu.Status.SUCCESS
        assert gpu.readv_tiling_used() == LIST
    for r in range(3):
        d_iov.copy_(d_sel[r])
        d_bm.copy_(d_bms[r])
        out.buf.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == 0, r
        assert torch.equal(out.buf[GUARD:GUARD + totals[r]], d_wants[r]), f"replay {r}"
        assert bool((out.buf[GUARD + totals[r]:] == SENTINEL).all()) and out.guards_intact(), r
        assert guards_of(wkeep)
    del g
    b.assert_untouched("after the replays")


# -------------------------------------------------------------------------- 10
def test_past_4_gib(gpu):
    """16+1 x 1 MiB x 260 stripes: the last stripe starts past 4 GiB of data.
    (a) a handful of small ranges of it, one of a lost block, expected from that
    stripe's blocks alone; (b) 4,100 whole present blocks and then three small
    ranges: an output past 4 GiB, compared on the device with the source blocks."""
    torch = _torch()
    S, k, m, bs = 260, 16, 1, 1 << 20
    last = S - 1
    s = torch.cuda.current_stream()
    d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
    p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
    assert gpu.fill_splitmix64(d, S, k * bs, 4242, s) == 0
    assert gpu.encode(d, p, S, bs, k, m, s) == 0
    torch.cuda.synchronize()
    blocks = d.view(S, k, bs)
    tail = blocks[last].cpu().numpy()
    par = np.bitwise_xor.reduce(tail, axis=0)
    assert np.array_equal(p.view(S, bs)[last].cpu().numpy(), par)
    bm = np.ones((S, k + m), np.uint8)
    bm[last, 5] = 0
    bm[0, 5] = bm[0, 6] = 0  # and an unrecoverable stripe nobody asks for
    blocks[last, 5] = GARBAGE
    d_bm = torch.from_numpy(bm.reshape(-1)).to("cuda")
    src = {5: tail[5], k: par, 15: tail[15], 0: tail[0]}
    small = [(5, bs - 4096 - 16, 4096), (k, 16, 1040), (15, 0, 16), (5, 1008, 2064), (0, bs - 16, 16)]
    iov = make_iov([(last << 8) | i for i, _, _ in small], [o for _, o, _ in small],
                   [ln for _, _, ln in small])
    want = np.concatenate([src[i][o:o + ln] for i, o, ln in small])
    d_iov = torch.from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wbytes = gpu.readv_device_work_bytes(5000)
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    for form in ("host", "device"):  # (a)
        out = VOut(len(want))
        if form == "host":
            st = gpu.readv(d, p, S, bs, k, m, bm.reshape(-1), iov, len(iov), out.ptr, out.total,
                           None, 0, s)
        else:
            st = gpu.readv_device(d, p, S, bs, k, m, d_bm, d_iov, len(iov), out.ptr, out.total, work,
                                  wbytes, status, s)
        torch.cuda.synchronize()
        assert st == gpu.Status.SUCCESS and (form == "host" or int(status.item()) == 0)
        assert np.array_equal(out.body(), want) and out.guards_intact(), form
    # (b) present blocks only, from every part of the batch, repeats included
    rng = np.random.default_rng(77)
    n_big = 4100
    cs = rng.integers(1, S, n_big)
    cs[-1] = last
    is_ = rng.integers(0, k, n_big)
    is_[(cs == last) & (is_ == 5)] = 6
    big = make_iov(np.concatenate([(cs << 8) | is_, iov["item"][:3]]).astype(np.uint32),
                   np.concatenate([np.zeros(n_big, np.int64), iov["offset"][:3]]),
                   np.concatenate([np.full(n_big, bs, np.int64), iov["len"][:3]]))
    total = total_of(big)
    assert total > 1 << 32
    want_tail = want[:int(iov["len"][:3].sum())]
    d_want_tail = torch.from_numpy(want_tail).to("cuda")
    d_big = torch.from_numpy(big.view(np.uint8).reshape(-1).copy()).to("cuda")
    out = VOut(total)
    scratch = torch.empty(gpu.readv_scratch_bytes(len(big)), dtype=torch.uint8, device="cuda")
    sample = sorted(set([0, 1, 2047, 4094, 4095, 4096, n_big - 1] + rng.integers(0, n_big, 40).tolist()))
    for form in ("host", "device"):
        if form == "host":
            st = gpu.readv(d, p, S, bs, k, m, bm.reshape(-1), big, len(big), out.ptr, total, scratch,
                           scratch.numel(), s)
        else:
            out.buf.fill_(SENTINEL)
            st = gpu.readv_device(d, p, S, bs, k, m, d_bm, d_big, len(big), out.ptr, total, work,
                                  wbytes, status, s)
        torch.cuda.synchronize()
        assert st == gpu.Status.SUCCESS and (form == "host" or int(status.item()) == 0)
        body = out.buf[GUARD:GUARD + total]
        for t in sample:
            assert torch.equal(body[t * bs:(t + 1) * bs], blocks[int(cs[t]), int(is_[t])]), (form, t)
        assert torch.equal(body[n_big * bs:], d_want_tail), form
        assert out.guards_intact(), form
    assert bool((blocks[last, 5] == GARBAGE).all())  # the lost block was not written
    del d, p, out, blocks, body
    torch.cuda.empty_cache()


# -------------------------------------------------------------------------- 11
def test_kernel_events_cover_both_calls(gpu):
    """An armed pair is consumed by each call -- also one that launches nothing
    -- and times the read kernel: a positive interval."""
    torch = _torch()
    S, k, m, bs = 5, 32, 4, 65536
    b = Batch.get(S, k, m, bs)
    s = b.stream
    iov = mixed_iov(b, np.random.default_rng(7), 64)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    enc_p = torch.empty_like(b.p)  # an unarmed codec call between: encode into a spare buffer
    for entry in ("host", "device"):
        for e in ev:
            e.record(s)  # torch creates the HIP handle at the first record
        torch.cuda.synchronize()
        base = ev[0].elapsed_time(ev[1])
        assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
        out = VOut(total_of(iov))
        # an empty list launches nothing, but consumes the setting
        assert host_readv(gpu, b, iov[:0], out) == gpu.Status.SUCCESS
        assert gpu.encode(b.d, enc_p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed
        torch.cuda.synchronize()
        assert ev[0].elapsed_time(ev[1]) == base
        assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
        if entry == "host":
            assert host_readv(gpu, b, iov, out) == gpu.Status.SUCCESS
        else:
            assert device_readv(gpu, b, iov, out) == (gpu.Status.SUCCESS, 0)
        t_kernel = ev[0].elapsed_time(ev[1])
        assert t_kernel > 0 and t_kernel != base, entry
        check_served(b, iov, out, f"timed {entry} readv")
        assert gpu.encode(b.d, enc_p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed any more
        torch.cuda.synchronize()
        assert ev[0].elapsed_time(ev[1]) == t_kernel
