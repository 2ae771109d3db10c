"""Degraded read on an MI355X: xec_read (host bitmap and items) and
xec_read_device (both on the device).

The expected bytes of every case are the PRISTINE batch before erasure,

    want[t] = original[c, i][offset : offset + len]

with the parity computed by numpy; the library is never compared with itself.
Before a call every lost block is overwritten with 0xEE on the device, so a
kernel that reads a lost block delivers wrong bytes.  After every accepted
call data, parity and the bitmap are byte-identical to copies taken before it
and the 64 guard bytes on either side of d_out still hold their sentinel;
after every rejected or failed call d_out holds its sentinel throughout.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GARBAGE, SENTINEL, GUARD = 0xEE, 0x5C, 64
KMS = {(4, 1): 23, (16, 1): 7, (6, 2): 11, (66, 2): 3, (32, 4): 5}  # (k, m) -> stripes
BSS = [256, 4352, 65536]  # a quarter of a one-wave tile; 4 tiles and a ragged one; 64 tiles
ARG_LIST, LIST = 4, 3     # XEC_TILING_ARG_LIST, XEC_TILING_LIST


def _torch():
    import torch
    return torch


def ranges_for(bs):
    r = [(0, bs), (0, 16), (bs - 16, 16)]
    if bs >= 16 + 1024:
        r.append((16, 1024))
    if bs >= 1008 + 2064:
        r.append((1008, 2064))  # starts and ends off tile boundaries
    return r


class Batch:
    """A pristine batch in numpy (parity by numpy) and a damaged copy on the device."""
    cache: dict = {}

    @classmethod
    def get(cls, S, k, m, bs, pattern="classes"):
        key = (S, k, m, bs, pattern)
        if key not in cls.cache:
            cls.cache[key] = cls(S, k, m, bs, pattern)
        return cls.cache[key]

    def __init__(self, S, k, m, bs, pattern):
        torch = _torch()
        self.S, self.k, self.m, self.bs = S, k, m, bs
        rng = np.random.default_rng(S * 1_000_003 + k * 1009 + m * 31 + bs)
        data = rng.integers(0, 256, size=(S, k, bs), dtype=np.uint8)
        # block i is member i // m of class i % m
        par = np.bitwise_xor.reduce(data.reshape(S, k // m, m, bs), axis=1)
        self.blocks = np.concatenate([data, par], axis=1)  # (S, k+m, bs): the expectation
        bm = rng.choice(np.array([1, 2, 255], np.uint8), size=(S, k + m))
        if pattern == "classes":  # one block per class, parity included, in 2 stripes of 3
            for c in range(S):
                if c % 3 == 1:
                    continue
                for j in range(m):
                    cls_blocks = list(range(j, k, m)) + [k + j]
                    bm[c, cls_blocks[int(rng.integers(len(cls_blocks)))]] = 0
            bm[0, k] = 0  # a lost parity block and a lost data block for certain
            bm[0, 0:k:m] = 1
            if S > 2:
                bm[2, 0] = 0
                bm[2, m:k:m] = 1
                bm[2, k] = 1
        self.bm = np.ascontiguousarray(bm)
        self.stream = torch.cuda.current_stream()
        dmg = self.blocks.copy()
        dmg[self.bm == 0] = GARBAGE
        self.d = torch.from_numpy(np.ascontiguousarray(dmg[:, :k]).reshape(-1)).to("cuda")
        self.p = torch.from_numpy(np.ascontiguousarray(dmg[:, k:]).reshape(-1)).to("cuda")
        self.d_bm = torch.from_numpy(self.bm.reshape(-1)).to("cuda")
        self.keep = (self.d.clone(), self.p.clone(), self.d_bm.clone(), self.bm.copy())

    def assert_untouched(self, what):
        torch = _torch()
        assert torch.equal(self.d, self.keep[0]), f"data written {what}"
        assert torch.equal(self.p, self.keep[1]), f"parity written {what}"
        assert torch.equal(self.d_bm, self.keep[2]), f"device bitmap written {what}"
        assert np.array_equal(self.bm, self.keep[3]), f"host bitmap written {what}"

    def want(self, items, offset, length):
        it = np.asarray(items, dtype=np.int64)
        return self.blocks[it >> 8, it & 0xFF, offset:offset + length]

    def mixed_items(self, rng, n):
        """n items, unordered, data and parity, present and lost, with duplicates."""
        S, k, m = self.S, self.k, self.m
        lost = np.argwhere(self.bm == 0)
        pres = np.argwhere(self.bm != 0)
        pick = [lost[rng.integers(len(lost), size=n // 2)], pres[rng.integers(len(pres), size=n - n // 2)]]
        ci = np.concatenate(pick)
        ci = ci[rng.permutation(len(ci))]
        items = ((ci[:, 0] << 8) | ci[:, 1]).astype(np.uint32)
        if n >= 4:
            items[0] = (0 << 8) | k        # a lost parity block
            items[1] = (2 << 8) | 0 if S > 2 else items[1]  # a lost data block
            items[n - 1] = items[0]        # a duplicate of a lost item
            items[n - 2] = items[n // 2]   # and another
        return items


class Out:
    """n*length bytes of d_out between two guards, all SENTINEL."""

    def __init__(self, n, length):
        torch = _torch()
        self.n, self.length = n, length
        self.buf = torch.full((GUARD + n * length + GUARD,), SENTINEL, dtype=torch.uint8,
                              device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def body(self):
        return self.buf[GUARD:GUARD + self.n * self.length].cpu().numpy().reshape(self.n, self.length)

    def guards_intact(self):
        b = self.buf
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())

    def all_sentinel(self):
        return bool((self.buf == SENTINEL).all())


def host_read(xec, b: Batch, items, offset, length, out: Out, bm="own", scratch="auto", stream=None):
    torch = _torch()
    items = np.ascontiguousarray(items, dtype=np.uint32)
    n = len(items)
    h_bm = b.bm.reshape(-1) if isinstance(bm, str) else bm
    d_scratch, sbytes = None, 0
    if scratch == "auto" and n > 1024:
        sbytes = xec.read_scratch_bytes(n)
        d_scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    elif scratch != "auto":
        d_scratch, sbytes = scratch
    st = xec.read(b.d, b.p, b.S, b.bs, b.k, b.m, h_bm, items, n, offset, length, out.ptr,
                  d_scratch, sbytes, b.stream if stream is None else stream)
    torch.cuda.synchronize()
    return st


def device_read(xec, b: Batch, items, offset, length, out: Out, bm="own", status=None):
    torch = _torch()
    d_items = torch.from_numpy(np.ascontiguousarray(items, dtype=np.uint32).view(np.int32)).to("cuda")
    d_bm = b.d_bm if isinstance(bm, str) else bm
    if status is None:
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    st = xec.read_device(b.d, b.p, b.S, b.bs, b.k, b.m, d_bm, d_items, len(items), offset, length,
                         out.ptr, status, b.stream)
    torch.cuda.synchronize()
    return st, int(status.item())


def check_served(b: Batch, items, offset, length, out: Out, what):
    got, want = out.body(), b.want(items, offset, length)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(items)} items differ from the pristine "
                           f"batch, first t={bad[0]} item={int(items[bad[0]]):#x}")
    assert out.guards_intact(), f"{what}: a guard byte of d_out was written"
    b.assert_untouched(what)


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_ranges_of_mixed_items_are_the_pristine_bytes(gpu, k, m, bs):
    S = KMS[(k, m)]
    b = Batch.get(S, k, m, bs)
    rng = np.random.default_rng(k + m + bs)
    items = b.mixed_items(rng, 37)
    lost = b.bm[items >> 8, items & 0xFF] == 0
    assert lost.any() and (~lost).any()
    assert (lost & ((items & 0xFF) >= k)).any() and (lost & ((items & 0xFF) < k)).any()
    assert np.any(np.diff(items.astype(np.int64)) < 0) and len(set(items.tolist())) < len(items)
    assert gpu.check_read_items(b.bm.reshape(-1), S, k, m, items, len(items)) == (0, int(lost.sum()))
    for offset, length in ranges_for(bs):
        what = f"{k}+{m} x {bs} x {S} [{offset}, +{length})"
        out = Out(len(items), length)
        assert host_read(gpu, b, items, offset, length, out) == gpu.Status.SUCCESS, what
        assert gpu.read_tiling_used() == ARG_LIST
        check_served(b, items, offset, length, out, "xec_read " + what)
        out_d = Out(len(items), length)
        assert device_read(gpu, b, items, offset, length, out_d) == (gpu.Status.SUCCESS, 0), what
        assert gpu.read_tiling_used() == LIST
        check_served(b, items, offset, length, out_d, "xec_read_device " + what)
        assert np.array_equal(out.body(), out_d.body())


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1024, 1025])
def test_item_counts_at_the_capacity_boundaries(gpu, n):
    """64 / 256 / 1024 are the kernel-argument capacities; 1,025 items are
    uploaded into d_scratch.  The range is off the tile boundaries at both ends."""
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    rng = np.random.default_rng(n)
    items = b.mixed_items(rng, n)
    if n == 1:
        items[0] = (2 << 8) | 0  # the one item is a lost data block
    for offset, length in [(1008, 2064), (bs - 16, 16)]:
        out = Out(n, length)
        assert host_read(gpu, b, items, offset, length, out) == gpu.Status.SUCCESS
        assert gpu.read_tiling_used() == (ARG_LIST if n <= 1024 else LIST)
        check_served(b, items, offset, length, out, f"xec_read n={n}")
        out_d = Out(n, length)
        assert device_read(gpu, b, items, offset, length, out_d) == (gpu.Status.SUCCESS, 0)
        assert gpu.read_tiling_used() == LIST
        check_served(b, items, offset, length, out_d, f"xec_read_device n={n}")


def test_upload_path_needs_its_scratch(gpu):
    """Step 11 of the checks: only lists past 1,024 items look at d_scratch."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St = gpu.Status
    n = 1025
    items = b.mixed_items(np.random.default_rng(5), n)
    need = gpu.read_scratch_bytes(n)
    scratch = torch.empty(need + 8, dtype=torch.uint8, device="cuda")
    out = Out(n, 16)
    assert host_read(gpu, b, items, 0, 16, out, scratch=(scratch.data_ptr() + 2, need)) == St.INVALID_ALIGNMENT
    assert host_read(gpu, b, items, 0, 16, out, scratch=(None, need)) == St.INVALID_SIZE
    assert host_read(gpu, b, items, 0, 16, out, scratch=(scratch, need - 1)) == St.INVALID_SIZE
    assert gpu.read_tiling_used() == 0 and out.all_sentinel()
    # the items are judged first: an unservable one outranks a missing scratch
    bad = items.copy()
    bad[n - 1] = (S << 8)
    assert host_read(gpu, b, bad, 0, 16, out, scratch=(None, 0)) == St.INVALID_COUNTS
    assert out.all_sentinel()
    assert host_read(gpu, b, items, 0, 16, out, scratch=(scratch.data_ptr() + 4, need)) == St.SUCCESS
    assert gpu.read_tiling_used() == LIST
    check_served(b, items, 0, 16, out, "exact scratch at a 4-byte offset")
    # at 1,024 items the scratch is not looked at
    out2 = Out(1024, 16)
    assert host_read(gpu, b, items[:1024], 0, 16, out2, scratch=(1, 0)) == St.SUCCESS
    check_served(b, items[:1024], 0, 16, out2, "1,024 items without scratch")


def test_every_check_in_order(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St, s = gpu.Status, b.stream
    ok = np.array([(2 << 8) | 0, (0 << 8) | k, (1 << 8) | 3], np.uint32)
    out = Out(3, 256)
    flat = b.bm.reshape(-1)

    def host(d=None, p=None, SS=S, bb=bs, kk=k, mm=m, bm=flat, items=ok, n=3, off=0, ln=256,
             o=out.ptr):
        st = gpu.read(b.d if d is None else d, b.p if p is None else p, SS, bb, kk, mm, bm, items,
                      n, off, ln, o, None, 0, s)
        assert gpu.read_tiling_used() == 0
        return st

    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    d_ok = torch.from_numpy(ok.view(np.int32)).to("cuda")

    def dev(SS=S, bb=bs, kk=k, mm=m, items=d_ok, n=3, off=0, ln=256, o=out.ptr, stt=status,
            d=None):
        st = gpu.read_device(b.d if d is None else d, b.p, SS, bb, kk, mm, b.d_bm, items, n, off,
                             ln, o, stt, s)
        assert gpu.read_tiling_used() == 0
        return st

    # 2. xec_check_args, before everything that follows
    assert host(d=b.d.data_ptr() + 16, ln=0) == St.INVALID_ALIGNMENT
    assert host(bb=100, n=0) == St.INVALID_SIZE
    assert host(kk=6, mm=4, items=None) == St.INVALID_COUNTS
    assert dev(d=b.d.data_ptr() + 16, stt=None) == St.INVALID_ALIGNMENT
    # 3. nothing to do, before the range and the pointers are looked at
    assert host(n=0, ln=0, o=None, items=None) == St.SUCCESS
    assert host(SS=0, off=8, o=None) == St.SUCCESS
    # 4. the packing
    assert host(kk=255, mm=5, o=None) == St.INVALID_SIZE
    assert host(SS=(1 << 24) + 1, ln=0) == St.INVALID_SIZE
    assert dev(kk=255, mm=5) == St.INVALID_SIZE
    # 5. the range
    for off, ln in [(0, 0), (8, 256), (0, 24), (bs - 16, 32), (bs, 16), (bs + 16, 16)]:
        assert host(off=off, ln=ln, o=None) == St.INVALID_SIZE, (off, ln)
        assert dev(off=off, ln=ln) == St.INVALID_SIZE, (off, ln)
    # 6. NULL d_out or items
    assert host(o=None) == St.INVALID_SIZE
    assert host(items=None, o=out.ptr + 8) == St.INVALID_SIZE
    assert dev(o=None) == St.INVALID_SIZE and dev(items=None) == St.INVALID_SIZE
    # 7. d_out's alignment, before the overlap
    assert host(o=b.d.data_ptr() + 8) == St.INVALID_ALIGNMENT
    assert dev(o=out.ptr + 8) == St.INVALID_ALIGNMENT
    assert dev(items=d_ok.data_ptr() + 2) == St.INVALID_ALIGNMENT
    # 8. d_out on the data or the parity range, before the items are judged
    bad = np.array([(S << 8), 0, 0], np.uint32)
    assert host(o=b.d.data_ptr() + bs, items=bad) == St.INVALID_SIZE
    assert host(o=b.p.data_ptr() + S * m * bs - 16) == St.INVALID_SIZE
    assert host(o=b.d.data_ptr() - 2 * 256 - 16) == St.INVALID_SIZE  # ends inside the data
    assert dev(o=b.p.data_ptr()) == St.INVALID_SIZE
    # 9. an item out of range outranks 10. an item that is not servable
    dbl = flat.copy().reshape(S, k + m)
    dbl[1, 1] = dbl[1, 3] = 0  # stripe 1, class 1
    unserv = np.array([(1 << 8) | 1, 0, 0], np.uint32)
    assert host(bm=dbl.reshape(-1), items=unserv) == St.DECODE_FAILURE
    assert host(bm=dbl.reshape(-1), items=np.array([(1 << 8) | 1, (S << 8), 0], np.uint32)) == St.INVALID_COUNTS
    assert host(items=np.array([0, 0, k + m], np.uint32)) == St.INVALID_COUNTS
    # d_status: NULL or misaligned
    assert dev(stt=None) == St.INVALID_ALIGNMENT
    assert dev(stt=status.data_ptr() + 2) == St.INVALID_ALIGNMENT
    torch.cuda.synchronize()
    # nothing was queued: no byte of d_out, and not even *d_status = 0
    assert out.all_sentinel() and int(status.item()) == 77
    b.assert_untouched("after rejected calls")
    # an empty device read queues the verdict alone
    assert dev(n=0, items=None, o=None) == St.SUCCESS
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and out.all_sentinel()
    # and the accepted call works from this state
    assert host_read(gpu, b, ok, 0, 256, out) == St.SUCCESS
    check_served(b, ok, 0, 256, out, "after the rejected calls")


def test_reads_are_served_where_repair_refuses(gpu):
    """Another stripe has a doubly-lost class: xec_repair refuses the batch,
    xec_read serves every item that is not a lost block of that class --
    present blocks of the broken class included."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    bm = b.bm.copy()
    bm[1] = 1
    bm[1, 0] = bm[1, 2] = 0  # stripe 1 is intact in the batch's own pattern: class 0 doubly lost
    flat = np.ascontiguousarray(bm.reshape(-1))
    St = gpu.Status
    scratch = torch.empty(flat.size, dtype=torch.uint8, device="cuda")
    # repair is asked first and must leave the (shared, read-only) buffers alone
    assert gpu.repair(b.d, b.p, S, bs, k, m, flat, scratch, b.stream) == St.DECODE_FAILURE
    torch.cuda.synchronize()
    b.assert_untouched("after the refused repair")
    items = np.array([(2 << 8) | 0, (1 << 8) | 4, (1 << 8) | k, (0 << 8) | k, (1 << 8) | 1,
                      (2 << 8) | 0], np.uint32)
    out = Out(len(items), 2064)
    assert host_read(gpu, b, items, 1008, 2064, out, bm=flat) == St.SUCCESS
    check_served(b, items, 1008, 2064, out, "beside a doubly-lost class")
    d_bm = torch.from_numpy(flat).to("cuda")
    out_d = Out(len(items), 2064)
    assert device_read(gpu, b, items, 1008, 2064, out_d, bm=d_bm) == (St.SUCCESS, 0)
    check_served(b, items, 1008, 2064, out_d, "beside a doubly-lost class (device)")
    # its lost blocks are not servable, and then nothing is written at all
    worse = np.append(items, np.uint32((1 << 8) | 2))
    out2 = Out(len(worse), 2064)
    assert host_read(gpu, b, worse, 1008, 2064, out2, bm=flat) == St.DECODE_FAILURE
    assert gpu.read_tiling_used() == 0 and out2.all_sentinel()
    assert device_read(gpu, b, worse, 1008, 2064, out2, bm=d_bm) == (St.SUCCESS, 4)
    assert out2.all_sentinel()


def test_device_verdicts_and_the_pure_gather(gpu):
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    St = gpu.Status
    bm = b.bm.copy()
    bm[1] = 1
    bm[1, 1] = bm[1, k + 1] = 0  # stripe 1, class 1: a member and the parity
    d_bm = torch.from_numpy(np.ascontiguousarray(bm.reshape(-1))).to("cuda")
    good = [(2 << 8) | 0, (0 << 8) | k, (1 << 8) | 0, (1 << 8) | 3]
    far = [(S << 8) | 0, (0xFFFFFF << 8) | 0xFF, (0 << 8) | (k + m)]  # never dereferenced
    unserv = [(1 << 8) | 1, (1 << 8) | (k + 1)]
    for items, verdict in [(good, 0), (good + far[:1], 3), (far, 3), (good + unserv[:1], 4),
                           (unserv, 4), (far[:1] + good + unserv + far[1:], 4)]:
        items = np.array(items, np.uint32)
        out = Out(len(items), 1024)
        assert device_read(gpu, b, items, 16, 1024, out, bm=d_bm) == (St.SUCCESS, verdict)
        if verdict == 0:
            check_served(b, items, 16, 1024, out, "verdict 0")
        else:
            assert out.all_sentinel(), f"d_out written under verdict {verdict}"
    b.assert_untouched("after failed device reads")
    # NULL bitmaps: a pure gather of whatever the blocks hold -- the garbage included
    items = b.mixed_items(np.random.default_rng(3), 50)
    held = np.concatenate([b.keep[0].cpu().numpy().reshape(S, k, bs),
                           b.keep[1].cpu().numpy().reshape(S, m, bs)], axis=1)
    want = held[items >> 8, items & 0xFF, 1008:1008 + 2064]
    assert (want == GARBAGE).all(axis=1).any()
    for entry in ("host", "device"):
        out = Out(len(items), 2064)
        if entry == "host":
            assert host_read(gpu, b, items, 1008, 2064, out, bm=None) == St.SUCCESS
            assert gpu.read_tiling_used() == ARG_LIST
        else:
            assert device_read(gpu, b, items, 1008, 2064, out, bm=None) == (St.SUCCESS, 0)
        assert np.array_equal(out.body(), want), entry
        assert out.guards_intact()
    b.assert_untouched("after the gathers")


@pytest.mark.parametrize("launch", [dict(block_threads=64), dict(block_threads=256),
                                    dict(unroll=1), dict(unroll=2), dict(cache_policy=1),
                                    dict(cache_policy=2), dict(max_grid=3),
                                    dict(block_threads=256, unroll=2, max_grid=3)],
                         ids=lambda d: "-".join(f"{a}{v}" for a, v in d.items()))
def test_launch_overrides_give_identical_bytes(gpu, launch):
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    b66 = Batch.get(3, 66, 2, 4352)  # a member count without a compiled unroll
    try:
        assert gpu.set_launch(**launch) == gpu.Status.SUCCESS
        for bb in (b, b66):
            items = bb.mixed_items(np.random.default_rng(9), 70)
            for offset, length in [(1008, 2064), (0, bs), (bs - 16, 16)]:
                out = Out(len(items), length)
                assert host_read(gpu, bb, items, offset, length, out) == gpu.Status.SUCCESS
                check_served(bb, items, offset, length, out, f"xec_read under {launch}")
                out_d = Out(len(items), length)
                assert device_read(gpu, bb, items, offset, length, out_d) == (0, 0)
                check_served(bb, items, offset, length, out_d, f"xec_read_device under {launch}")
    finally:
        gpu.set_launch()
    # rotation plays no part
    try:
        assert gpu.set_rotation(3) == gpu.Status.SUCCESS
        items = b.mixed_items(np.random.default_rng(10), 20)
        out = Out(len(items), bs)
        assert host_read(gpu, b, items, 0, bs, out) == gpu.Status.SUCCESS
        check_served(b, items, 0, bs, out, "under a rotation")
    finally:
        gpu.set_rotation(0)


def test_host_form_refuses_graph_capture(gpu):
    """xec_read reads its host arguments at call time: with work it returns
    XEC_DEVICE_ERROR on a capturing stream and queues nothing."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    items = np.array([(2 << 8) | 0, 1], np.uint32)
    out = Out(2, 256)
    St = gpu.Status
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.read(b.d, b.p, S, bs, k, m, b.bm.reshape(-1), items, 2, 0, 256, out.ptr, None, 0,
                        cs) == St.DEVICE_ERROR
        assert gpu.read_tiling_used() == 0
        assert gpu.read(b.d, b.p, S, bs, k, m, b.bm.reshape(-1), items, 0, 0, 256, out.ptr, None, 0,
                        cs) == St.SUCCESS
    g.replay()  # an empty graph
    torch.cuda.synchronize()
    del g
    assert out.all_sentinel()
    b.assert_untouched("after a refused capture")


def test_graph_of_read_device_serves_the_selection_of_each_replay(gpu):
    """xec_read_device captured once and replayed three times.  Every input is
    on the device before the capture; between the replays items and bitmap are
    rewritten by device-to-device copies only (the constraint recorded at
    xec_verify).  Each replay serves what they hold then."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    b = Batch.get(S, k, m, bs)
    n, offset, length = 40, 1008, 2064
    rng = np.random.default_rng(41)
    sel = [b.mixed_items(rng, n) for _ in range(2)]
    # a third selection under a bitmap of no losses: the garbage is what the blocks hold
    held = np.concatenate([b.keep[0].cpu().numpy().reshape(S, k, bs),
                           b.keep[1].cpu().numpy().reshape(S, m, bs)], axis=1)
    d_sel = [torch.from_numpy(x.view(np.int32)).to("cuda") for x in sel + [sel[0]]]
    d_bms = [b.d_bm.clone(), b.d_bm.clone(), torch.ones_like(b.d_bm)]
    wants = [b.want(sel[0], offset, length), b.want(sel[1], offset, length),
             held[sel[0] >> 8, sel[0] & 0xFF, offset:offset + length]]
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[0], wants[2])
    d_wants = [torch.from_numpy(np.ascontiguousarray(w)).to("cuda") for w in wants]
    d_items, d_bm = d_sel[0].clone(), d_bms[0].clone()
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    out = Out(n, length)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.read_device(b.d, b.p, S, bs, k, m, d_bm, d_items, n, offset, length, out.ptr,
                               status, cs) == gpu.Status.SUCCESS
        assert gpu.read_tiling_used() == LIST
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
    b.assert_untouched("after the replays")


def test_past_4_gib(gpu):
    """16+1 x 1 MiB x 257 stripes: stripe 256 starts past 4 GiB of data.  One
    lost and one present block of it; the expectation comes from that stripe's
    blocks alone."""
    torch = _torch()
    S, k, m, bs = 257, 16, 1, 1 << 20
    s = torch.cuda.current_stream()
    d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
    p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
    assert gpu.fill_splitmix64(d, S, k * bs, 4242, s) == 0
    assert gpu.encode(d, p, S, bs, k, m, s) == 0
    torch.cuda.synchronize()
    last = d.view(S, k, bs)[256].cpu().numpy()
    par = np.bitwise_xor.reduce(last, axis=0)
    assert np.array_equal(p.view(S, bs)[256].cpu().numpy(), par)
    bm = np.ones((S, k + m), np.uint8)
    bm[256, 5] = 0
    bm[0, 5] = bm[0, 6] = 0  # and an unrecoverable stripe nobody asks for
    d.view(S, k, bs)[256, 5] = GARBAGE
    items = np.array([(256 << 8) | 5, (256 << 8) | k, (256 << 8) | 15, (256 << 8) | 5], np.uint32)
    want_blocks = np.stack([last[5], par, last[15], last[5]])
    d_bm = torch.from_numpy(bm.reshape(-1)).to("cuda")
    for offset, length in [(0, bs), (bs - 4096 - 16, 4096)]:
        want = want_blocks[:, offset:offset + length]
        out = Out(4, length)
        assert gpu.read(d, p, S, bs, k, m, bm.reshape(-1), items, 4, offset, length, out.ptr, None,
                        0, s) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert np.array_equal(out.body(), want) and out.guards_intact()
        out_d = Out(4, length)
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        d_items = torch.from_numpy(items.view(np.int32)).to("cuda")
        assert gpu.read_device(d, p, S, bs, k, m, d_bm, d_items, 4, offset, length, out_d.ptr,
                               status, s) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        assert np.array_equal(out_d.body(), want) and out_d.guards_intact()
    assert bool((d.view(S, k, bs)[256, 5] == GARBAGE).all())  # the lost block was not written
    del d, p
    torch.cuda.empty_cache()


def test_kernel_events_cover_both_calls(gpu):
    """An armed pair is consumed by each new call -- also one that launches
    nothing -- and times the read kernel: a positive interval."""
    torch = _torch()
    S, k, m, bs = 5, 32, 4, 65536
    b = Batch.get(S, k, m, bs)
    s = b.stream
    items = b.mixed_items(np.random.default_rng(7), 64)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    enc_p = torch.empty_like(b.p)  # an unarmed codec call between: encode into a spare buffer
    for entry in ("host", "device"):
        for e in ev:
            e.record(s)  # torch creates the HIP handle at the first record
        torch.cuda.synchronize()
        base = ev[0].elapsed_time(ev[1])
        assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
        out = Out(64, bs)
        # an empty list launches nothing, but consumes the setting
        assert host_read(gpu, b, items[:0], 0, bs, out) == gpu.Status.SUCCESS
        assert gpu.encode(b.d, enc_p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed
        torch.cuda.synchronize()
        assert ev[0].elapsed_time(ev[1]) == base
        assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
        if entry == "host":
            assert host_read(gpu, b, items, 0, bs, out) == gpu.Status.SUCCESS
        else:
            assert device_read(gpu, b, items, 0, bs, out) == (gpu.Status.SUCCESS, 0)
        t_kernel = ev[0].elapsed_time(ev[1])
        assert t_kernel > 0 and t_kernel != base, entry
        check_served(b, items, 0, bs, out, f"timed {entry} read")
        assert gpu.encode(b.d, enc_p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed any more
        torch.cuda.synchronize()
        assert ev[0].elapsed_time(ev[1]) == t_kernel
