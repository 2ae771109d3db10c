"""Full-stripe repair on an MI355X: xec_repair (host bitmap, work-list tiles)
and xec_repair_device (device bitmap, class tiles) rebuild every lost block,
data or parity, bit-exactly against the CPU oracle's data and parity.

Loss patterns are built by construction -- each class draws one of {nothing
lost, data member r, parity} -- so every pattern is recoverable; the
unrecoverable ones are built separately.  Lost blocks are filled with 0xA5
garbage before every call: what a lost block holds must not matter.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import Batch, encode_and_check

pytestmark = pytest.mark.gpu

KM = [(4, 1), (8, 4), (12, 3), (6, 6), (10, 2), (32, 1), (66, 2)]  # members 4 2 4 1 5 32 33
BS = [256, 1280, 4352]  # a quarter of a one-wave tile; one tile and a ragged one; 4 and a ragged
SS = [1, 3, 23]
ENTRIES = ["host", "device"]
LAUNCHES = [dict(block_threads=256), dict(unroll=2), dict(cache_policy=2), dict(max_grid=2),
            dict(rotation=3)]


def _torch():
    import torch
    return torch


class Case:
    """An encoded device batch with the oracle's data and parity beside it on
    the device; every test leaves it as it found it (checked), so one is shared
    per shape."""
    _cache: dict = {}

    def __init__(self, xec, oracle, S, k, m, bs):
        torch = _torch()
        self.b, ref_d, ref_p = encode_and_check(xec, oracle, S, k, m, bs)
        self.S, self.k, self.m, self.bs = S, k, m, bs
        self.ref_d = torch.from_numpy(ref_d).to("cuda")
        self.ref_p = torch.from_numpy(ref_p).to("cuda")
        self.d = self.b.d[: S * k * bs]
        self.p = self.b.p[: S * m * bs]

    @classmethod
    def get(cls, xec, oracle, S, k, m, bs):
        key = (S, k, m, bs)
        if key not in cls._cache:
            if len(cls._cache) > 8:
                cls._cache.clear()
            cls._cache[key] = cls(xec, oracle, S, k, m, bs)
        c = cls._cache[key]
        c.assert_exact("a previous test left the shared batch changed")
        return c

    def assert_exact(self, what=""):
        torch = _torch()
        torch.cuda.synchronize()
        assert torch.equal(self.d, self.ref_d), f"data != oracle {what}"
        assert torch.equal(self.p, self.ref_p), f"parity != oracle {what}"

    def garbage(self, bm, value=0xA5):
        """Fill every lost block (bitmap byte 0) with `value`."""
        torch = _torch()
        lost = torch.from_numpy(np.ascontiguousarray(bm.reshape(self.S, -1) == 0)).to("cuda")
        self.d.view(self.S, self.k, self.bs)[lost[:, : self.k]] = value
        self.p.view(self.S, self.m, self.bs)[lost[:, self.k:]] = value

    def restore(self):
        self.d.copy_(self.ref_d)
        self.p.copy_(self.ref_p)


def pattern(rng, S, k, m, kind):
    """kind: 'parity' {nothing, parity}, 'data' {nothing, data member r},
    'mixed' all three, 'none'.  One draw per class, so always recoverable; a
    kind that loses something loses at least one block (mixed: a data block in
    the first class and the parity of the last, where there are two classes)."""
    bm = np.ones((S, k + m), np.uint8)
    if kind == "none":
        return bm
    nm = k // m
    for c in range(S):
        for j in range(m):
            roll = int(rng.integers(3))
            if roll == 1 and kind in ("data", "mixed"):
                bm[c, j + m * int(rng.integers(nm))] = 0
            elif roll == 2 and kind in ("parity", "mixed"):
                bm[c, k + j] = 0
    if kind in ("data", "mixed"):
        bm[0, :k][0::m] = 1
        bm[0, k] = 1
        bm[0, m * int(rng.integers(nm))] = 0  # class 0 of stripe 0 loses a data block
    if kind == "parity" or (kind == "mixed" and S * m > 1):
        last = m - 1
        bm[S - 1, :k][last::m] = 1
        bm[S - 1, k + last] = 0  # the last class loses its parity
    return bm


def run_repair(xec, c: Case, bm, entry, scratch=None):
    """The call on c's buffers; returns (return value, verdict)."""
    torch = _torch()
    flat = np.ascontiguousarray(bm.reshape(-1))
    S, k, m, bs = c.S, c.k, c.m, c.bs
    if entry == "host":
        h_bm = torch.from_numpy(flat).pin_memory()
        if scratch is None:
            scratch = torch.empty(flat.size, dtype=torch.uint8, device="cuda")
        st = xec.repair(c.d, c.p, S, bs, k, m, h_bm, scratch, c.b.stream)
        torch.cuda.synchronize()
        return st, int(st)
    d_bm = torch.from_numpy(flat).to("cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    st = xec.repair_device(c.d, c.p, S, bs, k, m, d_bm, status, c.b.stream)
    torch.cuda.synchronize()
    return st, int(status.item())


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_repair_patterns_bit_exact(gpu, oracle, k, m, bs):
    """Parity-only, data-only and mixed losses, present bytes 2 / 3 / 255, and
    nothing lost, on both entry points, at S = 1, 3 and 23."""
    torch = _torch()
    rng = np.random.default_rng(k * 1000 + m * 10 + bs)
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        for kind in ("parity", "data", "mixed", "bytes", "none"):
            bm = pattern(rng, S, k, m, "mixed" if kind == "bytes" else kind)
            if kind == "bytes":  # present blocks marked 2, 3 or 255: still present
                present = bm != 0
                marks = rng.choice(np.array([1, 2, 3, 255], np.uint8), size=bm.shape)
                bm[present] = marks[present]
            for entry in ENTRIES:
                c.garbage(bm)
                if kind == "data" and entry == "host":
                    # xec_decode on the same input: the same bytes, parity untouched
                    d2 = c.d.clone()
                    h_bm = torch.from_numpy(np.ascontiguousarray(bm.reshape(-1))).pin_memory()
                    assert gpu.decode(d2, c.p, S, bs, k, m, h_bm,
                                      torch.empty(bm.size, dtype=torch.uint8, device="cuda"),
                                      c.b.stream) == gpu.Status.SUCCESS
                st, verdict = run_repair(gpu, c, bm, entry)
                assert st == gpu.Status.SUCCESS and verdict == 0, (kind, entry, S)
                c.assert_exact(f"after {entry} repair of {kind} at S={S}")
                if kind == "data" and entry == "host":
                    assert torch.equal(d2, c.d), "repair and decode rebuilt different bytes"
                used = gpu.repair_tiling_used()
                if entry == "device":
                    assert used == 2
                elif kind == "none":
                    assert used == 0  # nothing lost: nothing launched
                else:
                    assert used == 4  # at most 23 * 6 entries: in the kernel arguments


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("how", ["data_and_parity", "two_data"])
@pytest.mark.parametrize("k,m,bs,S", [(8, 4, 1280, 3), (12, 3, 256, 23), (32, 1, 4352, 3),
                                      (66, 2, 1280, 3), (10, 2, 4352, 1)])
def test_unrecoverable_batch_is_left_untouched(gpu, oracle, k, m, bs, S, how, entry):
    """One class of one stripe lost two blocks in an otherwise repairable
    batch: the verdict is 4 (the return value of the host form, *d_status of
    the device form) and both buffers are byte-identical to before the call."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(S * 100 + k)
    bm = pattern(rng, S, k, m, "mixed")
    cs, j = S // 2, m - 1  # the stripe and class that cannot be repaired
    bm[cs, :k][j::m] = 1
    bm[cs, j] = 0
    if how == "data_and_parity":
        bm[cs, k + j] = 0
    else:
        bm[cs, k + j] = 1
        bm[cs, j + m] = 0
    try:
        c.garbage(bm)
        before_d, before_p = c.d.clone(), c.p.clone()
        st, verdict = run_repair(gpu, c, bm, entry)
        assert verdict == 4
        assert st == (gpu.Status.DECODE_FAILURE if entry == "host" else gpu.Status.SUCCESS)
        assert torch.equal(c.d, before_d) and torch.equal(c.p, before_p)
        if entry == "host":
            assert gpu.repair_tiling_used() == 0
    finally:
        c.restore()


@pytest.mark.parametrize("k,m,bs,S", [(8, 4, 1280, 3), (32, 1, 4352, 3)])
def test_lost_parity_decode_leaves_it_repair_puts_it_back(gpu, oracle, k, m, bs, S):
    """Today's xec_decode is unchanged: a lost (erased) parity block is still
    zero after it.  After xec_repair it equals the encode."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    bm = np.ones((S, k + m), np.uint8)
    bm[:, k + m - 1] = 0  # the last parity block of every stripe
    if m > 1:
        bm[:, 0] = 0      # and a data block of class 0
    flat = np.ascontiguousarray(bm.reshape(-1))
    h_bm = torch.from_numpy(flat).pin_memory()
    d_bm = h_bm.to("cuda")
    try:
        assert gpu.erase(c.d, c.p, S, bs, k, m, d_bm, c.b.stream) == gpu.Status.SUCCESS
        assert gpu.decode(c.d, c.p, S, bs, k, m, h_bm, torch.empty_like(d_bm),
                          c.b.stream) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        lost_p = c.p.view(S, m, bs)[:, m - 1]
        assert int(lost_p.count_nonzero()) == 0, "xec_decode wrote a lost parity block"
        assert torch.equal(c.d, c.ref_d)
        st, _ = run_repair(gpu, c, bm, "host")
        assert st == gpu.Status.SUCCESS
        c.assert_exact("after repair of the parity decode left lost")
    finally:
        c.restore()


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1024, 1025, 1200])
def test_list_boundaries_host_form(gpu, oracle, n):
    """Lists of up to 1,024 entries travel in the kernel arguments (capacities
    64 / 256 / 1024); a longer one is uploaded into the scratch -- here 1,200
    entries through a scratch that holds 900, so in two pieces."""
    S, k, m, bs = 300, 8, 4, 256
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(n)
    bm = np.ones((S, k + m), np.uint8)
    for q in rng.permutation(S * m)[:n]:  # one loss in each of n classes
        cs, j = divmod(int(q), m)
        if q % 3 == 0:
            bm[cs, k + j] = 0
        else:
            bm[cs, j + m * int(rng.integers(k // m))] = 0
    c.garbage(bm)
    st, _ = run_repair(gpu, c, bm, "host")
    assert st == gpu.Status.SUCCESS
    assert gpu.repair_tiling_used() == (4 if n <= 1024 else 3)
    c.assert_exact(f"after a list of {n}")
    assert gpu.decode_tiling_used() in range(7)  # its neighbour still answers


def test_long_list_through_an_unaligned_scratch(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 300, 8, 4, 256
    c = Case.get(gpu, oracle, S, k, m, bs)
    bm = pattern(np.random.default_rng(5), S, k, m, "mixed")
    bm[:, k:] = 0  # every parity block, and the data losses of 'mixed' put back
    bm[:, :k] = 1
    bm[::2, 3] = 0
    bm[::2, k + 3] = 1
    n = int((bm == 0).sum())
    assert n > 1024
    c.garbage(bm)
    scratch = torch.empty(bm.size + 8, dtype=torch.uint8, device="cuda")
    st, _ = run_repair(gpu, c, bm, "host", scratch=scratch.data_ptr() + 1)
    assert st == gpu.Status.SUCCESS and gpu.repair_tiling_used() == 3
    c.assert_exact("after a long list through an unaligned scratch")


def test_row_width_limits(gpu, oracle):
    """k + m = 256 is accepted by the host form and exact; 257 is
    XEC_INVALID_SIZE with nothing written; the device form has no limit."""
    torch = _torch()
    c = Case.get(gpu, oracle, 3, 252, 4, 256)
    bm = pattern(np.random.default_rng(9), 3, 252, 4, "mixed")
    bm[2, 252 + 3] = 0  # item index 255
    bm[2, :252][3::4] = 1
    for entry in ENTRIES:
        c.garbage(bm)
        st, verdict = run_repair(gpu, c, bm, entry)
        assert st == gpu.Status.SUCCESS and verdict == 0
        c.assert_exact(f"252+4 {entry}")
    c = Case.get(gpu, oracle, 3, 256, 1, 256)
    bm = pattern(np.random.default_rng(10), 3, 256, 1, "mixed")
    try:
        c.garbage(bm)
        before_d, before_p = c.d.clone(), c.p.clone()
        st, _ = run_repair(gpu, c, bm, "host")
        assert st == gpu.Status.INVALID_SIZE and gpu.repair_tiling_used() == 0
        assert torch.equal(c.d, before_d) and torch.equal(c.p, before_p)
        st, verdict = run_repair(gpu, c, bm, "device")
        assert st == gpu.Status.SUCCESS and verdict == 0
        c.assert_exact("256+1 device")
    finally:
        c.restore()


def set_shape(xec, unroll=0, max_grid=0, cache_policy=0, block_threads=0, rotation=0):
    assert xec.set_launch(unroll, max_grid, cache_policy, block_threads) == xec.Status.SUCCESS
    assert xec.set_rotation(rotation) == xec.Status.SUCCESS


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", LAUNCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_launch_shapes_identical(gpu, oracle, shape, entry):
    """block_threads 256, unroll 2, the default cache policy, a grid of 2
    workgroups striding over the tiles, and rotation 3: the same bytes."""
    try:
        set_shape(gpu, **shape)
        for (k, m, bs, S) in [(12, 3, 4352, 23), (32, 1, 1280, 3), (10, 2, 4352, 3)]:
            c = Case.get(gpu, oracle, S, k, m, bs)
            bm = pattern(np.random.default_rng(S + k), S, k, m, "mixed")
            c.garbage(bm)
            st, verdict = run_repair(gpu, c, bm, entry)
            assert st == gpu.Status.SUCCESS and verdict == 0
            c.assert_exact(f"{shape} {entry} {(k, m, bs, S)}")
    finally:
        set_shape(gpu)


def test_offsets_past_4_gib(gpu):
    """16+2 x 1 MiB x 260 stripes: 4.06 GiB of data.  Parity 1 of the last
    stripe and a data block of stripe 257 are rebuilt from byte offsets past
    2^32; the scrub then finds nothing, and after one flipped byte in the last
    stripe exactly the last flag."""
    torch = _torch()
    S, k, m, bs = 260, 16, 2, 1 << 20
    free, _ = torch.cuda.mem_get_info()
    assert free > S * (k + m) * bs + (2 << 30), "needs 7 GiB of free HBM"
    b = Batch(gpu, S, k, m, bs)
    assert gpu.encode(b.d, b.p, S, bs, k, m, b.stream) == gpu.Status.SUCCESS
    d3, p3 = b.d[: S * k * bs].view(S, k, bs), b.p[: S * m * bs].view(S, m, bs)
    keep_p, keep_d = p3[S - 1, 1].clone(), d3[257, 5].clone()
    bm = np.ones((S, k + m), np.uint8)
    bm[S - 1, k + 1] = 0
    bm[257, 5] = 0
    flat = np.ascontiguousarray(bm.reshape(-1))
    h_bm = torch.from_numpy(flat).pin_memory()
    d_bm = h_bm.to("cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    for entry in ENTRIES:
        p3[S - 1, 1] = 0xA5
        d3[257, 5] = 0xA5
        if entry == "host":
            st = gpu.repair(b.d, b.p, S, bs, k, m, h_bm, torch.empty_like(d_bm), b.stream)
        else:
            st = gpu.repair_device(b.d, b.p, S, bs, k, m, d_bm, status, b.stream)
        assert st == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(p3[S - 1, 1], keep_p), entry
        assert torch.equal(d3[257, 5], keep_d), entry
    assert int(status.item()) == 0
    assert gpu.verify(b.d, b.p, S, bs, k, m, flags, count, b.stream) == gpu.Status.SUCCESS
    assert int(count.item()) == 0 and int(flags.count_nonzero()) == 0
    d3[S - 1, 13, bs - 7] ^= 0x40  # class 1 of the last stripe
    assert gpu.verify(b.d, b.p, S, bs, k, m, flags, count, b.stream) == gpu.Status.SUCCESS
    assert int(count.item()) == 1
    assert torch.nonzero(flags).flatten().tolist() == [S * m - 1]
    del b, d3, p3
    torch.cuda.empty_cache()


def test_argument_errors_queue_nothing(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    bm = pattern(np.random.default_rng(2), S, k, m, "mixed")
    flat = np.ascontiguousarray(bm.reshape(-1))
    d_bm = torch.from_numpy(flat).to("cuda")
    status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    St = gpu.Status
    try:
        c.garbage(bm)
        before_d, before_p = c.d.clone(), c.p.clone()
        s = c.b.stream
        assert gpu.repair_device(c.d, c.p, S, bs, k, m, d_bm, None, s) == St.INVALID_ALIGNMENT
        assert gpu.repair_device(c.d, c.p, S, bs, k, m, d_bm, status.data_ptr() + 2,
                                 s) == St.INVALID_ALIGNMENT
        assert gpu.repair_device(c.d, c.p, S, bs, k, m, None, status, s) == St.INVALID_SIZE
        assert gpu.repair_device(c.d.data_ptr() + 16, c.p, S, bs, k, m, d_bm, status,
                                 s) == St.INVALID_ALIGNMENT
        assert gpu.repair_device(c.d, c.p, S, 100, k, m, d_bm, status, s) == St.INVALID_SIZE
        assert gpu.repair_device(c.d, c.p, S, bs, 6, 4, d_bm, status, s) == St.INVALID_COUNTS
        assert gpu.repair(c.d, c.p.data_ptr() + 32, S, bs, k, m, flat, d_bm,
                          s) == St.INVALID_ALIGNMENT
        assert gpu.repair(c.d, c.p, S, 100, k, m, flat, d_bm, s) == St.INVALID_SIZE
        assert gpu.repair(c.d, c.p, S, bs, 6, 4, flat, d_bm, s) == St.INVALID_COUNTS
        torch.cuda.synchronize()
        assert status.tolist() == [77, 77], "a rejected call wrote d_status"
        assert torch.equal(c.d, before_d) and torch.equal(c.p, before_p)
        # S = 0: the verdict is 0 and nothing else happens
        assert gpu.repair_device(c.d, c.p, 0, bs, k, m, None, status, s) == St.SUCCESS
        assert gpu.repair(c.d, c.p, 0, bs, k, m, flat, None, s) == St.SUCCESS
        torch.cuda.synchronize()
        assert status.tolist() == [0, 77]
        assert torch.equal(c.d, before_d) and torch.equal(c.p, before_p)
    finally:
        c.restore()


def test_host_form_refuses_graph_capture(gpu, oracle):
    """xec_repair scans h_bitmap at call time, as xec_decode does: with blocks
    to rebuild it returns XEC_DEVICE_ERROR on a capturing stream and queues
    nothing; with nothing lost, or an unrecoverable batch, the verdict comes
    from the scan alone."""
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    work = pattern(np.random.default_rng(3), S, k, m, "mixed")
    bad = work.copy()
    bad[1, 0] = bad[1, k] = 0
    pins = [torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).pin_memory()
            for x in (work, np.ones_like(work), bad)]
    scratch = torch.empty(work.size, dtype=torch.uint8, device="cuda")
    St = gpu.Status
    try:
        c.garbage(work)
        before_d, before_p = c.d.clone(), c.p.clone()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.repair(c.d, c.p, S, bs, k, m, pins[0], scratch, cs) == St.DEVICE_ERROR
            assert gpu.repair(c.d, c.p, S, bs, k, m, pins[1], scratch, cs) == St.SUCCESS
            assert gpu.repair(c.d, c.p, S, bs, k, m, pins[2], scratch, cs) == St.DECODE_FAILURE
        g.replay()  # an empty graph
        torch.cuda.synchronize()
        del g
        assert torch.equal(c.d, before_d) and torch.equal(c.p, before_p)
    finally:
        c.restore()


def test_graph_of_encode_erase_repair_verify(gpu, oracle):
    """One linear chain on one stream -- encode, erase, repair_device, verify --
    captured once and replayed twice, with a different device bitmap copied in
    from outside the graph between the replays."""
    torch = _torch()
    S, k, m, bs = 23, 12, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(11)
    bms = [torch.from_numpy(np.ascontiguousarray(pattern(rng, S, k, m, "mixed").reshape(-1)))
           .to("cuda") for _ in range(2)]
    assert not torch.equal(bms[0], bms[1])
    d_bm = bms[0].clone()
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.encode(c.d, c.p, S, bs, k, m, cs) == St.SUCCESS
            assert gpu.erase(c.d, c.p, S, bs, k, m, d_bm, cs) == St.SUCCESS
            assert gpu.repair_device(c.d, c.p, S, bs, k, m, d_bm, status, cs) == St.SUCCESS
            assert gpu.verify(c.d, c.p, S, bs, k, m, flags, count, cs) == St.SUCCESS
        for bm in bms:
            d_bm.copy_(bm)
            status.fill_(77)
            count.fill_(77)
            flags.fill_(0xFF)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert int(status.item()) == 0 and int(count.item()) == 0
            assert int(flags.count_nonzero()) == 0
            c.assert_exact("after a replay")
        del g
    finally:
        c.restore()
