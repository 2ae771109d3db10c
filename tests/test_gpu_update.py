"""In-place block update on an MI355X: xec_update (host list, work-list tiles)
and xec_update_device (device mask, class tiles) against the CPU oracle.

Expectation of every case: the same blocks are replaced in the oracle's data
with numpy and the result is encoded with oracle.encode_batch; data and parity
on the device must match both bit-exactly -- which also says that blocks not
named and classes without an item are byte-identical afterwards.  Whatever of
d_new the call must not read (the blocks past the list's end in the host form,
the unmarked blocks of the shadow in the device form) is 0xA5.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_repair import Case, set_shape

pytestmark = pytest.mark.gpu

KM = [(4, 1), (8, 4), (12, 3), (6, 6), (10, 2), (32, 1), (66, 2)]
BS = [256, 1280, 4352]  # a quarter of a one-wave tile; one tile and a ragged one; 4 and a ragged
SS = [1, 3, 23]
ENTRIES = ["host", "device"]
LAUNCHES = [dict(block_threads=256), dict(unroll=2), dict(cache_policy=2), dict(max_grid=2),
            dict(rotation=3)]
SETS = ["one", "class", "stripe", "third", "interleaved", "same", "empty"]


def _torch():
    import torch
    return torch


def items_of(blocks):
    return np.array([(c << 8) | i for c, i in blocks], dtype=np.uint32)


def expected(oracle, c: Case, ref_d, blocks, fresh):
    """(data, parity) after `blocks` of ref_d took the rows of `fresh`."""
    S, k, m, bs = c.S, c.k, c.m, c.bs
    d = oracle.aligned(S * k * bs)
    d[:] = ref_d
    v = d.reshape(S, k, bs)
    for t, (cs, i) in enumerate(blocks):
        v[cs, i] = fresh[t]
    p = oracle.aligned(S * m * bs)
    assert oracle.encode_batch(d, p, S, bs, k, m) == 0
    return d, p


def run_update(xec, c: Case, blocks, fresh, entry, scratch=None, scratch_bytes=None, stream=None):
    """Apply `blocks` (sorted (stripe, i)) <- rows of `fresh` on c's buffers."""
    torch = _torch()
    S, k, m, bs = c.S, c.k, c.m, c.bs
    n = len(blocks)
    s = c.b.stream if stream is None else stream
    if entry == "host":
        new = torch.full(((n + 2) * bs,), 0xA5, dtype=torch.uint8, device="cuda")
        if n:
            new[: n * bs] = torch.from_numpy(np.ascontiguousarray(fresh).reshape(-1)).to("cuda")
        if scratch_bytes is None:
            scratch_bytes = xec.update_scratch_bytes(n)
            scratch = torch.empty(max(scratch_bytes, 4), dtype=torch.uint8, device="cuda")
        st = xec.update(c.d, c.p, new, S, bs, k, m, items_of(blocks), n, scratch, scratch_bytes, s)
    else:
        h_shadow = np.full((S, k, bs), 0xA5, np.uint8)
        mask = np.zeros((S, k), np.uint8)
        for t, (cs, i) in enumerate(blocks):
            h_shadow[cs, i] = fresh[t]
            mask[cs, i] = (1, 2, 255)[t % 3]  # any nonzero byte marks the block
        shadow = torch.from_numpy(h_shadow.reshape(-1)).to("cuda")
        st = xec.update_device(c.d, c.p, shadow, S, bs, k, m,
                               torch.from_numpy(mask.reshape(-1)).to("cuda"), s)
    torch.cuda.synchronize()
    return st


def assert_state(c: Case, exp_d, exp_p, what):
    torch = _torch()
    torch.cuda.synchronize()
    assert np.array_equal(c.d.cpu().numpy(), exp_d), f"data != oracle {what}"
    assert np.array_equal(c.p.cpu().numpy(), exp_p), f"parity != oracle {what}"


def update_set(rng, S, k, m, kind):
    """Sorted (stripe, block) pairs of one update set."""
    nm = k // m
    cs = S // 2
    if kind == "one":
        out = [(cs, int(rng.integers(k)))]
    elif kind == "class":  # every member of one class
        j = int(rng.integers(m))
        out = [(cs, j + r * m) for r in range(nm)]
    elif kind == "stripe":  # every block of one stripe
        out = [(S - 1, i) for i in range(k)]
    elif kind == "third":
        pick = np.flatnonzero(rng.random(S * k) < 1 / 3)
        if pick.size == 0:
            pick = np.array([S * k - 1])
        out = [divmod(int(q), k) for q in pick]
    elif kind == "interleaved":
        # members 0 and nm-1 of class 0 with the blocks of other classes that lie
        # between them in the list (m == 1 or one member: what the shape allows),
        # and an item of a neighbouring stripe on either side
        last = (nm - 1) * m
        out = [(cs, i) for i in range(last + 1) if i % m == 0 and i in (0, last) or
               (i % m != 0 and i < 2 * m + 1)]
        if nm > 2:
            out.append((cs, m))  # a third member of class 0
        if cs > 0:
            out.append((cs - 1, k - 1))
        if cs + 1 < S:
            out.append((cs + 1, 0))
    elif kind == "same":
        out = [(c, int(rng.integers(k))) for c in range(S)]
    else:
        out = []
    return sorted(set(out))


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_update_sets_bit_exact(gpu, oracle, k, m, bs):
    rng = np.random.default_rng(k * 1000 + m * 10 + bs)
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
        for kind in SETS:
            blocks = update_set(rng, S, k, m, kind)
            if kind == "interleaved" and k // m >= 2:
                cls0 = [i for cs, i in blocks if cs == S // 2 and i % m == 0]
                assert len(cls0) >= 2
                if m > 1:  # items of other classes lie between two members of class 0
                    mid = [i for cs, i in blocks if cs == S // 2 and cls0[0] < i < cls0[-1]
                           and i % m != 0]
                    assert mid
            if kind == "same":
                fresh = np.stack([ref_d.reshape(S, k, bs)[cs, i] for cs, i in blocks])
            else:
                fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
            exp_d, exp_p = expected(oracle, c, ref_d, blocks, fresh)
            if kind in ("same", "empty"):
                assert np.array_equal(exp_p, ref_p) and np.array_equal(exp_d, ref_d)
            for entry in ENTRIES:
                try:
                    st = run_update(gpu, c, blocks, fresh, entry)
                    assert st == gpu.Status.SUCCESS, (kind, entry, S)
                    assert_state(c, exp_d, exp_p, f"after {entry} update '{kind}' at S={S}")
                    used = gpu.update_tiling_used()
                    if entry == "device":
                        assert used == 2
                    else:  # at most 23 * 66 / 3 + ... items: in the kernel arguments, or none
                        assert used == (0 if kind == "empty" else 4 if len(blocks) <= 1024 else 3)
                finally:
                    c.restore()
    # no stripes at all: no device call either way
    c = Case.get(gpu, oracle, 1, k, m, bs)
    assert gpu.update_device(c.d, c.p, c.d, 0, bs, k, m, None, c.b.stream) == gpu.Status.SUCCESS
    assert gpu.update_tiling_used() == 0
    assert gpu.update(c.d, c.p, c.d, 0, bs, k, m, items_of([(0, 0)]), 1, None, 0,
                      c.b.stream) == gpu.Status.SUCCESS
    assert gpu.update_tiling_used() == 0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", LAUNCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_launch_shapes_identical(gpu, oracle, shape, entry):
    """block_threads 256, unroll 2, the default cache policy, a grid of 2
    workgroups striding over the tiles, and rotation 3: the same bytes."""
    S, k, m, bs = 23, 12, 3, 4352  # 5 one-wave chunks per block, the last ragged
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d = c.ref_d.cpu().numpy()
    rng = np.random.default_rng(41)
    blocks = update_set(rng, S, k, m, "third")
    fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
    exp_d, exp_p = expected(oracle, c, ref_d, blocks, fresh)
    try:
        set_shape(gpu, **shape)
        assert run_update(gpu, c, blocks, fresh, entry) == gpu.Status.SUCCESS
        assert_state(c, exp_d, exp_p, f"{shape} {entry}")
    finally:
        set_shape(gpu)
        c.restore()


@pytest.mark.parametrize("n", [64, 65, 256, 257, 1024, 1025])
def test_list_capacities_host_form(gpu, oracle, n):
    """Up to 1,024 items travel in the kernel arguments (capacities 64 / 256 /
    1024); 1,025 go through the scratch, which must be there and large enough."""
    torch = _torch()
    S, k, m, bs = 130, 8, 4, 256
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d = c.ref_d.cpu().numpy()
    rng = np.random.default_rng(n)
    blocks = [divmod(int(q), k) for q in np.sort(rng.permutation(S * k)[:n])]
    fresh = rng.integers(0, 256, size=(n, bs), dtype=np.uint8)
    exp_d, exp_p = expected(oracle, c, ref_d, blocks, fresh)
    try:
        if n > 1024:
            St = gpu.Status
            short = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
            assert run_update(gpu, c, blocks, fresh, "host", None, 0) == St.INVALID_SIZE
            assert run_update(gpu, c, blocks, fresh, "host", short, 4 * n - 1) == St.INVALID_SIZE
            assert run_update(gpu, c, blocks, fresh, "host", short.data_ptr() + 2,
                              4 * n) == St.INVALID_ALIGNMENT
            assert gpu.update_tiling_used() == 0
            c.assert_exact("after rejected scratch arguments")
        assert run_update(gpu, c, blocks, fresh, "host") == gpu.Status.SUCCESS
        assert gpu.update_tiling_used() == (4 if n <= 1024 else 3)
        assert_state(c, exp_d, exp_p, f"after a list of {n}")
        assert gpu.decode_tiling_used() in range(7)  # its neighbours still answer
        assert gpu.repair_tiling_used() in range(5)
    finally:
        c.restore()


def run_whole_range(xec, c: Case, blocks, fresh, entry):
    """run_update's call through the ranged entry points: [0, bs), no digests."""
    torch = _torch()
    S, k, m, bs = c.S, c.k, c.m, c.bs
    n = len(blocks)
    if entry == "host":
        new = torch.full(((n + 2) * bs,), 0xA5, dtype=torch.uint8, device="cuda")
        new[: n * bs] = torch.from_numpy(np.ascontiguousarray(fresh).reshape(-1)).to("cuda")
        scratch = torch.empty(max(xec.update_scratch_bytes(n), 4), dtype=torch.uint8, device="cuda")
        st = xec.update_range(c.d, c.p, new, S, bs, k, m, items_of(blocks), n, 0, bs, None,
                              scratch, scratch.numel(), c.b.stream)
    else:
        h_shadow = np.full((S, k, bs), 0xA5, np.uint8)
        mask = np.zeros((S, k), np.uint8)
        for t, (cs, i) in enumerate(blocks):
            h_shadow[cs, i] = fresh[t]
            mask[cs, i] = (1, 2, 255)[t % 3]
        st = xec.update_range_device(c.d, c.p, torch.from_numpy(h_shadow.reshape(-1)).to("cuda"),
                                     S, bs, k, m, torch.from_numpy(mask.reshape(-1)).to("cuda"),
                                     0, bs, None, c.b.stream)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("bs", [256, 1280])
@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_whole_block_update_is_the_ranged_update(gpu, oracle, k, m, bs):
    """xec_update against xec_update_range(offset=0, len=bs, d_digests=NULL) and
    xec_update_device against xec_update_range_device, on identical inputs:
    byte-identical data and parity, both equal to the oracle's re-encode, and
    the same tiling reported.

    Shapes: the ABI takes block sizes that are multiples of 256 only, so the
    smallest block (256: a quarter of the default one-wave tile, 48 of its 64
    lanes idle) stands for "one granule", and 1280 (one full default tile and a
    ragged second one of 256 bytes) for "a tile plus 16 bytes"; 16 and 1040
    themselves must be refused alike by all four calls.  Lists at S = 3: two
    items of one class in one stripe (the owner folds the later one) with an
    item of another stripe, and an item in the last stripe only; at S = 520 a
    list of 1,030 items, which is uploaded (tiling 3) where the others travel in
    the kernel arguments (tiling 4)."""
    torch = _torch()
    St = gpu.Status
    rng = np.random.default_rng(100 * k + bs)
    long_S = 520
    every = [(cs, i) for cs in range(long_S) for i in range(k)]
    long_list = sorted(every[q] for q in rng.permutation(len(every))[:1030])
    for S, blocks in [(3, [(0, k - 1), (1, 0), (1, m)]), (3, [(2, 1)]), (long_S, long_list)]:
        c = Case.get(gpu, oracle, S, k, m, bs)
        fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
        exp_d, exp_p = expected(oracle, c, c.ref_d.cpu().numpy(), blocks, fresh)
        try:
            for entry in ENTRIES:
                tiling = 2 if entry == "device" else 4 if len(blocks) <= 1024 else 3
                assert run_update(gpu, c, blocks, fresh, entry) == St.SUCCESS
                assert gpu.update_tiling_used() == tiling
                assert_state(c, exp_d, exp_p, f"after {entry} update of {len(blocks)} at S={S}")
                d_whole, p_whole = c.d.clone(), c.p.clone()
                c.restore()
                assert run_whole_range(gpu, c, blocks, fresh, entry) == St.SUCCESS
                assert gpu.update_tiling_used() == tiling
                assert torch.equal(c.d, d_whole) and torch.equal(c.p, p_whole), (entry, S)
                assert_state(c, exp_d, exp_p, f"after {entry} ranged update over [0, bs) at S={S}")
                c.restore()
        finally:
            c.restore()
    # block sizes below the ABI's granularity: every form refuses them, nothing changes
    c = Case.get(gpu, oracle, 3, k, m, bs)
    items, s = items_of([(2, 1)]), c.b.stream
    for bad in (16, 1040):
        assert gpu.update(c.d, c.p, c.ref_d, 3, bad, k, m, items, 1, None, 0, s) == St.INVALID_SIZE
        assert gpu.update_range(c.d, c.p, c.ref_d, 3, bad, k, m, items, 1, 0, bad, None, None, 0,
                                s) == St.INVALID_SIZE
        assert gpu.update_device(c.d, c.p, c.ref_d, 3, bad, k, m, c.ref_d, s) == St.INVALID_SIZE
        assert gpu.update_range_device(c.d, c.p, c.ref_d, 3, bad, k, m, c.ref_d, 0, bad, None,
                                       s) == St.INVALID_SIZE
    c.assert_exact("after refused block sizes")


@pytest.mark.parametrize("entry", ENTRIES)
def test_update_keeps_the_syndrome(gpu, oracle, entry):
    """A class that was corrupt before the update is still flagged after it (a
    re-encode would bless the damage); the other updated class scrubs clean."""
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(17)
    blocks = [(1, 2), (1, 3)]  # classes 2 and 3 of stripe 1
    fresh = rng.integers(0, 256, size=(2, bs), dtype=np.uint8)
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    try:
        c.p.view(S, m, bs)[1, 2, 1031] ^= 0x10  # one parity byte of class 2
        assert run_update(gpu, c, blocks, fresh, entry) == gpu.Status.SUCCESS
        assert gpu.verify(c.d, c.p, S, bs, k, m, flags, count, c.b.stream) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert int(count.item()) == 1
        assert torch.nonzero(flags).flatten().tolist() == [1 * m + 2]
        assert torch.equal(c.d.view(S, k, bs)[1, 2].cpu(), torch.from_numpy(fresh[0]))
    finally:
        c.restore()


def test_rejected_calls_change_nothing(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    St, s = gpu.Status, c.b.stream
    new = torch.full((4 * bs + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    shadow = torch.full((S * k * bs + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    mask = torch.ones(S * k, dtype=torch.uint8, device="cuda")

    def host(items, d_new=new, kk=k, SS_=S):
        it = np.array(items, dtype=np.uint32)
        st = gpu.update(c.d, c.p, d_new, SS_, bs, kk, m, it, len(it), None, 0, s)
        assert gpu.update_tiling_used() == 0
        return st

    def dev(d_new=shadow, d_mask=mask, kk=k):
        st = gpu.update_device(c.d, c.p, d_new, S, bs, kk, m, d_mask, s)
        assert gpu.update_tiling_used() == 0
        return st

    ok = [(0 << 8) | 1, (1 << 8) | 0, (1 << 8) | 5]
    try:
        assert host([ok[1], ok[0], ok[2]]) == St.INVALID_COUNTS          # unsorted
        assert host([ok[0], ok[1], ok[1]]) == St.INVALID_COUNTS          # duplicate
        assert host([ok[0], (1 << 8) | k]) == St.INVALID_COUNTS          # i >= k
        assert host([ok[0], (S << 8) | 0]) == St.INVALID_COUNTS          # c >= S
        assert host(ok, kk=264) == St.INVALID_SIZE                       # beyond the item packing
        assert host(ok, SS_=(1 << 24) + 1) == St.INVALID_SIZE
        assert host(ok, d_new=new.data_ptr() + 32) == St.INVALID_ALIGNMENT
        assert dev(d_new=shadow.data_ptr() + 16) == St.INVALID_ALIGNMENT
        assert host(ok, d_new=c.d.data_ptr() + 4 * bs) == St.INVALID_SIZE   # on the data
        assert host(ok, d_new=c.p.data_ptr() + bs - 64) == St.INVALID_SIZE  # on the parity
        # a new buffer that ends inside the data range
        assert host(ok, d_new=c.d.data_ptr() - 2 * bs) == St.INVALID_SIZE
        assert dev(d_new=c.d) == St.INVALID_SIZE
        assert dev(d_new=c.p.data_ptr() - (S * k - 1) * bs) == St.INVALID_SIZE
        assert dev(d_mask=None) == St.INVALID_SIZE                       # NULL mask
        assert host(ok, d_new=None) == St.INVALID_SIZE
        # xec_check_args first
        assert gpu.update(c.d.data_ptr() + 16, c.p, new, S, bs, k, m, np.array(ok, np.uint32), 3,
                          None, 0, s) == St.INVALID_ALIGNMENT
        assert gpu.update(c.d, c.p, new, S, 100, k, m, np.array(ok, np.uint32), 3, None, 0,
                          s) == St.INVALID_SIZE
        assert gpu.update_device(c.d, c.p, shadow, S, bs, 6, 4, mask, s) == St.INVALID_COUNTS
        torch.cuda.synchronize()
        c.assert_exact("after rejected calls")
        # the same list, accepted: the call works from this state
        assert host(ok[:0]) == St.SUCCESS  # empty: nothing launched
        c.assert_exact("after an empty list")
    finally:
        c.restore()


def test_host_form_refuses_graph_capture(gpu, oracle):
    """xec_update reads h_items at call time: with work it returns
    XEC_DEVICE_ERROR on a capturing stream and queues nothing; the capture
    stays valid and the graph is empty."""
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    new = torch.full((2 * bs,), 0x3C, dtype=torch.uint8, device="cuda")
    items = items_of([(0, 1), (2, 7)])
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.update(c.d, c.p, new, S, bs, k, m, items, 2, None, 0, cs) == St.DEVICE_ERROR
            assert gpu.update_tiling_used() == 0
            assert gpu.update(c.d, c.p, new, S, bs, k, m, items, 0, None, 0, cs) == St.SUCCESS
        g.replay()  # an empty graph
        torch.cuda.synchronize()
        del g
        c.assert_exact("after a refused capture")
    finally:
        c.restore()


def test_graph_of_update_device_and_verify(gpu, oracle):
    """One linear chain on one stream -- update_device, verify -- captured once
    and replayed twice, as test_gpu_repair's captured chain is: both masks,
    both shadows and both expected states are on the device before the capture,
    and between the replays the mask and the shadow are only rewritten by
    device-to-device copies from outside the graph.  Each replay applies what
    they hold then: data and parity match the oracle, and the captured
    xec_verify counts no class and sets no flag."""
    torch = _torch()
    S, k, m, bs = 23, 12, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(23)
    state = c.ref_d.cpu().numpy()
    masks, shadows, want = [], [], []
    for kind in ("third", "interleaved"):
        blocks = update_set(rng, S, k, m, kind)
        fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
        state, exp_p = expected(oracle, c, state, blocks, fresh)
        h_mask = np.zeros((S, k), np.uint8)
        h_shadow = np.full((S, k, bs), 0xA5, np.uint8)
        for t, (cs_, i) in enumerate(blocks):
            h_mask[cs_, i] = (1, 2, 255)[t % 3]
            h_shadow[cs_, i] = fresh[t]
        masks.append(torch.from_numpy(h_mask.reshape(-1)).to("cuda"))
        shadows.append(torch.from_numpy(h_shadow.reshape(-1)).to("cuda"))
        want.append((torch.from_numpy(state.copy()).to("cuda"), torch.from_numpy(exp_p).to("cuda")))
    assert not torch.equal(masks[0], masks[1])
    mask, shadow = masks[0].clone(), shadows[0].clone()
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.update_device(c.d, c.p, shadow, S, bs, k, m, mask, cs) == St.SUCCESS
            assert gpu.update_tiling_used() == 2
            assert gpu.verify(c.d, c.p, S, bs, k, m, flags, count, cs) == St.SUCCESS
        for r in range(2):
            mask.copy_(masks[r])
            shadow.copy_(shadows[r])
            count.fill_(77)
            flags.fill_(0xFF)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            print(f"replay {r}: captured verify count {int(count.item())}, "
                  f"flag bytes {sorted(set(flags.tolist()))}")
            assert int(count.item()) == 0
            assert int(flags.count_nonzero()) == 0
            assert torch.equal(c.d, want[r][0]), f"data != oracle after replay {r}"
            assert torch.equal(c.p, want[r][1]), f"parity != oracle after replay {r}"
        del g
    finally:
        c.restore()


def test_kernel_events_cover_both_calls(gpu, oracle):
    """An armed pair is consumed by each new call -- also one that launches
    nothing -- and times the update kernel: a positive interval."""
    torch = _torch()
    S, k, m, bs = 23, 12, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    s = c.b.stream
    rng = np.random.default_rng(29)
    blocks = update_set(rng, S, k, m, "third")
    fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    try:
        for entry in ENTRIES:
            for e in ev:
                e.record(s)  # torch creates the HIP handle at the first record
            torch.cuda.synchronize()
            base = ev[0].elapsed_time(ev[1])
            assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
            # an empty list launches nothing, but consumes the setting
            assert run_update(gpu, c, [], fresh[:0], "host") == gpu.Status.SUCCESS
            assert gpu.encode(c.d, c.p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed
            torch.cuda.synchronize()
            assert ev[0].elapsed_time(ev[1]) == base
            assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
            assert run_update(gpu, c, blocks, fresh, entry) == gpu.Status.SUCCESS
            t_kernel = ev[0].elapsed_time(ev[1])
            assert t_kernel > 0 and t_kernel != base, entry
            assert gpu.encode(c.d, c.p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed any more
            torch.cuda.synchronize()
            assert ev[0].elapsed_time(ev[1]) == t_kernel
            c.restore()
    finally:
        c.restore()
