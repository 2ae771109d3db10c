"""The shard-major layout on an MI355X: xec_encode_shards,
xec_repair_shards_device and xec_verify_shards over one buffer per shard.

Every expectation is the PRISTINE batch of test_gpu_read.Batch (parity by
numpy), laid out by this file's own arithmetic

    data block i   of stripe c : shard[i]     + c * data_stride
    parity block j of stripe c : shard[k + j] + c * parity_stride

in three placements of the same bytes:

  A  the shards aliased into a batch (data_stride = k*bs, parity_stride = m*bs),
     where the bytes must also equal the batch call's;
  B  one arena, the shards in shuffled address order, data_stride = bs + 64 and
     parity_stride = 2*bs, 64 sentinel bytes between neighbours and at both ends;
  C  data shards 0 and 1 interleaved in one allocation (data_stride = 2*bs), every
     other shard in an allocation of its own between two guards.

Whatever is not a block -- guards, the gaps a stride leaves between blocks, the
gaps between shards -- holds SENTINEL, lost blocks hold GARBAGE before a call,
and after every call each allocation is compared as a whole with the image this
file expects: blocks, gaps and guards at once.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_read import BSS, GARBAGE, GUARD, KMS, SENTINEL, Batch

pytestmark = pytest.mark.gpu

PLACEMENTS = ["A", "B", "C"]
POISON = 77
# (block_threads, unroll) x cache policy x (max_grid, rotation): the launch shapes
# tests/test_gpu_ops_matrix.py walks; max_grid 2 strides two workgroups over every tile
SHAPES = [(64, 1), (64, 2), (256, 1), (256, 2)]
POLICIES = [1, 2]
GRID_ROT = [(0, -1), (2, 3), (2, -1), (0, 3)]


def _torch():
    import torch
    return torch


class Layout:
    """Where the k + m shards of one placement live: sizes of the allocations,
    (allocation, byte offset) of each shard, and the two strides."""

    def __init__(self, S, k, m, bs, placement):
        self.S, self.k, self.m, self.bs, self.placement = S, k, m, bs, placement
        self.images = {}
        G = GUARD
        if placement == "A":
            self.ds, self.ps = k * bs, m * bs
            par = G + S * k * bs + G
            self.sizes = [par + S * m * bs + G]
            self.loc = [(0, G + i * bs) for i in range(k)] + [(0, par + j * bs) for j in range(m)]
            self.batch_offsets = (G, par)
        elif placement == "B":
            self.ds, self.ps = bs + 64, 2 * bs
            order = np.random.default_rng(S * 131 + k * 17 + m + bs).permutation(k + m)
            self.loc = [None] * (k + m)
            pos = G
            for x in order:
                self.loc[int(x)] = (0, pos)
                pos += self.hull(int(x)) + 64
            self.sizes = [pos]  # the last gap is the end guard
        else:
            self.ds, self.ps = 2 * bs, bs
            self.sizes = [G + 2 * S * bs + G]
            self.loc = [(0, G), (0, G + bs)]
            for x in range(2, k + m):
                self.loc.append((len(self.sizes), G))
                self.sizes.append(G + self.hull(x) + G)
        assert len(self.loc) == k + m and all(o % 64 == 0 for _, o in self.loc)

    def stride(self, x):
        return self.ds if x < self.k else self.ps

    def hull(self, x):
        return (self.S - 1) * self.stride(x) + self.bs

    def at(self, x, c):
        r, o = self.loc[x]
        return r, o + c * self.stride(x)

    def image(self, blocks, bm=None):
        """The allocations as numpy arrays: SENTINEL everywhere, block (c, x) of
        `blocks` (S, k+m, bs) at its place, GARBAGE instead where bm[c, x] == 0.
        Built once per (blocks, bm) and shared: a caller that edits one copies it."""
        key = (id(blocks), None if bm is None else bm.tobytes())
        if key in self.images:
            return self.images[key]
        img = self.images[key] = [np.full(n, SENTINEL, np.uint8) for n in self.sizes]
        for x in range(self.k + self.m):
            for c in range(self.S):
                r, o = self.at(x, c)
                img[r][o:o + self.bs] = GARBAGE if bm is not None and bm[c, x] == 0 else blocks[c, x]
        return img

    def block_mask(self, bm):
        """Boolean images: True on the bytes of the blocks with bm[c, x] == 0."""
        mask = [np.zeros(n, bool) for n in self.sizes]
        for c, x in np.argwhere(bm == 0):
            r, o = self.at(int(x), int(c))
            mask[r][o:o + self.bs] = True
        return mask


class Store:
    """A layout's allocations on the device and its pointer table."""

    def __init__(self, lay: Layout, img):
        torch = _torch()
        self.lay = lay
        self.t = [torch.from_numpy(a).to("cuda") for a in img]
        assert all(t.data_ptr() % 64 == 0 for t in self.t)
        self.ptrs = [self.t[r].data_ptr() + o for r, o in lay.loc]
        self.args = (self.ptrs, lay.ds, lay.ps, lay.S, lay.bs, lay.k, lay.m)

    def load(self, img):
        torch = _torch()
        for t, a in zip(self.t, img):
            t.copy_(torch.from_numpy(a))

    def assert_image(self, want, what):
        lay = self.lay
        for r, (t, w) in enumerate(zip(self.t, want)):
            got = t.cpu().numpy()
            if np.array_equal(got, w):
                continue
            at = int(np.flatnonzero(got != w)[0])
            where = "a guard or a gap"
            for x in range(lay.k + lay.m):
                for c in range(lay.S):
                    rr, o = lay.at(x, c)
                    if rr == r and o <= at < o + lay.bs:
                        where = f"block {x} of stripe {c}, byte {at - o}"
            raise AssertionError(f"{what}: allocation {r} differs at byte {at} ({where}): "
                                 f"{got[at]:#x} for {w[at]:#x}")


def pristine(S, k, m, bs):
    return Batch.get(S, k, m, bs, "pristine").blocks


def describe(k, m, bs, S, placement):
    return f"{k}+{m} x {bs} x {S} placement {placement}"


def loss_bitmap(kind, S, k, m, rng):
    bm = rng.choice(np.array([1, 2, 255], np.uint8), size=(S, k + m))
    nm = k // m
    if kind == "data":  # one data block of every class of every stripe
        for c in range(S):
            for j in range(m):
                bm[c, j + m * int(rng.integers(nm))] = 0
    elif kind == "parity":
        bm[:, k:][rng.random((S, m)) < 0.6] = 0
        bm[0, k] = 0
    elif kind == "mixed":  # data or parity or nothing per class; every third stripe intact
        for c in range(S):
            if c % 3 == 1:
                continue
            for j in range(m):
                r = int(rng.integers(nm + 2))
                if r <= nm:
                    bm[c, k + j if r == nm else j + m * r] = 0
        bm[0, 0], bm[0, m:k:m] = 0, 1  # a data loss for certain, alone in its class
        bm[0, k] = 1
    else:
        assert kind == "none"
    return bm


def device_bitmap(bm):
    return _torch().from_numpy(np.ascontiguousarray(bm.reshape(-1))).to("cuda")


def poison():
    return _torch().full((1,), POISON, dtype=_torch().int32, device="cuda")


# -- the three cases, reused under every launch shape -------------------------
def run_encode(gpu, st: Store, blocks, what, stream=None):
    lay = st.lay
    parity_lost = np.ones((lay.S, lay.k + lay.m), np.uint8)
    parity_lost[:, lay.k:] = 0
    st.load(lay.image(blocks, parity_lost))
    assert gpu.encode_shards(*st.args, stream) == gpu.Status.SUCCESS, what
    assert gpu.shards_arg_capacity_used() == (64 if lay.k + lay.m <= 64 else 256), what
    _torch().cuda.synchronize()
    st.assert_image(lay.image(blocks), "encode, " + what)


def run_repair(gpu, st: Store, blocks, bm, what, want_status=0, stream=None):
    lay = st.lay
    before = lay.image(blocks, bm)
    st.load(before)
    d_bm, status = device_bitmap(bm), poison()
    assert gpu.repair_shards_device(*st.args, d_bm, status, stream) == gpu.Status.SUCCESS, what
    _torch().cuda.synchronize()
    assert int(status.item()) == want_status, what
    # a refused batch keeps every byte, garbage included
    st.assert_image(lay.image(blocks) if want_status == 0 else before, "repair, " + what)
    assert np.array_equal(d_bm.cpu().numpy(), bm.reshape(-1)), f"bitmap written, {what}"


def scrub(gpu, st: Store, stream=None):
    torch = _torch()
    lay = st.lay
    flags = torch.full((lay.S * lay.m,), 0xFF, dtype=torch.uint8, device="cuda")
    count = poison()
    assert gpu.verify_shards(*st.args, flags, count, stream) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    return np.flatnonzero(flags.cpu().numpy()).tolist(), int(count.item()), flags.cpu().numpy()


def run_verify(gpu, st: Store, blocks, what):
    """Clean: no flag.  One bit in the last 16 bytes of a data block (the ragged
    tile where bs has one) and one in a parity block of another stripe: exactly
    those two classes.  The store is put back afterwards."""
    lay = st.lay
    S, k, m, bs = lay.S, lay.k, lay.m, lay.bs
    clean = lay.image(blocks)
    st.load(clean)
    got = scrub(gpu, st)
    assert got[:2] == ([], 0) and set(got[2].tolist()) == {0}, f"clean store flagged, {what}"
    flips = [(0, k - 1, bs - 5, 0x10), (S - 1, k + m - 1, bs // 2, 0x01)]
    want = sorted({c * m + (x % m if x < k else x - k) for c, x, _, _ in flips})
    assert len(want) == 2
    bad = [a.copy() for a in clean]
    for c, x, byte, bit in flips:
        r, o = lay.at(x, c)
        bad[r][o + byte] ^= bit
    st.load(bad)
    got = scrub(gpu, st)
    assert got[:2] == (want, 2) and set(got[2].tolist()) == {0, 1}, (what, got[:2], want)
    st.assert_image(bad, "the scrub wrote a shard, " + what)
    st.load(clean)


# -- 1. encode ----------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_encode_is_numpys_parity(gpu, k, m, bs, placement):
    torch = _torch()
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, lay.image(blocks))
    what = describe(k, m, bs, S, placement)
    run_encode(gpu, st, blocks, what)
    if placement == "A":  # the batch call on the same data, into a second parity buffer
        d_off, p_off = lay.batch_offsets
        second = torch.full((S * m * bs,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert gpu.encode(st.t[0].data_ptr() + d_off, second, S, bs, k, m) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(second, st.t[0][p_off:p_off + S * m * bs]), what


# -- 2. repair ----------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_repair_restores_the_pristine_bytes(gpu, k, m, bs, placement):
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, lay.image(blocks))
    rng = np.random.default_rng(k * 7 + m + bs)
    for kind in ("data", "parity", "mixed", "none"):
        bm = loss_bitmap(kind, S, k, m, rng)
        assert (kind == "none") == bool((bm != 0).all())
        if kind == "parity":
            assert (bm[:, :k] != 0).all()
        if kind == "mixed":
            assert (bm[1] != 0).all() or S < 2
        run_repair(gpu, st, blocks, bm, f"{kind} losses, " + describe(k, m, bs, S, placement))
        assert gpu.shards_arg_capacity_used() == (64 if k + m <= 64 else 256)
    # a class with two losses, among recoverable ones: status 4 and not a byte moves
    bm = loss_bitmap("mixed", S, k, m, rng)
    bm[S - 1, m - 1] = bm[S - 1, k + m - 1] = 0
    run_repair(gpu, st, blocks, bm, "a doubly-lost class, " + describe(k, m, bs, S, placement),
               want_status=4)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_repair_refuses_everything_lost(gpu, placement):
    """k/m = 1: a class is one data block and its parity block, and a bitmap of
    all zeros loses both everywhere."""
    S, k, m, bs = 3, 2, 2, 256
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, lay.image(blocks))
    run_repair(gpu, st, blocks, np.zeros((S, k + m), np.uint8), f"all lost, placement {placement}",
               want_status=4)
    only_data = np.ones((S, k + m), np.uint8)
    only_data[:, :k] = 0
    run_repair(gpu, st, blocks, only_data, f"all data lost, placement {placement}")


# -- 3. verify ----------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("bs", BSS)
@pytest.mark.parametrize("k,m", list(KMS))
def test_verify_flags_the_damaged_classes(gpu, k, m, bs, placement):
    S = KMS[(k, m)]
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    st = Store(lay, lay.image(blocks))
    what = describe(k, m, bs, S, placement)
    run_verify(gpu, st, blocks, what)
    if placement == "B":  # a byte between two blocks of one shard, and one between two shards
        img = [a.copy() for a in lay.image(blocks)]
        r, o = lay.at(0, 0)
        for at in (o + bs + 7, o - 3, o + lay.hull(0) + 11):
            assert img[r][at] == SENTINEL
            img[r][at] ^= 0xFF
        st.load(img)
        assert scrub(gpu, st)[:2] == ([], 0), f"a gap byte was read, {what}"
        st.assert_image(img, what)


# -- 4. rejected calls ----------------------------------------------------------
def test_rejected_calls_queue_nothing(gpu):
    torch = _torch()
    St = gpu.Status
    S, k, m, bs = 5, 4, 1, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    bm = loss_bitmap("mixed", S, k, m, np.random.default_rng(3))
    before = lay.image(blocks, bm)
    st = Store(lay, before)
    ptrs, ds, ps = st.ptrs, lay.ds, lay.ps
    d_bm, status, count = device_bitmap(bm), poison(), poison()
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    wide = (ptrs * 52)[:257]
    tables = [  # (table, data_stride, parity_stride, k, m) -> the code of steps 3 to 7
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
        assert gpu.encode_shards(t, a, b, S, bs, kk, mm) == code
        assert gpu.repair_shards_device(t, a, b, S, bs, kk, mm, d_bm, status) == code
        assert gpu.verify_shards(t, a, b, S, bs, kk, mm, flags, count) == code
        assert gpu.shards_arg_capacity_used() == 0
    # the calls' own pointers, with a table that is fine -- and ahead of one that is not
    for t in (ptrs, [ptrs[0]] * (k + m)):
        assert gpu.repair_shards_device(t, ds, ps, S, bs, k, m, None, status) == St.INVALID_SIZE
        odd = status.data_ptr() + 2
        assert gpu.repair_shards_device(t, ds, ps, S, bs, k, m, d_bm, odd) == St.INVALID_ALIGNMENT
        assert gpu.repair_shards_device(t, ds, ps, S, bs, k, m, d_bm, None) == St.INVALID_ALIGNMENT
        assert gpu.verify_shards(t, ds, ps, S, bs, k, m, None, count) == St.INVALID_SIZE
        assert gpu.verify_shards(t, ds, ps, S, bs, k, m, flags,
                                 count.data_ptr() + 1) == St.INVALID_ALIGNMENT
    assert gpu.encode_shards(ptrs, ds, ps, S, 100, k, m) == St.INVALID_SIZE
    assert gpu.repair_shards_device(ptrs, ds, ps, S, bs, 6, 4, d_bm, status) == St.INVALID_COUNTS
    torch.cuda.synchronize()
    st.assert_image(before, "after rejected calls")
    assert int(status.item()) == POISON and int(count.item()) == POISON
    assert bool((flags == 0xFF).all())
    # no stripes: success, and only the verdicts are queued
    assert gpu.encode_shards(None, ds, ps, 0, bs, k, m) == St.SUCCESS
    assert gpu.repair_shards_device(None, ds, ps, 0, bs, k, m, None, status) == St.SUCCESS
    assert gpu.verify_shards(None, ds, ps, 0, bs, k, m, None, count) == St.SUCCESS
    assert gpu.shards_arg_capacity_used() == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(count.item()) == 0
    st.assert_image(before, "after calls without stripes")


# -- 5. every launch shape ------------------------------------------------------
@pytest.mark.parametrize("k,m", [(4, 1), (16, 1), (6, 2)])
def test_every_launch_shape(gpu, k, m):
    """One shape per compiled member-count class at four tiles and a ragged one,
    in the placement with two different strides, under every (threads, unroll),
    both cache policies, a grid of two workgroups striding over the tiles and
    rotation off and 3."""
    S, bs = KMS[(k, m)], 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "B")
    st = Store(lay, lay.image(blocks))
    bm = loss_bitmap("mixed", S, k, m, np.random.default_rng(k + m))
    try:
        for threads, unroll in SHAPES:
            for policy in POLICIES:
                for max_grid, rotation in GRID_ROT:
                    assert gpu.set_launch(unroll, max_grid, policy, threads) == gpu.Status.SUCCESS
                    assert gpu.set_rotation(rotation) == gpu.Status.SUCCESS
                    what = (f"{k}+{m} threads={threads} unroll={unroll} policy={policy} "
                            f"max_grid={max_grid} rotation={rotation}")
                    run_encode(gpu, st, blocks, what)
                    run_repair(gpu, st, blocks, bm, what)
                    run_verify(gpu, st, blocks, what)
    finally:
        assert gpu.set_launch(0, 0, 0, 0) == gpu.Status.SUCCESS
        assert gpu.set_rotation(0) == gpu.Status.SUCCESS


# -- 6. queued ------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_encode_repair_verify_queued_on_one_stream(gpu, placement):
    """Encode, then repair, then the scrub issued back to back on a side stream
    with one synchronisation at the end.  Between encode and repair the lost
    blocks are overwritten with garbage by a fill queued on the same stream."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, placement)
    bm = loss_bitmap("mixed", S, k, m, np.random.default_rng(5))
    parity_lost = np.ones_like(bm)
    parity_lost[:, k:] = 0
    st = Store(lay, lay.image(blocks, parity_lost))
    masks = [torch.from_numpy(a).to("cuda") for a in lay.block_mask(bm)]
    d_bm, status, count = device_bitmap(bm), poison(), poison()
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert gpu.encode_shards(*st.args, s) == gpu.Status.SUCCESS
        for t, mask in zip(st.t, masks):
            t.masked_fill_(mask, GARBAGE)
        assert gpu.repair_shards_device(*st.args, d_bm, status, s) == gpu.Status.SUCCESS
        assert gpu.verify_shards(*st.args, flags, count, s) == gpu.Status.SUCCESS
    s.synchronize()
    assert int(status.item()) == 0 and int(count.item()) == 0
    assert int(flags.count_nonzero()) == 0
    st.assert_image(lay.image(blocks), f"queued, placement {placement}")


# -- 7. capture -------------------------------------------------------------------
def test_captured_encode_and_repair_replayed_with_other_bytes(gpu):
    """xec_encode_shards, a garbage fill of the lost blocks and
    xec_repair_shards_device captured on a side stream; every input is on the
    device before the capture, and between the replays the store, the loss mask
    and the bitmap are rewritten by device-to-device copies.  The scrub runs on a
    plain stream after each replay (a captured scrub has memset nodes, see
    xec_verify)."""
    torch = _torch()
    S, k, m, bs = 11, 6, 2, 4352
    lay = Layout(S, k, m, bs, "B")
    first = pristine(S, k, m, bs)
    rounds = []
    rng = np.random.default_rng(9)
    parity_lost = np.ones((S, k + m), np.uint8)
    parity_lost[:, k:] = 0
    for blocks, kind in ((first, "mixed"), (np.ascontiguousarray(first[::-1]), "data")):
        bm = loss_bitmap(kind, S, k, m, rng)
        rounds.append(dict(
            blocks=blocks, bm=device_bitmap(bm),
            start=[torch.from_numpy(a).to("cuda") for a in lay.image(blocks, parity_lost)],
            mask=[torch.from_numpy(a).to("cuda") for a in lay.block_mask(bm)]))
    assert not torch.equal(rounds[0]["bm"], rounds[1]["bm"])
    st = Store(lay, lay.image(first, parity_lost))
    mask = [x.clone() for x in rounds[0]["mask"]]
    d_bm, status = rounds[0]["bm"].clone(), poison()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.encode_shards(*st.args, cs) == gpu.Status.SUCCESS
        st.t[0].masked_fill_(mask[0], GARBAGE)
        assert gpu.repair_shards_device(*st.args, d_bm, status, cs) == gpu.Status.SUCCESS
    for rd in rounds:
        st.t[0].copy_(rd["start"][0])
        mask[0].copy_(rd["mask"][0])
        d_bm.copy_(rd["bm"])
        status.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        st.assert_image(lay.image(rd["blocks"]), "after a replay")
        assert scrub(gpu, st)[:2] == ([], 0)
    del g


# -- 8. kernel events ---------------------------------------------------------------
def test_kernel_events_time_one_encode_and_are_consumed(gpu):
    torch = _torch()
    S, k, m, bs = 7, 16, 1, 65536
    blocks = pristine(S, k, m, bs)
    lay = Layout(S, k, m, bs, "C")
    st = Store(lay, lay.image(blocks))
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)  # torch creates the HIP handle at the first record
    e1.record(s)
    torch.cuda.synchronize()
    assert gpu.set_kernel_events(e0, e1) == gpu.Status.SUCCESS
    assert gpu.encode_shards(*st.args, s) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1)
    assert t > 0
    # moves S*(k+m)*bs bytes: slower than HBM could, so it is the kernel's own interval
    assert S * (k + m) * bs / (t * 1e-3) / 1e9 < 8000.0
    assert gpu.encode_shards(*st.args, s) == gpu.Status.SUCCESS  # not armed any more
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) == t
    st.assert_image(lay.image(blocks), "timed encode")
