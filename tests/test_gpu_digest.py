"""Block digests and xec_locate on an MI355X.

Every expected digest is the numpy restatement of the formula
(tests/test_digest_abi.py np_digest) over the CPU oracle's data and parity;
every expected bitmap is built here from the blocks the test damaged.  Nothing
the library computed is compared with itself.

The digest kernel's tile is a 64 KiB segment of one block
(kDigestSegmentBytes, csrc/xec_kernels.h), so BIG = 2 * 64 KiB + 256 bytes
makes three workgroups -- two full segments and a ragged quarter tile -- add
into one slot.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_digest_abi import np_digest
from test_gpu_repair import Case, set_shape

pytestmark = pytest.mark.gpu

KM = [(4, 1), (8, 4), (12, 3), (6, 6), (32, 1), (66, 2)]
BS = [256, 1280, 4352]  # a quarter of a one-wave tile; one tile and a ragged one; 4 and a ragged
SS = [1, 3, 23]
BIG = 2 * (64 << 10) + 256  # two digest segments and a ragged tail
OVERRIDES = [dict(), dict(block_threads=256), dict(cache_policy=2), dict(max_grid=2)]


def _torch():
    import torch
    return torch


def ref_digests(c: Case) -> np.ndarray:
    """(S, k+m) uint64 from the oracle's bytes: k data slots, then m parity slots."""
    key = "_np_digests"
    if not hasattr(c, key):
        d = np_digest(c.ref_d.cpu().numpy().reshape(c.S, c.k, c.bs))
        p = np_digest(c.ref_p.cpu().numpy().reshape(c.S, c.m, c.bs))
        setattr(c, key, np.concatenate([d, p], axis=1))
    return getattr(c, key)


def slots(c: Case, fill=0xA5):
    """S*(k+m) u64 of device memory as bytes, prefilled."""
    return _torch().full((8 * c.S * (c.k + c.m),), fill, dtype=_torch().uint8, device="cuda")


def as_u64(t) -> np.ndarray:
    return t.cpu().numpy().view("<u8")


def stored(c: Case):
    """The reference digests on the device (what a parity store would keep)."""
    return _torch().from_numpy(ref_digests(c).reshape(-1).view(np.uint8).copy()).to("cuda")


def flip(c: Case, cs, i, byte, bit=0x10):
    """Flip one bit of block i (i >= k: parity block i - k) of stripe cs."""
    if i < c.k:
        c.d.view(c.S, c.k, c.bs)[cs, i, byte] ^= bit
    else:
        c.p.view(c.S, c.m, c.bs)[cs, i - c.k, byte] ^= bit


def run_locate(xec, c: Case, dig, flags=None, work=None):
    """(status, bitmap (S, k+m), count) of one xec_locate on c's buffers."""
    torch = _torch()
    n = c.S * (c.k + c.m)
    bitmap = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wb = xec.locate_work_bytes(c.S, c.k, c.m)
    if work is None:
        work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
    st = xec.locate(c.d, c.p, c.S, c.bs, c.k, c.m, dig, flags, bitmap, count, work, wb, c.b.stream)
    torch.cuda.synchronize()
    return st, bitmap.cpu().numpy().reshape(c.S, c.k + c.m), int(count.item())


def expect_bitmap(c: Case, bad):
    bm = np.ones((c.S, c.k + c.m), np.uint8)
    for cs, i in bad:
        bm[cs, i] = 0
    return bm


def run_verify(xec, c: Case):
    torch = _torch()
    flags = torch.full((c.S * c.m,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    assert xec.verify(c.d, c.p, c.S, c.bs, c.k, c.m, flags, count, c.b.stream) == xec.Status.SUCCESS
    torch.cuda.synchronize()
    return flags, int(count.item())


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_digest_all_blocks_equals_numpy(gpu, oracle, k, m, bs):
    torch = _torch()
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        dig = slots(c)
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, c.b.stream) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert np.array_equal(as_u64(dig), ref_digests(c).reshape(-1)), f"S={S}"
        c.assert_exact("after a digest")
    # one block against the host digest's known answer shape: digest_host is the same sum
    assert gpu.digest_host(c.ref_d[:bs].cpu().numpy()) == int(ref_digests(c)[0, 0])
    # no stripes: success, nothing written, NULL digests allowed
    dig = slots(c)
    assert gpu.digest(c.d, c.p, 0, bs, k, m, None, None, c.b.stream) == gpu.Status.SUCCESS
    assert gpu.digest(c.d, c.p, 0, bs, k, m, dig, None, c.b.stream) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    assert int((dig != 0xA5).sum()) == 0


@pytest.mark.parametrize("shape", OVERRIDES,
                         ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()) or "default")
@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, BIG, 3), (4, 1, BIG, 1)])
def test_digest_launch_overrides_and_segments(gpu, oracle, k, m, bs, S, shape):
    """The default launch, 256 threads per workgroup, the default cache policy
    and a grid of 2 workgroups striding over the tiles give the same bits; at
    BIG three workgroups' partial sums meet in every slot."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    dig = slots(c)
    try:
        set_shape(gpu, **shape)
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, c.b.stream) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
    finally:
        set_shape(gpu)
    assert np.array_equal(as_u64(dig), ref_digests(c).reshape(-1))


@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, 1280, 3), (66, 2, 256, 3),
                                      (4, 1, BIG, 3)])
def test_digest_selection(gpu, oracle, k, m, bs, S):
    """Selected slots equal numpy, unselected ones keep their prefill; 1, 2 and
    255 all select; an all-zero selection writes nothing."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    n = S * (k + m)
    rng = np.random.default_rng(n + bs)
    want = ref_digests(c).reshape(-1)
    pre = np.frombuffer(b"\xA5" * 8, dtype="<u8")[0]
    for kind in ("third", "one", "last", "none", "all"):
        pick = {"third": rng.random(n) < 1 / 3, "one": np.arange(n) == n // 2,
                "last": np.arange(n) == n - 1, "none": np.zeros(n, bool),
                "all": np.ones(n, bool)}[kind]
        sel = np.where(pick, rng.choice(np.array([1, 2, 255], np.uint8), size=n), 0).astype(np.uint8)
        if kind == "third":
            sel[0], sel[1], sel[2] = 1, 2, 255  # each nonzero value is used at least once
            pick = sel != 0
        dig = slots(c)
        st = gpu.digest(c.d, c.p, S, bs, k, m, dig, torch.from_numpy(sel).to("cuda"), c.b.stream)
        assert st == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        got = as_u64(dig)
        assert np.array_equal(got[pick], want[pick]), kind
        assert np.all(got[~pick] == pre), f"{kind}: an unselected slot was written"
    c.assert_exact("after selected digests")


@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_locate_full_names_the_damaged_block(gpu, oracle, k, m, bs):
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        dig = stored(c)
        rng = np.random.default_rng(S * 100 + k + bs)
        st, bm, cnt = run_locate(gpu, c, dig)
        assert st == gpu.Status.SUCCESS and cnt == 0 and np.all(bm == 1), f"intact, S={S}"
        cs = S // 2
        cases = {
            "data bit": [(cs, int(rng.integers(k)), int(rng.integers(bs)))],
            "parity bit": [(cs, k + int(rng.integers(m)), int(rng.integers(bs)))],
            "last word": [(S - 1, k - 1, bs - 1)],  # the ragged tile's last word, where bs has one
            "one per stripe": [(q, int(rng.integers(k + m)), int(rng.integers(bs)))
                               for q in range(S)],
        }
        for name, damage in cases.items():
            try:
                for q, i, byte in damage:
                    flip(c, q, i, byte, 1 << int(rng.integers(8)))
                st, bm, cnt = run_locate(gpu, c, dig)
                assert st == gpu.Status.SUCCESS, name
                assert np.array_equal(bm, expect_bitmap(c, [(q, i) for q, i, _ in damage])), \
                    f"{name}, S={S}"
                assert cnt == len(damage), name
            finally:
                c.restore()


def test_locate_full_at_segment_boundaries(gpu, oracle):
    """BIG blocks: a bit in each of the three segments of one block, one at a time."""
    k, m, S = 4, 1, 3
    c = Case.get(gpu, oracle, S, k, m, BIG)
    dig = stored(c)
    for byte in (0, (64 << 10) - 1, 64 << 10, 2 * (64 << 10), BIG - 1):
        try:
            flip(c, 1, 2, byte, 0x80)
            st, bm, cnt = run_locate(gpu, c, dig)
            assert st == gpu.Status.SUCCESS and cnt == 1
            assert np.array_equal(bm, expect_bitmap(c, [(1, 2)])), byte
        finally:
            c.restore()


@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, 1280, 3), (4, 1, 256, 1)])
def test_cancelling_errors_are_found_by_a_full_locate(gpu, oracle, k, m, bs, S):
    """The same bit at the same offset of two blocks of one class: the class
    still XORs to zero, so xec_verify flags nothing; both digests differ."""
    c = Case.get(gpu, oracle, S, k, m, bs)
    dig = stored(c)
    cs, j = S // 2, m - 1
    pairs = [((cs, j), (cs, j + m)), ((cs, j), (cs, k + j))]  # two data blocks; data and parity
    for a, b in pairs:
        try:
            flip(c, *a, bs - 3, 0x04)
            flip(c, *b, bs - 3, 0x04)
            flags, count = run_verify(gpu, c)
            assert count == 0 and int(flags.count_nonzero()) == 0  # invisible to the scrub
            st, bm, cnt = run_locate(gpu, c, dig)
            assert st == gpu.Status.SUCCESS and cnt == 2
            assert np.array_equal(bm, expect_bitmap(c, [a, b]))
        finally:
            c.restore()


@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, 1280, 3), (66, 2, 256, 3)])
def test_locate_with_flags_checks_flagged_classes_only(gpu, oracle, k, m, bs, S):
    """A stored digest of an unflagged class is perturbed (its block is intact,
    so its class XORs to zero): with verify's flags that block still reads 1,
    without them it reads 0.  The damaged block of the flagged class reads 0."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    tot = k + m
    bad = (S // 2, m + 1)    # a data block of class 1; its class gets flagged
    cls = bad[1] % m
    other = (S - 1, k - 1)   # a data block of class m - 1 of another stripe: not flagged
    assert (other[0], other[1] % m) != (bad[0], cls)
    h = ref_digests(c).copy()
    h[other] ^= np.uint64(1)                        # stale stored digest, unflagged class
    dig = torch.from_numpy(h.reshape(-1).view(np.uint8).copy()).to("cuda")
    try:
        flip(c, *bad, 17, 0x01)
        flags, count = run_verify(gpu, c)
        assert count == 1 and torch.nonzero(flags).flatten().tolist() == [bad[0] * m + cls]
        # the unchecked slots of the scratch hold garbage that would not match
        st, bm, cnt = run_locate(gpu, c, dig, flags)
        assert st == gpu.Status.SUCCESS
        assert np.array_equal(bm, expect_bitmap(c, [bad])), "the gate let an unflagged class in"
        assert cnt == 1
        st, bm, cnt = run_locate(gpu, c, dig)  # no flags: both
        assert np.array_equal(bm, expect_bitmap(c, [bad, other])) and cnt == 2
        # flags of 2 and 255 count as set too
        flags[bad[0] * m + cls] = 255
        st, bm, cnt = run_locate(gpu, c, dig, flags)
        assert np.array_equal(bm, expect_bitmap(c, [bad])) and cnt == 1
        assert bm.shape == (S, tot)
    finally:
        c.restore()


@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, 1280, 3), (32, 1, 256, 3),
                                      (4, 1, BIG, 3)])
def test_heal_chain(gpu, oracle, k, m, bs, S):
    """encode (the shared batch), digest, corrupt, then verify -> locate(flags)
    -> repair_device on one stream with no host step in between."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    St, s = gpu.Status, c.b.stream
    n = S * (k + m)
    dig = slots(c)
    assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, s) == St.SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(dig), ref_digests(c).reshape(-1))
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    vcount = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    bitmap = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    lcount = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wb = gpu.locate_work_bytes(S, k, m)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")

    def chain():
        assert gpu.verify(c.d, c.p, S, bs, k, m, flags, vcount, s) == St.SUCCESS
        assert gpu.locate(c.d, c.p, S, bs, k, m, dig, flags, bitmap, lcount, work, wb,
                          s) == St.SUCCESS
        assert gpu.repair_device(c.d, c.p, S, bs, k, m, bitmap, status, s) == St.SUCCESS
        torch.cuda.synchronize()

    # one damaged block in each of several classes: a data block, a parity block, and
    # (more than one stripe) a data block of another stripe
    damage = [(S // 2, k - 1, bs - 1), (0, k + 0, 5), (S - 1, 0, 129)]
    assert len({(q, i % m if i < k else i - k) for q, i, _ in damage}) == 3  # three classes
    try:
        for q, i, byte in damage:
            flip(c, q, i, byte, 0x40)
        chain()
        assert int(status.item()) == 0
        assert int(vcount.item()) == len(damage) == int(lcount.item())
        c.assert_exact("after the heal chain")  # data and parity are the originals again
        _, again = run_verify(gpu, c)
        assert again == 0
        # two damaged blocks in one class: the verdict is 4 and nothing is written
        a, b = (S // 2, m - 1, 0), (S // 2, k + m - 1, bs // 2)
        flip(c, *a, 0x02)
        flip(c, *b, 0x08)
        hurt_d, hurt_p = c.d.clone(), c.p.clone()
        chain()
        assert int(status.item()) == 4
        assert int(vcount.item()) == 1 and int(lcount.item()) == 2
        assert torch.equal(c.d, hurt_d) and torch.equal(c.p, hurt_p)
    finally:
        c.restore()


@pytest.mark.parametrize("k,m,bs,S", [(12, 3, 4352, 23), (8, 4, 1280, 3)])
def test_refresh_after_update(gpu, oracle, k, m, bs, S):
    """xec_update of a few blocks: against the old digests a full locate names
    exactly those blocks and their classes' parity blocks; after an xec_digest
    over that selection it names nothing."""
    torch = _torch()
    c = Case.get(gpu, oracle, S, k, m, bs)
    St, s = gpu.Status, c.b.stream
    tot = k + m
    blocks = sorted({(0, 1), (S // 2, k - 1), (S - 1, 0), (S - 1, m)})  # the last two share a class
    rng = np.random.default_rng(S + bs)
    fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
    items = np.array([(q << 8) | i for q, i in blocks], dtype=np.uint32)
    changed = sorted(set(blocks) | {(q, k + i % m) for q, i in blocks})
    dig = stored(c)
    try:
        new = torch.from_numpy(fresh.reshape(-1)).to("cuda")
        assert gpu.update(c.d, c.p, new, S, bs, k, m, items, len(items), None, 0, s) == St.SUCCESS
        torch.cuda.synchronize()
        st, bm, cnt = run_locate(gpu, c, dig)
        assert st == St.SUCCESS and np.array_equal(bm, expect_bitmap(c, changed))
        assert cnt == len(changed)
        sel = np.zeros((S, tot), np.uint8)
        for q, i in changed:
            sel[q, i] = 1
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig,
                          torch.from_numpy(sel.reshape(-1)).to("cuda"), s) == St.SUCCESS
        st, bm, cnt = run_locate(gpu, c, dig)
        assert st == St.SUCCESS and cnt == 0 and np.all(bm == 1)
        # and the refreshed digests are numpy's of the new bytes
        got = as_u64(dig).reshape(S, tot)
        for t, (q, i) in enumerate(blocks):
            assert int(got[q, i]) == int(np_digest(fresh[t]))
    finally:
        c.restore()


def test_rejected_calls_write_nothing(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    St, s = gpu.Status, c.b.stream
    n = S * (k + m)
    wb = gpu.locate_work_bytes(S, k, m)
    assert wb == 8 * n
    dig = slots(c)
    work = slots(c, 0x3C)
    bitmap = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    flags = torch.ones(S * m, dtype=torch.uint8, device="cuda")
    D, P = c.d, c.p

    def dg(d=D, p=P, bs_=bs, k_=k, digests=dig, sel=None):
        return gpu.digest(d, p, S, bs_, k_, m, digests, sel, s)

    def lc(d=D, bs_=bs, k_=k, digests=dig, fl=flags, bmp=bitmap, cnt=count, wk=work, wbytes=wb):
        return gpu.locate(d, P, S, bs_, k_, m, digests, fl, bmp, cnt, wk, wbytes, s)

    assert dg(d=D.data_ptr() + 16) == St.INVALID_ALIGNMENT        # xec_check_args first
    assert dg(bs_=100) == St.INVALID_SIZE
    assert dg(k_=6) == St.INVALID_COUNTS
    assert dg(digests=None) == St.INVALID_SIZE
    assert dg(digests=dig.data_ptr() + 4) == St.INVALID_ALIGNMENT
    assert dg(bs_=100, digests=None) == St.INVALID_SIZE           # check_args ahead of the rest
    assert lc(d=D.data_ptr() + 16) == St.INVALID_ALIGNMENT
    assert lc(k_=6, digests=None) == St.INVALID_COUNTS
    assert lc(digests=None) == St.INVALID_SIZE
    assert lc(wk=None) == St.INVALID_SIZE
    assert lc(wbytes=wb - 1) == St.INVALID_SIZE
    assert lc(wbytes=0) == St.INVALID_SIZE
    assert lc(digests=dig.data_ptr() + 4) == St.INVALID_ALIGNMENT
    assert lc(wk=work.data_ptr() + 4, wbytes=wb - 4) == St.INVALID_SIZE  # size ahead of alignment
    assert lc(wk=work.data_ptr() + 4) == St.INVALID_ALIGNMENT
    assert lc(cnt=count.data_ptr() + 2) == St.INVALID_ALIGNMENT
    assert lc(bmp=None) == St.INVALID_SIZE
    assert lc(bmp=None, cnt=count.data_ptr() + 2) == St.INVALID_ALIGNMENT  # alignment ahead of it
    torch.cuda.synchronize()
    assert int((dig != 0xA5).sum()) == 0
    assert int((bitmap != 0xA5).sum()) == 0
    assert count.tolist() == [77, 77]
    c.assert_exact("after rejected calls")
    # S == 0: success, *d_count = 0, nothing else written
    assert gpu.locate(D, P, 0, bs, k, m, None, None, None, count, None, 0, s) == St.SUCCESS
    torch.cuda.synchronize()
    assert count.tolist() == [0, 77]
    assert int((bitmap != 0xA5).sum()) == 0
    # the same arguments, accepted
    assert lc(digests=stored(c)) == St.SUCCESS
    torch.cuda.synchronize()
    assert count.tolist() == [0, 77] and int((bitmap != 1).sum()) == 0


def test_captured_digest(gpu, oracle):
    """xec_digest with d_select == NULL captured in a hipGraph -- every input
    is on the device before the capture -- and replayed once."""
    torch = _torch()
    S, k, m, bs = 23, 12, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    want = ref_digests(c).reshape(-1)
    dig = slots(c)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, cs) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = as_u64(dig)
    del g
    assert np.array_equal(got, want)


def test_kernel_events_cover_digest_and_locate(gpu, oracle):
    """An armed pair times the digest kernel of either call and is consumed by
    it: the codec call after it records nothing."""
    torch = _torch()
    S, k, m, bs = 23, 12, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    s = c.b.stream
    dig = stored(c)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    flags, _ = run_verify(gpu, c)
    for call in ("digest", "locate"):
        # torch creates an event's HIP handle at its first record.  Twenty encodes lie
        # between the two records, so the interval they leave (tens of microseconds)
        # cannot be mistaken for one kernel of this shape (a few microseconds).
        ev[0].record(s)
        for _ in range(20):
            assert gpu.encode(c.d, c.p, S, bs, k, m, s) == gpu.Status.SUCCESS
        ev[1].record(s)
        torch.cuda.synchronize()
        base = ev[0].elapsed_time(ev[1])
        assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
        if call == "digest":
            assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, s) == gpu.Status.SUCCESS
            torch.cuda.synchronize()
        else:
            st, bm, cnt = run_locate(gpu, c, dig)
            assert st == gpu.Status.SUCCESS and cnt == 0
        t_kernel = ev[0].elapsed_time(ev[1])
        assert t_kernel > 0 and t_kernel != base, call
        flags2, _ = run_verify(gpu, c)  # not armed any more
        assert ev[0].elapsed_time(ev[1]) == t_kernel
    c.assert_exact("after timed digests")
