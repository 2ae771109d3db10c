"""Ranged update with digest upkeep on an MI355X: xec_update_range (host list)
and xec_update_range_device (device mask) against the CPU oracle.

Expectation model of every case: the ranges are put into a numpy copy of the
oracle's data and the result is encoded with oracle.encode_batch; data and
parity on the device must match both bit for bit -- which also says that bytes
outside the range, blocks not named and classes without an item are untouched.
With d_digests, the slot of every touched block (each updated data block and
the parity block of its class) must equal xec.digest_host of the expected
block; every other slot was seeded with a sentinel that is no digest and must
be unchanged.  Whatever of d_new the call must not read (past the list's end in
the host form; everything but the ranges of the marked blocks in the shadow) is
0xA5.
"""
from __future__ import annotations

import numpy as np
import pytest

from arena import Arena
from test_gpu_repair import Case, set_shape
from test_gpu_update import assert_state, items_of, run_update, update_set

pytestmark = pytest.mark.gpu

KM = [(4, 1), (6, 3), (32, 1), (66, 2)]
BS = [256, 1280, 4352]
SS = [1, 3]
ENTRIES = ["host", "device"]
SETS = ["one", "class", "interleaved", "third", "empty"]
LAUNCHES = [dict(block_threads=256), dict(unroll=2), dict(cache_policy=2), dict(max_grid=2),
            dict(rotation=3)]
MASK64 = (1 << 64) - 1
STALE = 0x1234


def _torch():
    import torch
    return torch


def ranges_of(bs):
    """(offset, len): one granule at the start and at the end, the whole block,
    both ends inside, a straddle of the 1 KiB chunk boundary, several chunks
    with a ragged last one -- the last two where they fit."""
    r = [(0, 16), (bs - 16, 16), (0, bs), (16, bs - 32), (1008, 48), (1008, 2064)]
    return [(o, n) for o, n in r if o + n <= bs]


def model(oracle, c: Case, ref_d, blocks, fresh, off, ln):
    """(data, parity) after [off, off+ln) of `blocks` of ref_d took the rows of `fresh`."""
    S, k, m, bs = c.S, c.k, c.m, c.bs
    d = oracle.aligned(S * k * bs)
    d[:] = ref_d
    v = d.reshape(S, k, bs)
    for t, (cs, i) in enumerate(blocks):
        v[cs, i, off:off + ln] = fresh[t]
    p = oracle.aligned(S * m * bs)
    assert oracle.encode_batch(d, p, S, bs, k, m) == 0
    return d, p


def touched_slots(c: Case, blocks):
    """Slot indices (into S*(k+m)) the call may change: the updated data blocks
    and the parity blocks of their classes."""
    row = c.k + c.m
    out = {cs * row + i for cs, i in blocks}
    out |= {cs * row + c.k + i % c.m for cs, i in blocks}
    return sorted(out)


def block_of(c: Case, d, p, slot):
    row = c.k + c.m
    cs, i = divmod(slot, row)
    if i < c.k:
        return d.reshape(c.S, c.k, c.bs)[cs, i]
    return p.reshape(c.S, c.m, c.bs)[cs, i - c.k]


def true_digests(xec, c: Case, d, p, which=None):
    """{slot: xec.digest_host(block)} of the blocks of (d, p) numpy buffers."""
    which = range(c.S * (c.k + c.m)) if which is None else which
    return {b: xec.digest_host(np.ascontiguousarray(block_of(c, d, p, b))) for b in which}


def sentinel(c: Case):
    """A value per slot that is no digest of anything here."""
    n = c.S * (c.k + c.m)
    return (np.arange(n, dtype=np.uint64) * np.uint64(0x0101010101010101)) ^ np.uint64(0xA5A5A5A5A5A5A5A5)


def seed_slots(xec, c: Case, ref_d, ref_p, blocks, bias=0):
    """Sentinels everywhere, the digests of the blocks before the call (+ bias)
    in the slots the call may touch.  Returns (host u64 array, device tensor)."""
    h = sentinel(c)
    for b, v in true_digests(xec, c, ref_d, ref_p, touched_slots(c, blocks)).items():
        h[b] = np.uint64((v + bias) & MASK64)
    return h, _torch().from_numpy(h.view(np.uint8).copy()).to("cuda")


def want_slots(xec, c: Case, seeded, exp_d, exp_p, blocks, bias=0):
    want = seeded.copy()
    for b, v in true_digests(xec, c, exp_d, exp_p, touched_slots(c, blocks)).items():
        want[b] = np.uint64((v + bias) & MASK64)
    return want


def as_u64(t) -> np.ndarray:
    return t.cpu().numpy().view("<u8")


def host_new(fresh, n, ln, pad=2):
    torch = _torch()
    new = torch.full(((n + pad) * ln,), 0xA5, dtype=torch.uint8, device="cuda")
    if n:
        new[: n * ln] = torch.from_numpy(np.ascontiguousarray(fresh).reshape(-1)).to("cuda")
    return new


def device_new(c: Case, blocks, fresh, off, ln):
    torch = _torch()
    h_shadow = np.full((c.S, c.k, c.bs), 0xA5, np.uint8)
    mask = np.zeros((c.S, c.k), np.uint8)
    for t, (cs, i) in enumerate(blocks):
        h_shadow[cs, i, off:off + ln] = fresh[t]
        mask[cs, i] = (1, 2, 255)[t % 3]  # any nonzero byte marks the block
    return (torch.from_numpy(h_shadow.reshape(-1)).to("cuda"),
            torch.from_numpy(mask.reshape(-1)).to("cuda"))


def run_range(xec, c: Case, blocks, fresh, off, ln, entry, dig=None, scratch=None,
              scratch_bytes=None, stream=None):
    """[off, off+ln) of `blocks` (sorted (stripe, i)) <- rows of `fresh` on c's buffers."""
    torch = _torch()
    S, k, m, bs = c.S, c.k, c.m, c.bs
    n = len(blocks)
    s = c.b.stream if stream is None else stream
    if entry == "host":
        new = host_new(fresh, n, ln)
        if scratch_bytes is None:
            scratch_bytes = xec.update_scratch_bytes(n)
            scratch = torch.empty(max(scratch_bytes, 4), dtype=torch.uint8, device="cuda")
        st = xec.update_range(c.d, c.p, new, S, bs, k, m, items_of(blocks), n, off, ln, dig,
                              scratch, scratch_bytes, s)
    else:
        shadow, mask = device_new(c, blocks, fresh, off, ln)
        st = xec.update_range_device(c.d, c.p, shadow, S, bs, k, m, mask, off, ln, dig, s)
    torch.cuda.synchronize()
    return st


def check_call(xec, oracle, c: Case, blocks, fresh, off, ln, entry, upkeep, what, exp=None, bias=0):
    """One call from the reference state: bytes and (with upkeep) slots."""
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    exp_d, exp_p = exp if exp is not None else model(oracle, c, ref_d, blocks, fresh, off, ln)
    dig = seeded = None
    if upkeep:
        seeded, dig = seed_slots(xec, c, ref_d, ref_p, blocks, bias)
    assert run_range(xec, c, blocks, fresh, off, ln, entry, dig) == xec.Status.SUCCESS, what
    assert_state(c, exp_d, exp_p, what)
    if upkeep:
        want = want_slots(xec, c, seeded, exp_d, exp_p, blocks, bias)
        got = as_u64(dig)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: slots {bad[:8].tolist()} (touched {touched_slots(c, blocks)[:8]})"


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_range_sets_bit_exact(gpu, oracle, k, m, bs):
    rng = np.random.default_rng(k * 1000 + m * 10 + bs)
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        ref_d = c.ref_d.cpu().numpy()
        for off, ln in ranges_of(bs):
            for kind in SETS:
                blocks = update_set(rng, S, k, m, kind)
                fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
                exp = model(oracle, c, ref_d, blocks, fresh, off, ln)
                for entry in ENTRIES:
                    for upkeep in (False, True):
                        what = f"{entry} '{kind}' [{off},+{ln}) S={S} upkeep={upkeep}"
                        try:
                            check_call(gpu, oracle, c, blocks, fresh, off, ln, entry, upkeep, what,
                                       exp)
                            used = gpu.update_tiling_used()
                            if entry == "device":
                                assert used == 2, what
                            else:
                                assert used == (0 if kind == "empty" else 4), what
                        finally:
                            c.restore()
    # no stripes at all: no device call either way
    c = Case.get(gpu, oracle, 1, k, m, bs)
    St = gpu.Status
    assert gpu.update_range_device(c.d, c.p, c.d, 0, bs, k, m, None, 0, 16, None,
                                   c.b.stream) == St.SUCCESS
    assert gpu.update_tiling_used() == 0
    assert gpu.update_range(c.d, c.p, c.d, 0, bs, k, m, items_of([(0, 0)]), 1, 0, 16, None, None, 0,
                            c.b.stream) == St.SUCCESS
    assert gpu.update_tiling_used() == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_whole_block_is_update(gpu, oracle, entry):
    """offset = 0, len = bs leaves what xec_update / xec_update_device leaves."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(5)
    blocks = update_set(rng, S, k, m, "third")
    fresh = rng.integers(0, 256, size=(len(blocks), bs), dtype=np.uint8)
    try:
        assert run_update(gpu, c, blocks, fresh, entry) == gpu.Status.SUCCESS
        d_old, p_old = c.d.clone(), c.p.clone()
        c.restore()
        for upkeep in (False, True):
            dig = seed_slots(gpu, c, c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy(), blocks)[1] \
                if upkeep else None
            assert run_range(gpu, c, blocks, fresh, 0, bs, entry, dig) == gpu.Status.SUCCESS
            assert torch.equal(c.d, d_old) and torch.equal(c.p, p_old), (entry, upkeep)
            c.restore()
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_writing_the_same_bytes_changes_nothing(gpu, oracle, entry):
    S, k, m, bs = 3, 6, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d = c.ref_d.cpu().numpy()
    rng = np.random.default_rng(6)
    blocks = update_set(rng, S, k, m, "third")
    off, ln = 1008, 2064
    fresh = np.stack([ref_d.reshape(S, k, bs)[cs, i, off:off + ln] for cs, i in blocks])
    seeded = sentinel(c)  # not even the touched slots hold a digest: the delta is 0
    dig = _torch().from_numpy(seeded.view(np.uint8).copy()).to("cuda")
    try:
        assert run_range(gpu, c, blocks, fresh, off, ln, entry, dig) == gpu.Status.SUCCESS
        c.assert_exact("after a write of the bytes already there")
        assert np.array_equal(as_u64(dig), seeded)
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_stale_slot_stays_stale_by_the_same_amount(gpu, oracle, entry):
    S, k, m, bs = 3, 6, 3, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(7)
    blocks = update_set(rng, S, k, m, "interleaved")
    off, ln = 1008, 48
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    try:
        check_call(gpu, oracle, c, blocks, fresh, off, ln, entry, True, f"stale {entry}",
                   bias=STALE)
    finally:
        c.restore()


# ---- the syndrome, the documented limit and the heal chain -----------------------
def full_slots(xec, c: Case, d, p):
    """Every slot = the digest of its block in (d, p), on the device."""
    t = true_digests(xec, c, d, p)
    h = np.array([t[b] for b in range(len(t))], dtype=np.uint64)
    return h, _torch().from_numpy(h.view(np.uint8).copy()).to("cuda")


def xor_word(c: Case, cs, i, byte, value=0x5A5A5A5A5A5A5A5A):
    """XOR one aligned 8-byte word of data block i of stripe cs on the device."""
    assert byte % 8 == 0 and i < c.k
    w = c.d.view(c.S, c.k, c.bs)[cs, i, byte:byte + 8]
    w ^= _torch().from_numpy(np.array([value], dtype="<u8").view(np.uint8).copy()).to("cuda")


def heal_chain(xec, c: Case, dig):
    """xec_verify -> xec_locate(flags) -> xec_repair_device on one stream:
    (verify's count, locate's count, repair's verdict)."""
    torch = _torch()
    S, k, m, bs, s = c.S, c.k, c.m, c.bs, c.b.stream
    n = S * (k + m)
    St = xec.Status
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    vcount = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    lcount = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    bitmap = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    wb = xec.locate_work_bytes(S, k, m)
    work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
    assert xec.verify(c.d, c.p, S, bs, k, m, flags, vcount, s) == St.SUCCESS
    assert xec.locate(c.d, c.p, S, bs, k, m, dig, flags, bitmap, lcount, work, wb, s) == St.SUCCESS
    assert xec.repair_device(c.d, c.p, S, bs, k, m, bitmap, status, s) == St.SUCCESS
    torch.cuda.synchronize()
    return int(vcount.item()), int(lcount.item()), int(status.item()), flags


def locate_all(xec, c: Case, dig):
    """Count of an xec_locate over every block."""
    torch = _torch()
    n = c.S * (c.k + c.m)
    bitmap = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    wb = xec.locate_work_bytes(c.S, c.k, c.m)
    work = torch.full((wb,), 0x3C, dtype=torch.uint8, device="cuda")
    assert xec.locate(c.d, c.p, c.S, c.bs, c.k, c.m, dig, None, bitmap, count, work, wb,
                      c.b.stream) == xec.Status.SUCCESS
    torch.cuda.synchronize()
    return int(count.item())


SYN = dict(S=3, k=6, m=3, bs=1280, blocks=[(1, 1), (1, 4), (2, 0)], off=1008, ln=48)


@pytest.mark.parametrize("entry", ENTRIES)
def test_damage_inside_the_range_moves_into_parity(gpu, oracle, entry):
    """The documented limit: old bytes damaged inside the range.  The class
    stays flagged, the data block holds exactly the new bytes, and its slot
    disagrees with it."""
    torch = _torch()
    S, k, m, bs, blocks, off, ln = (SYN[q] for q in ("S", "k", "m", "bs", "blocks", "off", "ln"))
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(8)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    exp_d, exp_p = model(oracle, c, ref_d, blocks, fresh, off, ln)
    _, dig = full_slots(gpu, c, ref_d, ref_p)
    try:
        xor_word(c, 1, 4, off + 16)  # inside [off, off + ln) of an updated block
        assert run_range(gpu, c, blocks, fresh, off, ln, entry, dig) == gpu.Status.SUCCESS
        flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
        count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        assert gpu.verify(c.d, c.p, S, bs, k, m, flags, count, c.b.stream) == gpu.Status.SUCCESS
        torch.cuda.synchronize()
        assert int(count.item()) == 1
        assert torch.nonzero(flags).flatten().tolist() == [1 * m + 4 % m]
        assert np.array_equal(c.d.cpu().numpy(), exp_d), "the data holds exactly the new bytes"
        got = as_u64(dig)
        slot = 1 * (k + m) + 4
        block = np.ascontiguousarray(exp_d.reshape(S, k, bs)[1, 4])
        assert int(got[slot]) != gpu.digest_host(block)
        # every other touched slot is right, the parity block carries the damage
        for b, v in true_digests(gpu, c, exp_d, exp_p, touched_slots(c, blocks)).items():
            if b not in (slot, 1 * (k + m) + k + 4 % m):
                assert int(got[b]) == v, b
        assert not np.array_equal(c.p.cpu().numpy(), exp_p)
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_damage_outside_the_range_heals(gpu, oracle, entry):
    S, k, m, bs, blocks, off, ln = (SYN[q] for q in ("S", "k", "m", "bs", "blocks", "off", "ln"))
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(9)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    exp_d, exp_p = model(oracle, c, ref_d, blocks, fresh, off, ln)
    _, dig = full_slots(gpu, c, ref_d, ref_p)
    try:
        xor_word(c, 1, 4, 64)  # outside the range, in an updated block
        assert run_range(gpu, c, blocks, fresh, off, ln, entry, dig) == gpu.Status.SUCCESS
        vcount, lcount, status, _ = heal_chain(gpu, c, dig)
        assert (vcount, lcount, status) == (1, 1, 0)
        assert_state(c, exp_d, exp_p, "after the heal chain")
        assert locate_all(gpu, c, dig) == 0
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_digests_are_usable_without_a_refresh(gpu, oracle, entry):
    """xec_digest of the batch, a ranged update with upkeep, then damage in an
    untouched class and in an updated block outside its range: the chain heals
    both from the kept digests, and locate's count is verify's."""
    torch = _torch()
    S, k, m, bs, blocks, off, ln = (SYN[q] for q in ("S", "k", "m", "bs", "blocks", "off", "ln"))
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d = c.ref_d.cpu().numpy()
    rng = np.random.default_rng(10)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    exp_d, exp_p = model(oracle, c, ref_d, blocks, fresh, off, ln)
    dig = torch.full((8 * S * (k + m),), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig, None, c.b.stream) == gpu.Status.SUCCESS
        assert run_range(gpu, c, blocks, fresh, off, ln, entry, dig) == gpu.Status.SUCCESS
        want = true_digests(gpu, c, exp_d, exp_p)
        assert as_u64(dig).tolist() == [want[b] for b in range(S * (k + m))]
        xor_word(c, 0, 2, 8)    # stripe 0, class 2: no item there
        xor_word(c, 1, 1, 512)  # an updated block of stripe 1, class 1, outside the range
        vcount, lcount, status, _ = heal_chain(gpu, c, dig)
        assert (vcount, lcount, status) == (2, 2, 0)
        assert_state(c, exp_d, exp_p, "after the heal chain")
        assert locate_all(gpu, c, dig) == 0
    finally:
        c.restore()


# ---- launch shapes, list capacities ---------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", LAUNCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_launch_shapes_identical(gpu, oracle, shape, entry):
    """block_threads 256, unroll 2, the default cache policy and a grid of 2
    workgroups striding over the tiles give the same bytes and slots; rotation
    3 changes nothing (it does not apply)."""
    S, k, m, bs = 3, 6, 3, 4352
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(41)
    blocks = update_set(rng, S, k, m, "third")
    try:
        set_shape(gpu, **shape)
        for off, ln in ((1008, 2064), (16, bs - 32), (bs - 16, 16)):
            fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
            for upkeep in (False, True):
                check_call(gpu, oracle, c, blocks, fresh, off, ln, entry, upkeep,
                           f"{shape} {entry} [{off},+{ln}) upkeep={upkeep}")
                c.restore()
    finally:
        set_shape(gpu)
        c.restore()


@pytest.mark.parametrize("n", [0, 64, 65, 256, 257, 1024, 1025])
def test_list_capacities_host_form(gpu, oracle, n):
    """Up to 1,024 items travel in the kernel arguments (capacities 64 / 256 /
    1024); 1,025 go through the scratch, which must be there and large enough."""
    torch = _torch()
    S, k, m, bs = 23, 66, 2, 256
    off, ln = 112, 16
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(n)
    blocks = [divmod(int(q), k) for q in np.sort(rng.permutation(S * k)[:n])]
    fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
    St = gpu.Status
    try:
        if n > 1024:
            short = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
            assert run_range(gpu, c, blocks, fresh, off, ln, "host", None, None, 0) == St.INVALID_SIZE
            assert run_range(gpu, c, blocks, fresh, off, ln, "host", None, short,
                             4 * n - 1) == St.INVALID_SIZE
            assert run_range(gpu, c, blocks, fresh, off, ln, "host", None, short.data_ptr() + 2,
                             4 * n) == St.INVALID_ALIGNMENT
            assert gpu.update_tiling_used() == 0
            c.assert_exact("after rejected scratch arguments")
        for upkeep in (False, True):
            check_call(gpu, oracle, c, blocks, fresh, off, ln, "host", upkeep, f"a list of {n}")
            assert gpu.update_tiling_used() == (0 if n == 0 else 4 if n <= 1024 else 3)
            c.restore()
    finally:
        c.restore()


# ---- rejections and minimum alignment, in a guarded arena ----------------------------
def arena_for(gpu, oracle, S, k, m, bs, n_new, ln, n_scratch=0):
    """data, parity at 64; new and shadow at 16; digests at 8; scratch at 4;
    mask at 1 -- each at exactly its minimum alignment."""
    from test_gpu_arena import arena_case
    nb = S * (k + m)
    sizes = [("data", S * k * bs, 64), ("parity", S * m * bs, 64), ("new", max(n_new * ln, 16), 16),
             ("shadow", S * k * bs, 16), ("digests", 8 * nb, 8),
             ("scratch", max(4 * n_scratch, 4), 4), ("mask", S * k, 1)]
    edge = max(bs, 4096)
    a = Arena(Arena.room([(nbytes, al) for _, nbytes, al in sizes], edge), "cuda", edge)
    for name, nbytes, al in sizes:
        a.carve(name, nbytes, al)
    assert a.ptr("new") % 32 == 16 and a.ptr("shadow") % 32 == 16 and a.ptr("digests") % 16 == 8
    assert a.ptr("scratch") % 8 == 4
    c = arena_case(gpu, oracle, a, S, k, m, bs)
    return a, c


def test_rejections_in_order_change_nothing(gpu, oracle):
    """Every rejection of the check list returns its status, an earlier check
    wins over a later one, and nothing in the arena changes."""
    S, k, m, bs = 3, 6, 3, 1280
    off, ln = 1008, 48
    blocks = [(0, 1), (1, 0), (1, 5)]
    n = len(blocks)
    a, c = arena_for(gpu, oracle, S, k, m, bs, n, ln, n_scratch=1100)
    St, s = gpu.Status, c.b.stream
    a.fill("new", 0x5A)
    a.fill("shadow", 0x5A)
    a.fill("mask", 1)
    ok = items_of(blocks)
    NEW, SH, DIG, D, P = a.ptr("new"), a.ptr("shadow"), a.ptr("digests"), a.ptr("data"), a.ptr("parity")
    nd, npar = S * k * bs, S * m * bs

    def host(d=D, new=NEW, S_=S, bs_=bs, k_=k, m_=m, it=ok, n_=n, off_=off, ln_=ln, dig=DIG,
             scr=None, scr_bytes=0):
        st = gpu.update_range(d, P, new, S_, bs_, k_, m_, it, n_, off_, ln_, dig, scr, scr_bytes, s)
        assert gpu.update_tiling_used() == 0
        return st

    def dev(d=D, new=SH, S_=S, bs_=bs, k_=k, m_=m, mask=a.ptr("mask"), off_=off, ln_=ln, dig=DIG):
        st = gpu.update_range_device(d, P, new, S_, bs_, k_, m_, mask, off_, ln_, dig, s)
        assert gpu.update_tiling_used() == 0
        return st

    bad_items = np.array([ok[1], ok[0], ok[2]], dtype=np.uint32)
    # 2. xec_check_args, ahead of everything behind it
    assert host(d=D + 16, off_=8, new=None) == St.INVALID_ALIGNMENT
    assert dev(d=D + 16, off_=8, new=None) == St.INVALID_ALIGNMENT
    assert host(bs_=100) == St.INVALID_SIZE and dev(bs_=100) == St.INVALID_SIZE
    assert host(k_=5) == St.INVALID_COUNTS and dev(k_=5) == St.INVALID_COUNTS
    # 3. nothing to do is a success even with arguments a later check rejects
    assert host(n_=0, off_=8, new=None, dig=DIG + 4) == St.SUCCESS
    assert host(S_=0, off_=8, new=None, dig=DIG + 4) == St.SUCCESS
    assert dev(S_=0, off_=8, new=None, mask=None) == St.SUCCESS
    # 4. the packing (host form only), ahead of the range
    assert host(k_=264, m_=4, off_=8) == St.INVALID_SIZE
    assert host(S_=(1 << 24) + 1, new=NEW + 8) == St.INVALID_SIZE
    # 5. the range, ahead of NULL pointers and alignment
    for o, l in ((off, 0), (8, 32), (16, 24), (bs - 16, 32), (bs + 16, 16), (bs, 16)):
        assert host(off_=o, ln_=l, new=NEW + 8) == St.INVALID_SIZE, (o, l)
        assert dev(off_=o, ln_=l, new=SH + 8) == St.INVALID_SIZE, (o, l)
    # 6. NULL pointers, ahead of alignment
    assert host(new=None, dig=DIG + 4) == St.INVALID_SIZE
    assert host(it=None, new=NEW + 8) == St.INVALID_SIZE
    assert dev(new=None, dig=DIG + 4) == St.INVALID_SIZE
    assert dev(mask=None, new=SH + 8) == St.INVALID_SIZE
    # 7. alignment, ahead of the overlaps
    assert host(new=D + 8) == St.INVALID_ALIGNMENT and dev(new=D + 8) == St.INVALID_ALIGNMENT
    assert host(dig=D + 4) == St.INVALID_ALIGNMENT and dev(dig=P + 4) == St.INVALID_ALIGNMENT
    # 8. the overlaps, ahead of the item rules
    assert host(new=D + 16, it=bad_items) == St.INVALID_SIZE           # on the data
    assert host(new=P + npar - 16, it=bad_items) == St.INVALID_SIZE    # its first granule on the parity
    assert host(new=D - n * ln + 16) == St.INVALID_SIZE                # its last granule on the data
    assert dev(new=D) == St.INVALID_SIZE and dev(new=P - nd + 16) == St.INVALID_SIZE
    assert host(dig=D + nd - 8) == St.INVALID_SIZE and dev(dig=P) == St.INVALID_SIZE
    assert host(dig=NEW + n * ln - 8) == St.INVALID_SIZE               # digests on d_new
    assert dev(dig=SH + 8) == St.INVALID_SIZE
    # 9. the item rules (host form), ahead of the scratch
    assert host(it=bad_items) == St.INVALID_COUNTS                                       # unsorted
    assert host(it=np.array([ok[0], ok[1], ok[1]], np.uint32)) == St.INVALID_COUNTS      # duplicate
    assert host(it=np.array([ok[0], (1 << 8) | k, ok[2]], np.uint32)) == St.INVALID_COUNTS
    assert host(it=np.array([ok[0], ok[1], (S << 8)], np.uint32)) == St.INVALID_COUNTS
    # 10. the scratch rules past 1,024 items (the arena's `new` is too short for
    # them, so d_new is a buffer outside it; the call is rejected before any read)
    torch = _torch()
    many = np.arange(1100, dtype=np.uint32)
    many = ((many // k) << 8 | (many % k)).astype(np.uint32)
    S_big = 1100 // k + 1
    big = torch.full((1100 * ln,), 0x5A, dtype=torch.uint8, device="cuda")
    # (data and parity extents grow with S_big; the arena regions are not touched either way)
    bigd = torch.zeros(S_big * k * bs, dtype=torch.uint8, device="cuda")
    bigp = torch.zeros(S_big * m * bs, dtype=torch.uint8, device="cuda")
    bigdig = torch.zeros(8 * S_big * (k + m), dtype=torch.uint8, device="cuda")

    def long(scr, scr_bytes):
        st = gpu.update_range(bigd, bigp, big, S_big, bs, k, m, many, 1100, off, ln, bigdig, scr,
                              scr_bytes, s)
        assert gpu.update_tiling_used() == 0
        return st

    assert long(a.ptr("scratch") + 2, 4400) == St.INVALID_ALIGNMENT
    assert long(None, 4400) == St.INVALID_SIZE
    assert long(a.ptr("scratch"), 4399) == St.INVALID_SIZE
    torch.cuda.synchronize()
    assert int(bigd.count_nonzero()) == 0 and int(bigp.count_nonzero()) == 0
    assert int(bigdig.count_nonzero()) == 0
    a.check(writable=[], what="after every rejection")
    c.assert_exact("after every rejection")
    # ranges that only touch are allowed: d_new ending exactly where the data
    # begins (the band in front of it is readable arena memory)
    assert (D - n * ln) % 16 == 0
    assert gpu.update_range(D, P, D - n * ln, S, bs, k, m, ok, n, off, ln, DIG, None, 0,
                            s) == St.SUCCESS
    assert gpu.update_tiling_used() == 4
    torch.cuda.synchronize()
    a.check(writable=["data", "parity", "digests"], what="d_new touching the data")
    c.restore()
    a.adopt(["data", "parity"])


@pytest.mark.parametrize("bs", [256, 8448])
def test_minimum_alignment_in_a_guarded_arena(gpu, oracle, bs):
    """Both calls, with and without upkeep, on regions at exactly their least
    alignment, over ranges that end on the last granule of the block: nothing
    but data, parity and (with upkeep) the digests changes -- nor the scratch's
    neighbours when a list of more than 1,024 items is uploaded."""
    if bs == 256:
        S, k, m, n = 23, 66, 2, 1100
    else:
        S, k, m, n = 3, 6, 3, 7
    rng = np.random.default_rng(bs)
    blocks = [divmod(int(q), k) for q in np.sort(rng.permutation(S * k)[:n])]
    ranges = [(bs - 16, 16), (bs - 48, 48)] + ([(1008, bs - 1008)] if bs > 1024 else [(0, bs)])
    ln_max = max(l for _, l in ranges)
    a, c = arena_for(gpu, oracle, S, k, m, bs, n + 1, ln_max, n_scratch=n)
    St, s = gpu.Status, c.b.stream
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    scr, scr_bytes = (a["scratch"], 4 * n) if n > 1024 else (None, 0)
    for off, ln in ranges:
        fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
        exp_d, exp_p = model(oracle, c, ref_d, blocks, fresh, off, ln)
        h_new = np.full(a.size("new"), 0xA5, np.uint8)
        h_new[: n * ln] = fresh.reshape(-1)
        a.put("new", h_new)
        h_shadow = np.full((S, k, bs), 0xA5, np.uint8)
        h_mask = np.zeros((S, k), np.uint8)
        for t, (cs, i) in enumerate(blocks):
            h_shadow[cs, i, off:off + ln] = fresh[t]
            h_mask[cs, i] = (1, 2, 255)[t % 3]
        a.put("shadow", h_shadow)
        a.put("mask", h_mask)
        for entry in ENTRIES:
            for upkeep in (False, True):
                what = f"{entry} [{off},+{ln}) upkeep={upkeep} bs={bs}"
                seeded, _ = seed_slots(gpu, c, ref_d, ref_p, blocks)
                a.put("digests", seeded)
                dig = a["digests"] if upkeep else None
                if entry == "host":
                    st = gpu.update_range(c.d, c.p, a["new"], S, bs, k, m, items_of(blocks), n, off,
                                          ln, dig, scr, scr_bytes, s)
                else:
                    st = gpu.update_range_device(c.d, c.p, a["shadow"], S, bs, k, m, a["mask"], off,
                                                 ln, dig, s)
                assert st == St.SUCCESS, what
                assert_state(c, exp_d, exp_p, what)
                writable = ["data", "parity"] + (["digests"] if upkeep else [])
                if entry == "host" and n > 1024:
                    writable.append("scratch")
                if upkeep:
                    want = want_slots(gpu, c, seeded, exp_d, exp_p, blocks)
                    assert np.array_equal(as_u64(a["digests"]), want), what
                a.check(writable=writable, what=what)
                c.restore()
                a.adopt(["data", "parity"])


# ---- capture, kernel events ------------------------------------------------------------
def test_host_form_refuses_graph_capture(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    new = torch.full((2 * 48,), 0x3C, dtype=torch.uint8, device="cuda")
    dig = torch.full((8 * S * (k + m),), 0xA5, dtype=torch.uint8, device="cuda")
    items = items_of([(0, 1), (2, 5)])
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.update_range(c.d, c.p, new, S, bs, k, m, items, 2, 1008, 48, dig, None, 0,
                                    cs) == St.DEVICE_ERROR
            assert gpu.update_tiling_used() == 0
            assert gpu.update_range(c.d, c.p, new, S, bs, k, m, items, 0, 1008, 48, dig, None, 0,
                                    cs) == St.SUCCESS
        g.replay()  # an empty graph
        torch.cuda.synchronize()
        del g
        c.assert_exact("after a refused capture")
        assert int((dig != 0xA5).sum()) == 0
    finally:
        c.restore()


def test_graph_of_update_range_device_with_upkeep(gpu, oracle):
    """The device form with upkeep, captured alone and replayed twice: both
    masks, both shadows and both expected states and slot arrays are on the
    device before the capture, and between the replays mask and shadow are only
    rewritten by device-to-device copies from outside the graph.  The second
    replay works on what the first left, digests included."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 4352
    off, ln = 1008, 2064
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(23)
    state = c.ref_d.cpu().numpy()
    dig = full_slots(gpu, c, state, c.ref_p.cpu().numpy())[1]
    masks, shadows, want = [], [], []
    for kind in ("third", "interleaved"):
        blocks = update_set(rng, S, k, m, kind)
        fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
        state, exp_p = model(oracle, c, state, blocks, fresh, off, ln)
        shadow, mask = device_new(c, blocks, fresh, off, ln)
        masks.append(mask)
        shadows.append(shadow)
        slots = full_slots(gpu, c, state, exp_p)[1]
        want.append((torch.from_numpy(state.copy()).to("cuda"), torch.from_numpy(exp_p).to("cuda"),
                     slots))
    assert not torch.equal(masks[0], masks[1])
    mask, shadow = masks[0].clone(), shadows[0].clone()
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.update_range_device(c.d, c.p, shadow, S, bs, k, m, mask, off, ln, dig,
                                           cs) == St.SUCCESS
            assert gpu.update_tiling_used() == 2
        for r in range(2):
            mask.copy_(masks[r])
            shadow.copy_(shadows[r])
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(c.d, want[r][0]), f"data != model after replay {r}"
            assert torch.equal(c.p, want[r][1]), f"parity != model after replay {r}"
            assert torch.equal(dig, want[r][2]), f"slots != digests after replay {r}"
        del g
    finally:
        c.restore()


def test_kernel_events_cover_both_calls(gpu, oracle):
    """An armed pair is consumed by each new call -- also one that launches
    nothing -- and times the kernel: a positive interval."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 4352
    off, ln = 1008, 2064
    c = Case.get(gpu, oracle, S, k, m, bs)
    s = c.b.stream
    rng = np.random.default_rng(29)
    blocks = update_set(rng, S, k, m, "third")
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    dig = torch.zeros(8 * S * (k + m), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    try:
        for entry in ENTRIES:
            for e in ev:
                e.record(s)  # torch creates the HIP handle at the first record
            torch.cuda.synchronize()
            base = ev[0].elapsed_time(ev[1])
            assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
            # an empty list launches nothing, but consumes the setting
            assert run_range(gpu, c, [], fresh[:0], off, ln, "host", dig) == gpu.Status.SUCCESS
            assert gpu.encode(c.d, c.p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed
            torch.cuda.synchronize()
            assert ev[0].elapsed_time(ev[1]) == base
            # the buffers are built first: the armed call is the very next library call
            if entry == "host":
                new = host_new(fresh, len(blocks), ln)
                torch.cuda.synchronize()
                assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
                st = gpu.update_range(c.d, c.p, new, S, bs, k, m, items_of(blocks), len(blocks), off,
                                      ln, dig, None, 0, s)
            else:
                shadow, mask = device_new(c, blocks, fresh, off, ln)
                torch.cuda.synchronize()
                assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
                st = gpu.update_range_device(c.d, c.p, shadow, S, bs, k, m, mask, off, ln, dig, s)
            assert st == gpu.Status.SUCCESS
            torch.cuda.synchronize()
            t_kernel = ev[0].elapsed_time(ev[1])
            assert t_kernel > 0 and t_kernel != base, entry
            assert gpu.encode(c.d, c.p, S, bs, k, m, s) == gpu.Status.SUCCESS  # not armed any more
            torch.cuda.synchronize()
            assert ev[0].elapsed_time(ev[1]) == t_kernel
            c.restore()
    finally:
        c.restore()
