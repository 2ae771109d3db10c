"""Degraded write on an MI355X: xec_write (host bitmap and list) and
xec_write_device (device bitmap and mask) against the CPU oracle.

Every case: the oracle's batch, every lost block overwritten ON THE DEVICE with
GARBAGE, the write, then
  * every present block equals the model -- a numpy patch of the ranges; the
    parity of a delta or rebuild-write class is oracle.encode_batch of the
    patched data inside the range and unchanged outside it; a lost parity block
    and the parity of classes without an item are unchanged;
  * every lost block still holds GARBAGE byte for byte;
  * after xec_repair (host form, same bitmap) the data equals the patched data
    everywhere and the parity equals oracle.encode_batch of it.  (Where the
    pattern itself is one xec_repair refuses -- a member and the parity of one
    class lost -- the refusal is asserted instead.)
The expectation never comes from the library.  d_new bytes the call must not
read are 0xA5 (test_gpu_update_range's host_new / device_new).

Digests follow test_gpu_update_range's sentinel scheme: the slots the call may
touch (written blocks, the lost one included, and the parity blocks of delta
and rebuild-write classes) and the parity slots of data-only classes start as
the digests of the pre-loss blocks, every other slot as a sentinel; afterwards
a touched slot equals xec.digest_host of the block the repair will produce and
every other slot is unchanged.
"""
from __future__ import annotations

import numpy as np
import pytest

from arena import Arena
from test_gpu_repair import Case, set_shape
from test_gpu_update import assert_state, items_of
from test_gpu_update_range import (as_u64, device_new, full_slots, host_new, locate_all,
                                   ranges_of, run_range, sentinel, true_digests)

pytestmark = pytest.mark.gpu

KM = [(3, 3), (6, 3), (8, 1), (9, 1), (66, 2)]  # member counts 1, 2, 8, 9, 33
BS = [256, 1280, 4352]
S3 = 3
ENTRIES = ["host", "device"]
GARBAGE = 0xC3
PATTERNS = ["null", "ones", "parity", "lost_alone", "lost_between", "unwritten_lost",
            "unwritten_and_parity", "mixed"]
LAUNCHES = [dict(block_threads=256), dict(unroll=2), dict(cache_policy=2), dict(max_grid=2),
            dict(rotation=3)]


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def tiling_diagnostics_left_at_zero():
    """The cases here end with an xec_repair or an xec_update_range of their
    own; a call with nothing to do puts those calls' *_tiling_used back to 0,
    which the ABI tests that run later in the same process ask of the main
    thread."""
    yield
    import xec
    xec.repair(0, 0, 0, 256, 1, 1, None, None)
    xec.update_range(0, 0, 0, 0, 256, 1, 1, None, 0, 0, 16)
    assert xec.repair_tiling_used() == 0 and xec.update_tiling_used() == 0


# ---- loss patterns ---------------------------------------------------------------------
def pattern(kind, S, k, m):
    """(bitmap or None, sorted written (stripe, block) pairs, repairable).  The
    classes named in the comments are (stripe, class)."""
    nm = k // m
    bm = np.ones((S, k + m), np.uint8)
    last = (nm - 1) * m
    mid = (nm // 2) * m
    # a base set every pattern shares: a block of stripe 0 and one of the last stripe
    w = {(0, k - 1), (S - 1, 0)}
    if kind in ("null", "ones"):
        w |= {(1, 0), (1, last), (1, min(1, k - 1))}
        return (None if kind == "null" else bm), sorted(w), True
    if kind == "parity":  # (1, 0) data-only: every member written where there are few
        w |= {(1, r * m) for r in range(min(nm, 3))}
        bm[1, k] = 0
        return bm, sorted(w), True
    if kind == "lost_alone":  # (1, 0) rebuild-write, W = {x}
        w |= {(1, mid)} | ({(1, 1)} if m > 1 else set())
        bm[1, mid] = 0
        return bm, sorted(w), True
    if kind == "lost_between":  # (1, 0) rebuild-write, a write before and one after x
        w |= {(1, 0), (1, mid), (1, last)} | ({(1, 1), (1, m + 1)} if m > 1 and nm > 1 else set())
        bm[1, mid] = 0
        return bm, sorted(w), True
    if kind == "unwritten_lost":  # (1, 0) delta beside a lost member nobody writes
        w |= {(1, 0)}
        if nm > 1:
            bm[1, last] = 0
        else:
            bm[1, 1 % k] = 0  # one member per class: a block of another class
            w.discard((1, 1 % k))
        return bm, sorted(w), True
    if kind == "unwritten_and_parity":  # (1, 0) data-only although xec_repair refuses the batch
        w |= {(1, 0)}
        bm[1, k] = 0
        if nm > 1:
            bm[1, last] = 0
        return bm, sorted(w), nm == 1
    assert kind == "mixed"
    # stripe 0: class 0 delta, the last class data-only; stripe 1: class 0
    # rebuild-write, the last class delta beside an unwritten loss; stripe 2:
    # class 0 data-only, the last class rebuild-write (one class: stripes only)
    j = m - 1
    w = {(0, 0), (0, last), (1, 0), (1, mid), (2, 0), (2, mid)}
    bm[1, mid] = 0
    bm[2, k] = 0
    if m > 1:
        w |= {(0, j), (1, j), (2, j + mid)}
        bm[0, k + j] = 0
        if nm > 1:
            bm[1, j + last] = 0
        bm[2, j + mid] = 0
    return bm, sorted(w), True


def modes_of(c: Case, bm, blocks):
    """{(stripe, class): 'delta' | 'data' | 'rebuild'} of the classes with an item."""
    out = {}
    for cs, i in blocks:
        j = i % c.m
        if bm is not None and bm[cs, c.k + j] == 0:
            out[(cs, j)] = "data"
        elif bm is not None and bm[cs, i] == 0:
            out[(cs, j)] = "rebuild"
        else:
            out.setdefault((cs, j), "delta")
    return out


def model(oracle, c: Case, ref_d, ref_p, bm, blocks, fresh, off, ln):
    """(device data, device parity, final data, final parity): the state the
    write must leave -- GARBAGE in the lost blocks -- and the state after the
    repair."""
    S, k, m, bs = c.S, c.k, c.m, c.bs
    fin_d = oracle.aligned(S * k * bs)
    fin_d[:] = ref_d
    v = fin_d.reshape(S, k, bs)
    for t, (cs, i) in enumerate(blocks):
        v[cs, i, off:off + ln] = fresh[t]
    fin_p = oracle.aligned(S * m * bs)
    assert oracle.encode_batch(fin_d, fin_p, S, bs, k, m) == 0
    dev_d = fin_d.copy().reshape(S, k, bs)
    dev_p = ref_p.copy().reshape(S, m, bs)
    enc = fin_p.reshape(S, m, bs)
    for (cs, j), mode in modes_of(c, bm, blocks).items():
        if mode != "data":
            dev_p[cs, j, off:off + ln] = enc[cs, j, off:off + ln]
    if bm is not None:
        lost = bm.reshape(S, k + m) == 0
        dev_d[lost[:, :k]] = GARBAGE
        dev_p[lost[:, k:]] = GARBAGE
    return dev_d.reshape(-1), dev_p.reshape(-1), fin_d, fin_p


def touched_slots(c: Case, bm, blocks):
    row = c.k + c.m
    out = {cs * row + i for cs, i in blocks}
    out |= {cs * row + c.k + j for (cs, j), mode in modes_of(c, bm, blocks).items()
            if mode != "data"}
    return sorted(out)


def stale_parity_slots(c: Case, bm, blocks):
    row = c.k + c.m
    return sorted(cs * row + c.k + j for (cs, j), mode in modes_of(c, bm, blocks).items()
                  if mode == "data")


def seed_slots(xec, c: Case, ref_d, ref_p, bm, blocks):
    h = sentinel(c)
    which = touched_slots(c, bm, blocks) + stale_parity_slots(c, bm, blocks)
    for b, v in true_digests(xec, c, ref_d, ref_p, which).items():
        h[b] = np.uint64(v)
    return h, _torch().from_numpy(h.view(np.uint8).copy()).to("cuda")


def want_slots(xec, c: Case, seeded, fin_d, fin_p, bm, blocks):
    want = seeded.copy()
    for b, v in true_digests(xec, c, fin_d, fin_p, touched_slots(c, bm, blocks)).items():
        want[b] = np.uint64(v)
    return want


def run_write(xec, c: Case, bm, blocks, fresh, off, ln, entry, dig=None, scratch=None,
              scratch_bytes=None, stream=None):
    """The call on c's buffers; returns (return value, verdict)."""
    torch = _torch()
    S, k, m, bs = c.S, c.k, c.m, c.bs
    n = len(blocks)
    s = c.b.stream if stream is None else stream
    flat = None if bm is None else np.ascontiguousarray(bm.reshape(-1))
    if entry == "host":
        new = host_new(fresh, n, ln)
        if scratch_bytes is None:
            scratch_bytes = xec.write_scratch_bytes(n)
            scratch = torch.empty(max(scratch_bytes, 4), dtype=torch.uint8, device="cuda")
        st = xec.write(c.d, c.p, new, S, bs, k, m, flat, items_of(blocks), n, off, ln, dig,
                       scratch, scratch_bytes, s)
        torch.cuda.synchronize()
        return st, int(st)
    shadow, mask = device_new(c, blocks, fresh, off, ln)
    d_bm = None if flat is None else torch.from_numpy(flat).to("cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    st = xec.write_device(c.d, c.p, shadow, S, bs, k, m, d_bm, mask, off, ln, dig, status, s)
    torch.cuda.synchronize()
    return st, int(status.item())


def run_repair(xec, c: Case, bm):
    torch = _torch()
    flat = np.ascontiguousarray(bm.reshape(-1))
    scratch = torch.empty(flat.size, dtype=torch.uint8, device="cuda")
    st = xec.repair(c.d, c.p, c.S, c.bs, c.k, c.m, torch.from_numpy(flat).pin_memory(), scratch,
                    c.b.stream)
    torch.cuda.synchronize()
    return st


def check_call(xec, oracle, c: Case, bm, blocks, fresh, off, ln, entry, upkeep, what, exp=None,
               repairable=True):
    """One call from the reference state with the lost blocks garbled: bytes,
    (with upkeep) slots, then the repair."""
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    dev_d, dev_p, fin_d, fin_p = exp if exp is not None else model(oracle, c, ref_d, ref_p, bm,
                                                                   blocks, fresh, off, ln)
    if bm is not None:
        c.garbage(bm, GARBAGE)
    dig = seeded = None
    if upkeep:
        seeded, dig = seed_slots(xec, c, ref_d, ref_p, bm, blocks)
    assert run_write(xec, c, bm, blocks, fresh, off, ln, entry, dig) == (xec.Status.SUCCESS, 0), what
    assert_state(c, dev_d, dev_p, what)
    if upkeep:
        want = want_slots(xec, c, seeded, fin_d, fin_p, bm, blocks)
        bad = np.flatnonzero(as_u64(dig) != want)
        assert bad.size == 0, f"{what}: slots {bad[:8].tolist()}"
    if bm is None:
        assert_state(c, fin_d, fin_p, what)
        return
    if not repairable:
        assert run_repair(xec, c, bm) == xec.Status.DECODE_FAILURE, what
        return
    assert run_repair(xec, c, bm) == xec.Status.SUCCESS, what
    assert_state(c, fin_d, fin_p, f"{what}, after the repair")


# --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_write_modes_bit_exact(gpu, oracle, k, m, bs):
    rng = np.random.default_rng(k * 1000 + m * 10 + bs)
    S = S3
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    for off, ln in ranges_of(bs):
        for kind in PATTERNS:
            bm, blocks, repairable = pattern(kind, S, k, m)
            fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
            exp = model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
            for entry in ENTRIES:
                for upkeep in (False, True):
                    what = f"{entry} '{kind}' [{off},+{ln}) upkeep={upkeep}"
                    try:
                        check_call(gpu, oracle, c, bm, blocks, fresh, off, ln, entry, upkeep, what,
                                   exp, repairable)
                        assert gpu.write_tiling_used() == (4 if entry == "host" else 2), what
                    finally:
                        c.restore()


def test_patterns_cover_the_three_modes():
    """The patterns are what their names say (no device needed, but it guards
    the cases above)."""
    import types
    for k, m in KM:
        c = types.SimpleNamespace(S=S3, k=k, m=m)
        nm = k // m
        seen = set()
        for kind in PATTERNS:
            bm, blocks, _ = pattern(kind, S3, k, m)
            assert blocks == sorted(set(blocks)) and all(i < k for _, i in blocks)
            md = modes_of(c, bm, blocks)
            seen |= set(md.values())
            if kind == "lost_between" and nm >= 3:
                x = (nm // 2) * m
                cls = [i for cs, i in blocks if cs == 1 and i % m == 0]
                assert cls.index(x) not in (0, len(cls) - 1) and md[(1, 0)] == "rebuild"
            if kind == "unwritten_and_parity":
                assert md[(1, 0)] == "data"
            if kind == "mixed":
                assert set(md.values()) == {"delta", "data", "rebuild"}
                if m > 1:
                    assert len({md[(cs, j)] for (cs, j) in md if cs == 0}) > 1
        assert seen == {"delta", "data", "rebuild"}


@pytest.mark.parametrize("entry", ENTRIES)
def test_everything_present_is_update_range(gpu, oracle, entry):
    """With everything present the data, parity and slots are those
    xec_update_range leaves on a second copy."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 4352
    off, ln = 1008, 2064
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(3)
    _, blocks, _ = pattern("ones", S, k, m)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    try:
        for upkeep in (False, True):
            dig_a = seed_slots(gpu, c, ref_d, ref_p, None, blocks)[1] if upkeep else None
            dig_b = dig_a.clone() if upkeep else None
            assert run_range(gpu, c, blocks, fresh, off, ln, entry, dig_a) == gpu.Status.SUCCESS
            d_a, p_a = c.d.clone(), c.p.clone()
            c.restore()
            for bm in (None, np.ones((S, k + m), np.uint8)):
                dig = dig_b.clone() if upkeep else None
                assert run_write(gpu, c, bm, blocks, fresh, off, ln, entry, dig) == (0, 0)
                assert torch.equal(c.d, d_a) and torch.equal(c.p, p_a), (entry, upkeep)
                if upkeep:
                    assert torch.equal(dig, dig_a)
                c.restore()
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_locate_counts_the_data_only_parity_blocks(gpu, oracle, entry):
    """Slots = the digests of the pre-loss blocks; xec_write, xec_repair, a
    full xec_locate: exactly the parity blocks of the data-only classes differ,
    and none after xec_digest(select) of those."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    off, ln = 1008, 48
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(12)
    bm, blocks, _ = pattern("mixed", S, k, m)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    _, _, fin_d, fin_p = model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
    stale = stale_parity_slots(c, bm, blocks)
    assert stale
    _, dig = full_slots(gpu, c, ref_d, ref_p)
    try:
        c.garbage(bm, GARBAGE)
        assert run_write(gpu, c, bm, blocks, fresh, off, ln, entry, dig) == (0, 0)
        assert run_repair(gpu, c, bm) == gpu.Status.SUCCESS
        assert_state(c, fin_d, fin_p, "after the repair")
        want = true_digests(gpu, c, fin_d, fin_p)
        got = as_u64(dig)
        wrong = [b for b in range(S * (k + m)) if int(got[b]) != want[b]]
        assert wrong == stale
        assert locate_all(gpu, c, dig) == len(stale)
        select = np.zeros(S * (k + m), np.uint8)
        select[stale] = 1
        assert gpu.digest(c.d, c.p, S, bs, k, m, dig, torch.from_numpy(select).to("cuda"),
                          c.b.stream) == gpu.Status.SUCCESS
        assert locate_all(gpu, c, dig) == 0
    finally:
        c.restore()


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_unservable_write_changes_nothing(gpu, oracle, entry):
    """A written lost member whose class lost a second block -- another member,
    or the parity: DECODE_FAILURE / *d_status == 4, and no byte changes."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    off, ln = 1008, 48
    c = Case.get(gpu, oracle, S, k, m, bs)
    rng = np.random.default_rng(13)
    blocks = [(0, 1), (1, 0), (1, 4), (2, 5)]
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    try:
        for second in (3, k + 0):  # the other member of class 0; its parity
            bm = np.ones((S, k + m), np.uint8)
            bm[1, 0] = bm[1, second] = 0
            c.garbage(bm, GARBAGE)
            d0, p0 = c.d.clone(), c.p.clone()
            dig = torch.full((8 * S * (k + m),), 0x5A, dtype=torch.uint8, device="cuda")
            st, verdict = run_write(gpu, c, bm, blocks, fresh, off, ln, entry, dig)
            if entry == "host":
                assert st == gpu.Status.DECODE_FAILURE and gpu.write_tiling_used() == 0
            else:
                assert st == gpu.Status.SUCCESS and verdict == 4
            assert torch.equal(c.d, d0) and torch.equal(c.p, p0), second
            assert int((dig != 0x5A).sum()) == 0
            # the same loss with the write aimed at a present block of another class: taken
            ok = [(0, 1), (1, 4), (2, 5)]
            assert run_write(gpu, c, bm, ok, fresh[:3], off, ln, entry, None) == (0, 0)
            c.restore()
    finally:
        c.restore()


# ---- launch shapes, list capacities ---------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", LAUNCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_launch_shapes_identical(gpu, oracle, shape, entry):
    """block_threads 256, unroll 2, the default cache policy and a grid of 2
    workgroups give the same bytes and slots; rotation 3 changes nothing."""
    for k, m, bs, ranges in ((6, 3, 1280, [(1008, 48), (16, 1248)]),
                             (9, 1, 4352, [(1008, 2064), (4336, 16)])):
        c = Case.get(gpu, oracle, S3, k, m, bs)
        rng = np.random.default_rng(41)
        bm, blocks, _ = pattern("mixed", S3, k, m)
        try:
            set_shape(gpu, **shape)
            for off, ln in ranges:
                fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
                for upkeep in (False, True):
                    check_call(gpu, oracle, c, bm, blocks, fresh, off, ln, entry, upkeep,
                               f"{shape} {entry} {k}+{m} [{off},+{ln}) upkeep={upkeep}")
                    c.restore()
        finally:
            set_shape(gpu)
            c.restore()


@pytest.mark.parametrize("n", [64, 65, 256, 257, 1024, 1025])
def test_list_capacities_host_form(gpu, oracle, n):
    """1,100 stripes of 4+2 x 256; a lost written member in every 7th stripe, a
    lost parity in every 5th.  Up to 1,024 items travel in the kernel arguments,
    1,025 through the scratch, which must be there, aligned and large enough."""
    torch = _torch()
    S, k, m, bs = 1100, 4, 2, 256
    off, ln = 112, 32
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(n)
    blocks = [divmod(int(q), k) for q in np.sort(rng.permutation(S * k)[:n])]
    bm = np.ones((S, k + m), np.uint8)
    for cs, i in blocks:
        if cs % 7 == 0 and bm[cs, i % m::m].all():
            bm[cs, i] = 0                      # a written member, alone in its class
        elif cs % 5 == 0 and bm[cs, i % m::m].all():
            bm[cs, k + i % m] = 0              # the parity of a written class
    md = modes_of(c, bm, blocks)
    assert {"delta", "data", "rebuild"} == set(md.values())
    st, n_rebuild, n_data = gpu.check_write_items(bm.reshape(-1), S, k, m, items_of(blocks), n)
    assert st == gpu.Status.SUCCESS and n_rebuild > 0 and n_data > 0
    fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
    exp = model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
    St = gpu.Status
    try:
        if n > 1024:
            need = gpu.write_scratch_bytes(n)
            assert need == 4 * (n + (n + 15) // 16)
            short = torch.empty(need + 8, dtype=torch.uint8, device="cuda")
            assert run_write(gpu, c, bm, blocks, fresh, off, ln, "host", None, None, 0)[0] == St.INVALID_SIZE
            assert run_write(gpu, c, bm, blocks, fresh, off, ln, "host", None, short,
                             need - 1)[0] == St.INVALID_SIZE
            assert run_write(gpu, c, bm, blocks, fresh, off, ln, "host", None, short.data_ptr() + 2,
                             need)[0] == St.INVALID_ALIGNMENT
            assert gpu.write_tiling_used() == 0
            c.assert_exact("after rejected scratch arguments")
        for upkeep in (False, True):
            check_call(gpu, oracle, c, bm, blocks, fresh, off, ln, "host", upkeep, f"a list of {n}",
                       exp)
            c.restore()
            # (check_call's repair is the last library call; the tiling is asked of a bare call)
        assert run_write(gpu, c, bm, blocks, fresh, off, ln, "host")[0] == St.SUCCESS
        assert gpu.write_tiling_used() == (4 if n <= 1024 else 3)
    finally:
        c.restore()


# ---- rejections and minimum alignment, in a guarded arena ----------------------------
def arena_for(gpu, oracle, S, k, m, bs, n_new, ln):
    """data, parity at 64; new and shadow at 16; digests at 8; scratch and status
    at 4; mask and bitmap at 1 -- each at exactly its minimum alignment.  Data,
    parity and digests are carved block by block and slot by slot (flush), so a
    check can name the very blocks and slots a call may write."""
    import copy
    row = k + m
    sizes = ([(bs, 64)] * (S * row) + [(max(n_new * ln, 16), 16), (S * k * bs, 16)] +
             [(8, 8)] * (S * row) + [(4400 + 4 * 69, 4), (4, 4), (S * k, 1), (S * row, 1)])
    edge = max(bs, 4096)
    a = Arena(Arena.room(sizes, edge), "cuda", edge)
    for t in range(S * k):
        a.carve(f"d{t // k}.{t % k}", bs, 64, **({} if t == 0 else dict(gap=0)))
    for t in range(S * m):
        a.carve(f"p{t // m}.{t % m}", bs, 64, **({} if t == 0 else dict(gap=0)))
    a.carve("new", max(n_new * ln, 16), 16)
    a.carve("shadow", S * k * bs, 16)
    for t in range(S * row):
        a.carve(f"s{t}", 8, 8, **({} if t == 0 else dict(gap=0)))
    a.carve("scratch", 4400 + 4 * 69, 4)
    a.carve("status", 4, 4)
    a.carve("mask", S * k, 1)
    a.carve("bitmap", S * row, 1)
    c = copy.copy(Case.get(gpu, oracle, S, k, m, bs))
    d0, p0, s0 = a.regions["d0.0"][0], a.regions["p0.0"][0], a.regions["s0"][0]
    c.d, c.p = a.buf[d0:d0 + S * k * bs], a.buf[p0:p0 + S * m * bs]
    dig = a.buf[s0:s0 + 8 * S * row]
    c.d.copy_(c.ref_d)
    c.p.copy_(c.ref_p)
    a.adopt([n for n in a.regions if n[0] in "dp" and n[1].isdigit()])
    assert c.d.data_ptr() % 128 == 64 and a.ptr("new") % 32 == 16 and a.ptr("shadow") % 32 == 16
    assert dig.data_ptr() % 16 == 8 and a.ptr("status") % 8 == 4 and a.ptr("bitmap") % 2 == 1
    return a, c, dig


def block_regions(c: Case):
    return ([f"d{cs}.{i}" for cs in range(c.S) for i in range(c.k)] +
            [f"p{cs}.{j}" for cs in range(c.S) for j in range(c.m)])


@pytest.mark.parametrize("entry", ENTRIES)
def test_minimum_alignment_in_a_guarded_arena(gpu, oracle, entry):
    """All three modes with upkeep at (6,3) x 1280, every buffer at its least
    alignment.  Writable: the present written blocks, the parity blocks of delta
    and rebuild-write classes, the touched slots and d_status -- so a lost block,
    a lost parity block and its slot are proven never stored to."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    row = k + m
    rng = np.random.default_rng(77)
    bm, blocks, _ = pattern("mixed", S, k, m)
    n = len(blocks)
    ranges = [(bs - 48, 48), (1008, bs - 1008)]
    a, c, dig = arena_for(gpu, oracle, S, k, m, bs, n, max(l for _, l in ranges))
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    St, s = gpu.Status, c.b.stream
    a.put("bitmap", bm)
    md = modes_of(c, bm, blocks)
    writable = [f"d{cs}.{i}" for cs, i in blocks if bm[cs, i] != 0]
    writable += [f"p{cs}.{j}" for (cs, j), mode in md.items() if mode != "data"]
    slots = touched_slots(c, bm, blocks)
    for off, ln in ranges:
        fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
        dev_d, dev_p, fin_d, fin_p = model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
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
        for upkeep in (False, True):
            what = f"{entry} [{off},+{ln}) upkeep={upkeep}"
            c.d.copy_(c.ref_d)
            c.p.copy_(c.ref_p)
            c.garbage(bm, GARBAGE)
            seeded, _ = seed_slots(gpu, c, ref_d, ref_p, bm, blocks)
            dig.copy_(torch.from_numpy(seeded.view(np.uint8).copy()).to("cuda"))
            a.fill("status", 0x4D)
            a.adopt(block_regions(c) + [f"s{t}" for t in range(S * row)])
            d_dig = dig if upkeep else None
            if entry == "host":
                st = gpu.write(c.d, c.p, a["new"], S, bs, k, m, bm.reshape(-1), items_of(blocks), n,
                               off, ln, d_dig, None, 0, s)
                may = list(writable)
            else:
                st = gpu.write_device(c.d, c.p, a["shadow"], S, bs, k, m, a["bitmap"], a["mask"],
                                      off, ln, d_dig, a["status"], s)
                may = writable + ["status"]
            torch.cuda.synchronize()
            assert st == St.SUCCESS, what
            if entry == "device":
                assert a["status"].view(torch.int32).item() == 0
            assert_state(c, dev_d, dev_p, what)
            if upkeep:
                want = want_slots(gpu, c, seeded, fin_d, fin_p, bm, blocks)
                assert np.array_equal(as_u64(dig), want), what
                may += [f"s{t}" for t in slots]
            a.check(writable=may, what=what)


def test_rejections_in_order_change_nothing(gpu, oracle):
    """Every rejection of the check list returns its status, an earlier check
    wins over a later one, and nothing in the arena changes."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    off, ln = 1008, 48
    blocks = [(0, 1), (1, 0), (1, 5)]
    n = len(blocks)
    a, c, dig = arena_for(gpu, oracle, S, k, m, bs, n, ln)
    St, s = gpu.Status, c.b.stream
    a.fill("new", 0x5A)
    a.fill("shadow", 0x5A)
    a.fill("mask", 1)
    a.fill("bitmap", 1)
    a.fill("status", 0x4D)
    ok = items_of(blocks)
    NEW, SH, DIG, D, P = a.ptr("new"), a.ptr("shadow"), dig.data_ptr(), c.d.data_ptr(), c.p.data_ptr()
    STAT, BM = a.ptr("status"), a.ptr("bitmap")
    nd, npar = S * k * bs, S * m * bs
    h_bm = np.ones(S * (k + m), np.uint8)
    lost2 = h_bm.copy().reshape(S, k + m)
    lost2[1, 0] = lost2[1, 3] = 0  # item (1, 0) is lost with the other member of its class
    lost2 = lost2.reshape(-1)

    def host(d=D, new=NEW, S_=S, bs_=bs, k_=k, m_=m, bm=h_bm, it=ok, n_=n, off_=off, ln_=ln, dg=DIG,
             scr=None, scr_bytes=0):
        st = gpu.write(d, P, new, S_, bs_, k_, m_, bm, it, n_, off_, ln_, dg, scr, scr_bytes, s)
        assert gpu.write_tiling_used() == 0
        return st

    def dev(d=D, new=SH, S_=S, bs_=bs, k_=k, m_=m, bm=BM, mask=a.ptr("mask"), off_=off, ln_=ln,
            dg=DIG, stat=STAT):
        st = gpu.write_device(d, P, new, S_, bs_, k_, m_, bm, mask, off_, ln_, dg, stat, s)
        assert gpu.write_tiling_used() == 0
        return st

    bad_items = np.array([ok[1], ok[0], ok[2]], dtype=np.uint32)
    # 2. xec_check_args, ahead of everything behind it
    assert host(d=D + 16, off_=8, new=None) == St.INVALID_ALIGNMENT
    assert dev(d=D + 16, off_=8, new=None, stat=None) == St.INVALID_ALIGNMENT
    assert host(bs_=100) == St.INVALID_SIZE and dev(bs_=100) == St.INVALID_SIZE
    assert host(k_=5) == St.INVALID_COUNTS and dev(k_=5) == St.INVALID_COUNTS
    # 3. nothing to do is a success even with arguments a later check rejects
    assert host(n_=0, off_=8, new=None, dg=DIG + 4, bm=lost2) == St.SUCCESS
    assert host(S_=0, off_=8, new=None, dg=DIG + 4) == St.SUCCESS
    assert dev(S_=0, off_=8, new=None, mask=None, stat=None) == St.SUCCESS
    # 4. the packing (host form only), ahead of the range
    assert host(k_=264, m_=4, off_=8) == St.INVALID_SIZE
    assert host(S_=(1 << 24) + 1, new=NEW + 8) == St.INVALID_SIZE
    # 5. the range, ahead of NULL pointers and alignment
    for o, l in ((off, 0), (8, 32), (16, 24), (bs - 16, 32), (bs + 16, 16), (bs, 16)):
        assert host(off_=o, ln_=l, new=NEW + 8) == St.INVALID_SIZE, (o, l)
        assert dev(off_=o, ln_=l, new=SH + 8, stat=STAT + 2) == St.INVALID_SIZE, (o, l)
    # 6. NULL pointers, ahead of alignment
    assert host(new=None, dg=DIG + 4) == St.INVALID_SIZE
    assert host(it=None, new=NEW + 8) == St.INVALID_SIZE
    assert dev(new=None, dg=DIG + 4) == St.INVALID_SIZE
    assert dev(mask=None, new=SH + 8) == St.INVALID_SIZE
    # 7. alignment, ahead of the overlaps
    assert host(new=D + 8) == St.INVALID_ALIGNMENT and dev(new=D + 8) == St.INVALID_ALIGNMENT
    assert host(dg=D + 4) == St.INVALID_ALIGNMENT and dev(dg=P + 4) == St.INVALID_ALIGNMENT
    # 8. the overlaps, ahead of the item rules (host) and of d_status (device)
    assert host(new=D + 16, it=bad_items) == St.INVALID_SIZE
    assert host(new=P + npar - 16, it=bad_items) == St.INVALID_SIZE
    assert host(new=D - n * ln + 16) == St.INVALID_SIZE
    assert dev(new=D, stat=None) == St.INVALID_SIZE and dev(new=P - nd + 16) == St.INVALID_SIZE
    assert host(dg=D + nd - 8) == St.INVALID_SIZE and dev(dg=P) == St.INVALID_SIZE
    assert host(dg=NEW + n * ln - 8) == St.INVALID_SIZE
    assert dev(dg=SH + 8, stat=STAT + 2) == St.INVALID_SIZE
    # device form, last: d_status NULL or not 4-byte aligned
    assert dev(stat=None) == St.INVALID_ALIGNMENT and dev(stat=STAT + 2) == St.INVALID_ALIGNMENT
    # 9. the item rules, ahead of servability -- anywhere in the list
    assert host(it=bad_items, bm=lost2) == St.INVALID_COUNTS                             # unsorted
    assert host(it=np.array([ok[0], ok[1], ok[1]], np.uint32), bm=lost2) == St.INVALID_COUNTS
    assert host(it=np.array([ok[0], ok[1], (1 << 8) | k], np.uint32), bm=lost2) == St.INVALID_COUNTS
    assert host(it=np.array([ok[0], ok[1], (S << 8)], np.uint32), bm=lost2) == St.INVALID_COUNTS
    # 10. servability, ahead of the scratch
    assert host(bm=lost2) == St.DECODE_FAILURE
    # 11. the scratch rules past 1,024 items (buffers of their own: the arena's
    # `new` is too short; the call is rejected before any read)
    many = np.arange(1100, dtype=np.uint32)
    many = ((many // k) << 8 | (many % k)).astype(np.uint32)
    S_big = 1100 // k + 1
    big = torch.full((1100 * ln,), 0x5A, dtype=torch.uint8, device="cuda")
    bigd = torch.zeros(S_big * k * bs, dtype=torch.uint8, device="cuda")
    bigp = torch.zeros(S_big * m * bs, dtype=torch.uint8, device="cuda")
    bigdig = torch.zeros(8 * S_big * (k + m), dtype=torch.uint8, device="cuda")
    big_bm = np.ones(S_big * (k + m), np.uint8)
    bad_bm = big_bm.copy()
    bad_bm[0] = bad_bm[3] = 0
    need = gpu.write_scratch_bytes(1100)
    assert need == 4 * (1100 + 69) and a.size("scratch") == need

    def long(scr, scr_bytes, bm=big_bm):
        st = gpu.write(bigd, bigp, big, S_big, bs, k, m, bm, many, 1100, off, ln, bigdig, scr,
                       scr_bytes, s)
        assert gpu.write_tiling_used() == 0
        return st

    assert long(a.ptr("scratch") + 2, need, bad_bm) == St.DECODE_FAILURE  # 10 ahead of 11
    assert long(a.ptr("scratch") + 2, need) == St.INVALID_ALIGNMENT
    assert long(None, need) == St.INVALID_SIZE
    assert long(a.ptr("scratch"), need - 1) == St.INVALID_SIZE
    torch.cuda.synchronize()
    assert int(bigd.count_nonzero()) == 0 and int(bigp.count_nonzero()) == 0
    assert int(bigdig.count_nonzero()) == 0
    a.check(writable=[], what="after every rejection")
    c.assert_exact("after every rejection")


# ---- capture, kernel events ------------------------------------------------------------
def test_host_form_refuses_graph_capture(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    new = torch.full((2 * 48,), 0x3C, dtype=torch.uint8, device="cuda")
    dig = torch.full((8 * S * (k + m),), 0xA5, dtype=torch.uint8, device="cuda")
    items = items_of([(0, 1), (2, 5)])
    bm = np.ones(S * (k + m), np.uint8)
    bm[1] = 0  # block (0, 1): a rebuild-write
    St = gpu.Status
    try:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.write(c.d, c.p, new, S, bs, k, m, bm, items, 2, 1008, 48, dig, None, 0,
                             cs) == St.DEVICE_ERROR
            assert gpu.write_tiling_used() == 0
            assert gpu.write(c.d, c.p, new, S, bs, k, m, bm, items, 0, 1008, 48, dig, None, 0,
                             cs) == St.SUCCESS
        g.replay()  # an empty graph
        torch.cuda.synchronize()
        del g
        c.assert_exact("after a refused capture")
        assert int((dig != 0xA5).sum()) == 0
    finally:
        c.restore()


def test_graph_of_write_device(gpu, oracle):
    """The device form with upkeep, captured alone -- bitmap, mask, shadow,
    slots and the expected state on the device before the capture -- and
    replayed once: exact."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 4352
    off, ln = 1008, 2064
    c = Case.get(gpu, oracle, S, k, m, bs)
    ref_d, ref_p = c.ref_d.cpu().numpy(), c.ref_p.cpu().numpy()
    rng = np.random.default_rng(23)
    bm, blocks, _ = pattern("mixed", S, k, m)
    fresh = rng.integers(0, 256, size=(len(blocks), ln), dtype=np.uint8)
    dev_d, dev_p, fin_d, fin_p = model(oracle, c, ref_d, ref_p, bm, blocks, fresh, off, ln)
    seeded, dig = seed_slots(gpu, c, ref_d, ref_p, bm, blocks)
    want = want_slots(gpu, c, seeded, fin_d, fin_p, bm, blocks)
    shadow, mask = device_new(c, blocks, fresh, off, ln)
    d_bm = torch.from_numpy(bm.reshape(-1).copy()).to("cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    want_d, want_p = torch.from_numpy(dev_d.copy()).to("cuda"), torch.from_numpy(dev_p.copy()).to("cuda")
    try:
        c.garbage(bm, GARBAGE)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            cs = torch.cuda.current_stream()
            assert gpu.write_device(c.d, c.p, shadow, S, bs, k, m, d_bm, mask, off, ln, dig, status,
                                    cs) == gpu.Status.SUCCESS
            assert gpu.write_tiling_used() == 2
        torch.cuda.synchronize()
        assert int(status.item()) == 77  # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        assert torch.equal(c.d, want_d) and torch.equal(c.p, want_p)
        assert np.array_equal(as_u64(dig), want)
        del g
    finally:
        c.restore()


def test_kernel_events_cover_both_calls(gpu, oracle):
    """An armed pair is consumed by each call and times the write kernel: a
    positive interval."""
    torch = _torch()
    S, k, m, bs = 3, 6, 3, 4352
    off, ln = 1008, 2064
    c = Case.get(gpu, oracle, S, k, m, bs)
    s = c.b.stream
    rng = np.random.default_rng(29)
    bm, blocks, _ = pattern("mixed", S, k, m)
    flat = bm.reshape(-1).copy()
    n = len(blocks)
    fresh = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
    dig = torch.zeros(8 * S * (k + m), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    try:
        for entry in ENTRIES:
            for e in ev:
                e.record(s)  # torch creates the HIP handle at the first record
            torch.cuda.synchronize()
            base = ev[0].elapsed_time(ev[1])
            if entry == "host":
                new = host_new(fresh, n, ln)
                torch.cuda.synchronize()
                assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
                st = gpu.write(c.d, c.p, new, S, bs, k, m, flat, items_of(blocks), n, off, ln, dig,
                               None, 0, s)
            else:
                shadow, mask = device_new(c, blocks, fresh, off, ln)
                d_bm = torch.from_numpy(flat).to("cuda")
                torch.cuda.synchronize()
                assert gpu.set_kernel_events(ev[0], ev[1]) == gpu.Status.SUCCESS
                st = gpu.write_device(c.d, c.p, shadow, S, bs, k, m, d_bm, mask, off, ln, dig,
                                      status, s)
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


def test_past_4_gib(gpu):
    """16+1 x 1 MiB x 257 stripes (tests/test_gpu_read.py's shape): stripe 256
    starts past 4 GiB of data.  A lost written member and a present written one
    in it; the expectation comes from that stripe's blocks alone."""
    torch = _torch()
    S, k, m, bs = 257, 16, 1, 1 << 20
    off, ln = bs - 4096 - 16, 4096
    s = torch.cuda.current_stream()
    d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
    p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
    assert gpu.fill_splitmix64(d, S, k * bs, 4242, s) == 0
    assert gpu.encode(d, p, S, bs, k, m, s) == 0
    torch.cuda.synchronize()
    last = d.view(S, k, bs)[256].cpu().numpy()
    par = np.bitwise_xor.reduce(last, axis=0)
    assert np.array_equal(p.view(S, bs)[256].cpu().numpy(), par)
    rng = np.random.default_rng(4)
    fresh = rng.integers(0, 256, size=(2, ln), dtype=np.uint8)
    bm = np.ones((S, k + m), np.uint8)
    bm[256, 5] = 0
    items = np.array([(256 << 8) | 5, (256 << 8) | 15], np.uint32)
    want = last.copy()
    want[5, off:off + ln] = fresh[0]
    want[15, off:off + ln] = fresh[1]
    want_par = np.bitwise_xor.reduce(want, axis=0)
    d.view(S, k, bs)[256, 5] = GARBAGE
    first_p = p.view(S, bs)[0].clone()
    new = host_new(fresh, 2, ln)
    assert gpu.write(d, p, new, S, bs, k, m, bm.reshape(-1), items, 2, off, ln, None, None, 0,
                     s) == gpu.Status.SUCCESS
    torch.cuda.synchronize()
    got = d.view(S, k, bs)[256].cpu().numpy()
    assert bool((got[5] == GARBAGE).all())  # the lost block was not written
    keep = [i for i in range(k) if i != 5]
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(p.view(S, bs)[256].cpu().numpy(), want_par)
    assert torch.equal(p.view(S, bs)[0], first_p)  # nothing wrapped round to the first stripe
    del d, p
    torch.cuda.empty_cache()
