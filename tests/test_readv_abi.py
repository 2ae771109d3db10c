"""Vectored read without a device: the binding, xec_iov's layout, the scratch
and work sizes, and xec_check_readv -- the host plan xec_readv runs -- against
a numpy restatement of the rule (CPU only).

An entry (item c << 8 | i, offset, len) has a valid range if len > 0, offset
and len are multiples of 16 and offset + len <= bs; it is servable if its block
is present (bitmap byte != 0, or no bitmap), or lost with every other block of
its class present.  A broken range anywhere outranks an entry out of range,
which outranks an entry that is not servable (steps 7, 9 and 10 of xec_readv).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import xec

NEW = ("xec_readv", "xec_readv_scratch_bytes", "xec_readv_device", "xec_readv_device_work_bytes",
       "xec_check_readv", "xec_readv_tiling_used")
St = xec.Status
OK, SIZE, COUNTS, FAIL = St.SUCCESS, St.INVALID_SIZE, St.INVALID_COUNTS, St.DECODE_FAILURE


def iov(entries):
    a = np.zeros(len(entries), dtype=xec.IOV)
    for t, (item, offset, length) in enumerate(entries):
        a[t] = (item, offset, length)
    return a


def rule(bm, S, bs, k, m, entries):
    """(status, n_lost, total_bytes) by the rule above, one entry at a time."""
    if any(ln == 0 or off % 16 or ln % 16 or off + ln > bs for _, off, ln in entries):
        return SIZE, 0, 0
    if any((it >> 8) >= S or (it & 0xFF) >= k + m for it, _, _ in entries):
        return COUNTS, 0, 0
    n_lost = 0
    for it, _, _ in entries:
        c, i = it >> 8, it & 0xFF
        if bm is None or bm[c, i] != 0:
            continue
        j = i % m if i < k else i - k
        cls = [l for l in range(j, k, m)] + [k + j]
        if any(bm[c, l] == 0 for l in cls if l != i):
            return FAIL, 0, 0
        n_lost += 1
    return OK, n_lost, sum(ln for _, _, ln in entries)


def check(bm, S, bs, k, m, entries):
    flat = None if bm is None else np.ascontiguousarray(bm, dtype=np.uint8).reshape(-1)
    return xec.check_readv(flat, S, bs, k, m, iov(entries), len(entries))


@pytest.mark.parametrize("k,m", [(4, 1), (6, 2), (66, 2)])
def test_check_readv_equals_the_rule_on_random_bitmaps(k, m):
    rng = np.random.default_rng(1000 * k + m)
    S, bs = 7, 4352
    seen = set()
    for trial in range(300):
        p_lost = (0.0, 0.02, 0.1, 0.3)[trial % 4]
        bm = (rng.random((S, k + m)) >= p_lost).astype(np.uint8)
        bm[bm != 0] = rng.choice([1, 2, 255], size=int((bm != 0).sum()))
        if trial % 7 == 3:  # a doubly-lost class for certain: a member and its parity
            bm[2, 0] = bm[2, k] = 0
        n = int(rng.integers(2, 40))
        entries = []
        for t in range(n):
            ln = 16 * int(rng.integers(1, bs // 16 + 1))
            off = 16 * int(rng.integers(0, (bs - ln) // 16 + 1))
            entries.append([int(rng.integers(S)) << 8 | int(rng.integers(k + m)), off, ln])  # data and parity
        entries[n // 2][0] = entries[0][0]  # a duplicate, with a range of its own
        if trial % 7 == 3 and trial % 2:
            entries[1][0] = (2 << 8) | 0
        if trial % 11 == 0:  # an entry out of range
            entries[int(rng.integers(n))][0] = (S << 8) | 0 if trial % 2 else ((S - 1) << 8) | (k + m)
        if trial % 13 == 0:  # a bad range
            t = int(rng.integers(n))
            entries[t][1:] = [(8, 16), (0, 0), (0, 24), (bs - 16, 32), (bs, 16)][trial % 5]
        want = rule(bm, S, bs, k, m, entries)
        got = check(bm, S, bs, k, m, entries)
        assert got[0] == want[0], (trial, entries, bm)
        if want[0] == OK:
            assert got[1:] == want[1:], trial
        seen.add((want[0], want[1] > 0))
    assert {(OK, False), (OK, True), (FAIL, False), (COUNTS, False), (SIZE, False)} <= seen


def test_named_cases():
    S, bs, k, m = 3, 4352, 6, 2  # class 0: data 0, 2, 4 and parity 6; class 1: 1, 3, 5 and 7
    bm = np.ones((S, k + m), np.uint8)
    bm[1, 0] = bm[1, 2] = 0  # stripe 1, class 0: doubly lost
    bad_range, far, unserv, fine = [0, 8, 16], [(S << 8), 0, 16], [(1 << 8) | 0, 0, 16], [5, 16, 32]
    # the order 7 -> 9 -> 10, wherever the entries stand in the list
    assert check(bm, S, bs, k, m, [fine, unserv])[0] == FAIL
    assert check(bm, S, bs, k, m, [unserv, fine, far])[0] == COUNTS
    assert check(bm, S, bs, k, m, [far, unserv])[0] == COUNTS
    assert check(bm, S, bs, k, m, [unserv, far, fine, bad_range])[0] == SIZE
    assert check(bm, S, bs, k, m, [bad_range, far, unserv])[0] == SIZE
    # an entry that breaks both its range and its item: the range comes first
    assert check(bm, S, bs, k, m, [[(S << 8), 0, 0]])[0] == SIZE
    # every way to break a range; offset + len is summed in 64 bits
    for off, ln in [(0, 0), (8, 256), (0, 24), (bs - 16, 32), (bs, 16), (bs + 16, 16),
                    (0xFFFFFFF0, 32), (16, 0xFFFFFFF0)]:
        assert check(bm, S, bs, k, m, [fine, [5, off, ln]])[0] == SIZE, (off, ln)
    # the ends of the block are fine
    assert check(bm, S, bs, k, m, [[5, 0, bs], [5, bs - 16, 16], [5, 0, 16]]) == (OK, 0, bs + 32)
    # a present block of a doubly-lost class; an unrecoverable class nobody names
    assert check(bm, S, bs, k, m, [[(1 << 8) | 4, 0, 16], [(1 << 8) | 6, 16, 16]]) == (OK, 0, 32)
    assert check(bm, S, bs, k, m, [[(1 << 8) | 1, 0, 16], [(2 << 8) | 7, 0, 4352]]) == (OK, 0, 4368)
    # singly lost: data, parity, and a repeat counts each time
    bm3 = np.ones((S, k + m), np.uint8)
    bm3[0, 5] = bm3[0, 6] = 0
    assert check(bm3, S, bs, k, m, [[5, 0, 16], [6, 16, 1024], [5, 32, 48], [1, 0, 16]]) == (OK, 3, 1104)
    # a lost block whose class also lost its parity, and that parity
    bm2 = np.ones((S, k + m), np.uint8)
    bm2[2, 3] = bm2[2, 7] = 0
    assert check(bm2, S, bs, k, m, [[(2 << 8) | 3, 0, 16]])[0] == FAIL
    assert check(bm2, S, bs, k, m, [[(2 << 8) | 7, 0, 16]])[0] == FAIL
    # a NULL bitmap: everything is present
    assert check(None, S, bs, k, m, [unserv, [(1 << 8) | 2, 0, 16]]) == (OK, 0, 32)
    assert check(None, S, bs, k, m, [far])[0] == COUNTS
    assert check(None, S, bs, k, m, [bad_range])[0] == SIZE
    # bitmap bytes 2 and 255 are present
    bm4 = np.full((S, k + m), 2, np.uint8)
    bm4[:, 1::2] = 255
    every = [[(c << 8) | i, 0, 16] for c in range(S) for i in range(k + m)]
    assert check(bm4, S, bs, k, m, every) == (OK, 0, 16 * len(every))
    bm4[0, 0] = 0
    assert check(bm4, S, bs, k, m, [[0, 0, 16]]) == (OK, 1, 16)
    # nothing asked; invalid k, m as xec_check_args; a NULL list with entries
    assert check(bm, S, bs, k, m, []) == (OK, 0, 0)
    assert check(bm, S, bs, 6, 4, [fine])[0] == COUNTS
    assert xec.check_readv(None, S, bs, k, m, None, 3)[0] == COUNTS
    # n_lost and total_bytes may be NULL
    one = iov([[5, 0, 16]])
    L = xec.lib()
    assert L.xec_check_readv(bm3.ctypes.data, S, bs, k, m, one.ctypes.data, 1, None, None) == 0
    total = ctypes.c_size_t(0)
    assert L.xec_check_readv(bm3.ctypes.data, S, bs, k, m, one.ctypes.data, 1, None,
                             ctypes.byref(total)) == 0 and total.value == 16


def test_iov_is_twelve_bytes():
    class Iov(ctypes.Structure):
        _fields_ = [("item", ctypes.c_uint32), ("offset", ctypes.c_uint32), ("len", ctypes.c_uint32)]

    assert ctypes.sizeof(Iov) == 12 and ctypes.alignment(Iov) == 4
    assert xec.IOV.itemsize == 12 and xec.IOV.names == ("item", "offset", "len")
    assert [xec.IOV.fields[n][1] for n in xec.IOV.names] == [0, 4, 8]
    # the library reads the same layout: one entry through the ctypes structure
    e = Iov((1 << 8) | 2, 32, 48)
    total = ctypes.c_size_t(0)
    assert xec.lib().xec_check_readv(None, 2, 256, 4, 1, ctypes.addressof(e), 1, None,
                                     ctypes.byref(total)) == 0 and total.value == 48


def test_size_functions_are_monotone():
    prev_s = prev_w = 0
    for n in list(range(0, 200)) + [255, 256, 257, 1023, 1024, 1025, 4096, 1 << 20, (1 << 24) + 5]:
        s, w = xec.readv_scratch_bytes(n), xec.readv_device_work_bytes(n)
        assert s >= prev_s and s % 4 == 0, n
        assert w >= prev_w and w % 8 == 0, n
        if n:
            assert s == 4 * (6 * n + 1 + (n + 31) // 32)  # the header's formula
            assert w == (12 * (n + 1) + 7) // 8 * 8
        prev_s, prev_w = s, w
    assert xec.readv_scratch_bytes(0) == 0 and xec.readv_device_work_bytes(0) == 0


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_readv_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == St.DEVICE_ERROR
    S, k, m, bs = 2, 4, 1, 4096
    NI = St.NOT_INITIALIZED
    ents = iov([[0, 0, 256], [(1 << 8) | 4, 16, 16]])
    bm = np.ones(S * (k + m), np.uint8)
    out, div, dst, dwk = 1 << 24, 1 << 25, 1 << 26, 1 << 27
    assert xec.readv(64, 128, S, bs, k, m, bm, ents, 2, out, 4096) == NI
    assert xec.readv(64, 128, S, bs, k, m, None, ents, 2, out, 4096) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, 1 << 23, div, 2, out, 4096, dwk, 64, dst) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, div, 2, out, 4096, dwk, 64, dst) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    assert xec.readv(65, 128, S, 100, 6, 4, bm, ents, 2, out, 4096) == NI        # xec_check_args
    assert xec.readv(64, 128, 0, bs, k, m, bm, ents, 0, out, 4096) == NI         # nothing to do
    assert xec.readv(64, 128, 1 << 25, bs, 255, 5, bm, ents, 2, out, 4096) == NI  # the packing
    assert xec.readv(64, 128, S, 1 << 32, k, m, bm, ents, 2, out, 4096) == NI
    assert xec.readv(64, 128, S, bs, k, m, bm, None, 2, None, 4096) == NI        # NULL
    assert xec.readv(64, 128, S, bs, k, m, bm, ents, 2, out + 8, 4096) == NI     # alignment
    assert xec.readv(64, 128, S, bs, k, m, bm, iov([[0, 8, 0]]), 1, out, 4096) == NI  # a range
    assert xec.readv(64, 128, S, bs, k, m, bm, ents, 2, out, 16) == NI           # out_bytes
    assert xec.readv(64, 128, S, bs, k, m, bm, ents, 2, 64, 4096) == NI          # overlap
    assert xec.readv(64, 128, S, bs, k, m, bm, iov([[S << 8, 0, 16]]), 1, out, 4096) == NI
    assert xec.readv(64, 128, S, bs, k, m, np.zeros_like(bm), ents, 2, out, 4096) == NI
    many = iov([[0, 0, 16]] * 300)
    assert xec.readv(64, 128, S, bs, k, m, bm, many, 300, out, 1 << 20, None, 0) == NI  # scratch
    assert xec.readv_device(65, 128, S, 100, 6, 4, None, div, 2, out, 4096, dwk, 64, dst) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, div, 2, out, 4096, dwk, 64, None) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, div, 2, out, 4096, dwk, 64, dst + 2) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, None, 2, out, 4096, None, 0, dst) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, div + 2, 2, out, 4096, dwk + 4, 8, dst) == NI
    assert xec.readv_device(64, 128, S, bs, k, m, None, div, 0, out, 4096, dwk, 64, dst) == NI
    assert xec.readv_tiling_used() == 0
    # the host plan needs no initialisation
    assert xec.check_readv(bm, S, bs, k, m, ents, 2) == (OK, 0, 272)


def test_readv_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_readv.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, sz, vp, sz, vp, sz, vp]
    assert list(L.xec_readv_device.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, sz, vp, sz, vp, sz,
                                                 vp, vp]
    assert L.xec_readv.restype is ctypes.c_int and L.xec_readv_device.restype is ctypes.c_int
    for fn in (L.xec_readv_scratch_bytes, L.xec_readv_device_work_bytes):
        assert list(fn.argtypes) == [sz] and fn.restype is sz
    assert list(L.xec_check_readv.argtypes) == [vp, sz, sz, sz, sz, vp, sz, ctypes.POINTER(sz),
                                                ctypes.POINTER(sz)]
    assert L.xec_check_readv.restype is ctypes.c_int
    assert list(L.xec_readv_tiling_used.argtypes) == []
    assert L.xec_readv_tiling_used.restype is ctypes.c_int
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("readv", "readv_device", "readv_scratch_bytes", "readv_device_work_bytes",
                 "check_readv", "readv_tiling_used", "IOV"):
        assert name in xec.__all__ and getattr(xec, name) is not None
