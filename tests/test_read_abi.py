"""Degraded read without a device: the binding, xec_read_scratch_bytes, and
xec_check_read_items -- the host scan xec_read runs -- against a numpy
restatement of the rule (CPU only).

An item c << 8 | i (i in [0, k+m), i >= k parity block i - k) is servable if
its block is present (bitmap byte != 0, or no bitmap), or lost with every other
block of its class present.  Only the classes the items name are looked at.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import xec

NEW = ("xec_read", "xec_read_scratch_bytes", "xec_read_device", "xec_check_read_items",
       "xec_read_tiling_used")
OK, COUNTS, FAIL = xec.Status.SUCCESS, xec.Status.INVALID_COUNTS, xec.Status.DECODE_FAILURE


def rule(bm, S, k, m, items):
    """(status, n_lost) by the rule above, one item at a time."""
    items = [int(x) for x in items]
    if any((it >> 8) >= S or (it & 0xFF) >= k + m for it in items):
        return COUNTS, 0
    n_lost = 0
    for it in items:
        c, i = it >> 8, it & 0xFF
        if bm is None or bm[c, i] != 0:
            continue
        j = i % m if i < k else i - k
        cls = [l for l in range(j, k, m)] + [k + j]
        if any(bm[c, l] == 0 for l in cls if l != i):
            return FAIL, 0
        n_lost += 1
    return OK, n_lost


def check(bm, S, k, m, items):
    items = np.asarray(items, dtype=np.uint32)
    flat = None if bm is None else np.ascontiguousarray(bm, dtype=np.uint8).reshape(-1)
    return xec.check_read_items(flat, S, k, m, items, len(items))


@pytest.mark.parametrize("k,m", [(4, 1), (6, 2), (66, 2)])
def test_check_read_items_equals_the_rule_on_random_bitmaps(k, m):
    rng = np.random.default_rng(100 * k + m)
    S = 7
    seen = set()
    for trial in range(300):
        p_lost = (0.0, 0.02, 0.1, 0.3)[trial % 4]
        bm = (rng.random((S, k + m)) >= p_lost).astype(np.uint8)
        bm[bm != 0] = rng.choice([1, 2, 255], size=int((bm != 0).sum()))
        n = int(rng.integers(1, 40))
        items = (rng.integers(0, S, n) << 8) | rng.integers(0, k + m, n)  # data and parity
        items[n // 2] = items[0]  # a duplicate
        if trial % 11 == 0:
            items[int(rng.integers(n))] = (S << 8) | 0 if trial % 2 else ((S - 1) << 8) | (k + m)
        want = rule(bm, S, k, m, items)
        got = check(bm, S, k, m, items)
        assert got[0] == want[0], (trial, items, bm)
        if want[0] == OK:
            assert got[1] == want[1], trial
        seen.add((want[0], want[1] > 0))
    assert {(OK, False), (OK, True), (FAIL, False), (COUNTS, False)} <= seen


def test_named_cases():
    S, k, m = 3, 6, 2  # class 0: data 0, 2, 4 and parity 6; class 1: data 1, 3, 5 and parity 7
    bm = np.ones((S, k + m), np.uint8)
    bm[1, 0] = bm[1, 2] = 0  # stripe 1, class 0: doubly lost
    # a present item in a doubly-lost class
    assert check(bm, S, k, m, [(1 << 8) | 4, (1 << 8) | 6]) == (OK, 0)
    # its lost members are not servable
    assert check(bm, S, k, m, [(1 << 8) | 0])[0] == FAIL
    # an unrecoverable class not named by any item
    assert check(bm, S, k, m, [(1 << 8) | 1, (0 << 8) | 0, (2 << 8) | 7]) == (OK, 0)
    # a lost item whose class also lost its parity
    bm2 = np.ones((S, k + m), np.uint8)
    bm2[2, 3] = bm2[2, 7] = 0
    assert check(bm2, S, k, m, [(2 << 8) | 3])[0] == FAIL
    assert check(bm2, S, k, m, [(2 << 8) | 7])[0] == FAIL  # and the parity, whose member is lost
    assert check(bm2, S, k, m, [(2 << 8) | 1, (2 << 8) | 5]) == (OK, 0)
    # singly lost: data, parity, and a repeat counts each time
    bm3 = np.ones((S, k + m), np.uint8)
    bm3[0, 5] = bm3[0, 6] = 0
    assert check(bm3, S, k, m, [5, 6, 5, 1]) == (OK, 3)
    # out of range outranks not servable, wherever it stands in the list
    assert check(bm, S, k, m, [(S << 8) | 0])[0] == COUNTS                # c == S
    assert check(bm, S, k, m, [(0 << 8) | (k + m)])[0] == COUNTS          # i == k+m
    assert check(bm, S, k, m, [(1 << 8) | 0, (S << 8) | 0])[0] == COUNTS
    assert check(bm, S, k, m, [(0 << 8) | (k + m), (1 << 8) | 0])[0] == COUNTS
    # a NULL bitmap: everything is present
    assert check(None, S, k, m, [(1 << 8) | 0, (1 << 8) | 2, 7]) == (OK, 0)
    assert check(None, S, k, m, [(S << 8) | 0])[0] == COUNTS
    # bitmap bytes 2 and 255 are present
    bm4 = np.full((S, k + m), 2, np.uint8)
    bm4[:, 1::2] = 255
    assert check(bm4, S, k, m, [(c << 8) | i for c in range(S) for i in range(k + m)]) == (OK, 0)
    bm4[0, 0] = 0
    assert check(bm4, S, k, m, [0]) == (OK, 1)
    # nothing asked; invalid k, m as xec_check_args
    assert check(bm, S, k, m, []) == (OK, 0)
    assert check(bm, S, 6, 4, [0])[0] == COUNTS
    assert xec.check_read_items(None, S, k, m, None, 3)[0] == COUNTS
    # n_lost may be NULL
    it = np.array([5], np.uint32)
    assert xec.lib().xec_check_read_items(bm3.ctypes.data, S, k, m, it.ctypes.data, 1, None) == 0


def test_read_scratch_bytes_is_monotone_and_holds_items_and_bits():
    prev = 0
    for n in list(range(0, 200)) + [1023, 1024, 1025, 1056, 1057, 4096, 1 << 20, (1 << 24) + 5]:
        b = xec.read_scratch_bytes(n)
        assert b >= prev and b % 4 == 0
        assert b == 4 * (n + (n + 31) // 32)  # the items and one bit each
        prev = b
    assert xec.read_scratch_bytes(0) == 0


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_read_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == xec.Status.DEVICE_ERROR
    S, k, m, bs = 2, 4, 1, 4096
    NI = xec.Status.NOT_INITIALIZED
    items = np.array([0, (1 << 8) | 4], np.uint32)
    bm = np.ones(S * (k + m), np.uint8)
    out, dit, dst = 1 << 24, 1 << 25, 1 << 26
    assert xec.read(64, 128, S, bs, k, m, bm, items, 2, 0, 256, out) == NI
    assert xec.read(64, 128, S, bs, k, m, None, items, 2, 16, 16, out) == NI
    assert xec.read_device(64, 128, S, bs, k, m, 1 << 23, dit, 2, 0, 256, out, dst) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, dit, 2, 0, 256, out, dst) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    assert xec.read(65, 128, S, 100, 6, 4, bm, items, 2, 0, 256, out) == NI       # xec_check_args
    assert xec.read(64, 128, 0, bs, k, m, bm, items, 0, 0, 256, out) == NI        # nothing to do
    assert xec.read(64, 128, 1 << 25, bs, 255, 5, bm, items, 2, 0, 256, out) == NI  # the packing
    assert xec.read(64, 128, S, bs, k, m, bm, items, 2, 8, 0, out) == NI          # the range
    assert xec.read(64, 128, S, bs, k, m, bm, items, 2, bs, 16, out) == NI
    assert xec.read(64, 128, S, bs, k, m, bm, None, 2, 0, 256, None) == NI        # NULL
    assert xec.read(64, 128, S, bs, k, m, bm, items, 2, 0, 256, out + 8) == NI    # alignment
    assert xec.read(64, 128, S, bs, k, m, bm, items, 2, 0, 256, 64) == NI         # overlap
    bad = np.array([(S << 8), k + m], np.uint32)
    assert xec.read(64, 128, S, bs, k, m, bm, bad, 2, 0, 256, out) == NI          # the items
    assert xec.read(64, 128, S, bs, k, m, np.zeros_like(bm), items, 2, 0, 256, out) == NI
    assert xec.read_device(65, 128, S, 100, 6, 4, None, dit, 2, 0, 256, out, dst) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, dit, 2, 0, 256, out, None) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, dit, 2, 0, 256, out, dst + 2) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, None, 2, 0, 256, out, dst) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, dit + 2, 2, 0, 256, out, dst) == NI
    assert xec.read_device(64, 128, S, bs, k, m, None, dit, 0, 0, 256, out, dst) == NI
    assert xec.read_tiling_used() == 0
    # the host scan needs no initialisation
    assert xec.check_read_items(bm, S, k, m, items, 2) == (OK, 0)


def test_read_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_read.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, sz, sz, sz, vp, vp, sz, vp]
    assert list(L.xec_read_device.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, sz, sz, sz, vp, vp,
                                                vp]
    assert L.xec_read.restype is ctypes.c_int and L.xec_read_device.restype is ctypes.c_int
    assert list(L.xec_read_scratch_bytes.argtypes) == [sz] and L.xec_read_scratch_bytes.restype is sz
    assert list(L.xec_check_read_items.argtypes) == [vp, sz, sz, sz, vp, sz, ctypes.POINTER(sz)]
    assert L.xec_check_read_items.restype is ctypes.c_int
    assert list(L.xec_read_tiling_used.argtypes) == [] and L.xec_read_tiling_used.restype is ctypes.c_int
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("read", "read_device", "read_scratch_bytes", "check_read_items",
                 "read_tiling_used"):
        assert name in xec.__all__ and callable(getattr(xec, name))
