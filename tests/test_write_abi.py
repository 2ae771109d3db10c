"""Degraded write without a device: the bindings, the header's declarations,
xec_write_scratch_bytes, and xec_check_write_items -- the host scan xec_write
runs -- against a numpy restatement of the rule (CPU only).

A written item c << 8 | i (i < k, strictly ascending) is servable if its block
is present (bitmap byte != 0, or no bitmap), or lost with every other block of
its class present.  A lost item is a rebuild-write item; an item whose class
lost its parity block is a data-only item.  Only the classes the items name are
looked at, and a broken item rule anywhere outranks an unservable item.
"""
from __future__ import annotations

import ctypes
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import xec
from conftest import PKG_DIR, ROOT

NEW = ("xec_write", "xec_write_scratch_bytes", "xec_write_device", "xec_check_write_items",
       "xec_write_tiling_used")
OK, COUNTS, FAIL = xec.Status.SUCCESS, xec.Status.INVALID_COUNTS, xec.Status.DECODE_FAILURE


def rule(bm, S, k, m, items):
    """(status, n_rebuild, n_data_only) by the rule above, one item at a time."""
    items = [int(x) for x in items]
    for t, it in enumerate(items):
        if (it >> 8) >= S or (it & 0xFF) >= k or (t > 0 and it <= items[t - 1]):
            return COUNTS, 0, 0
    n_rebuild = n_data = 0
    for it in items:
        c, i = it >> 8, it & 0xFF
        if bm is None:
            continue
        j = i % m
        if bm[c, i] == 0:
            cls = [l for l in range(j, k, m)] + [k + j]
            if any(bm[c, l] == 0 for l in cls if l != i):
                return FAIL, 0, 0
            n_rebuild += 1
        if bm[c, k + j] == 0:
            n_data += 1
    return OK, n_rebuild, n_data


def check(bm, S, k, m, items):
    items = np.asarray(items, dtype=np.uint32)
    flat = None if bm is None else np.ascontiguousarray(bm, dtype=np.uint8).reshape(-1)
    return xec.check_write_items(flat, S, k, m, items, len(items))


@pytest.mark.parametrize("k,m", [(4, 1), (6, 2), (66, 2)])
def test_check_write_items_equals_the_rule_on_random_bitmaps(k, m):
    rng = np.random.default_rng(200 * k + m)
    S = 7
    seen = set()
    for trial in range(300):
        p_lost = (0.0, 0.02, 0.1, 0.3)[trial % 4]
        bm = (rng.random((S, k + m)) >= p_lost).astype(np.uint8)
        bm[bm != 0] = rng.choice([1, 2, 255], size=int((bm != 0).sum()))
        n = int(rng.integers(1, 40))
        flat = np.sort(rng.permutation(S * k)[:n])
        items = ((flat // k) << 8) | (flat % k)
        n = len(items)
        if trial % 11 == 0:
            t = int(rng.integers(n))
            items[t] = [(S << 8) | 0, ((S - 1) << 8) | k, items[max(t - 1, 0)]][trial % 3]
        want = rule(bm, S, k, m, items)
        got = check(bm, S, k, m, items)
        assert got[0] == want[0], (trial, items, bm)
        if want[0] == OK:
            assert got[1:] == want[1:], trial
        seen.add((want[0], want[1] > 0, want[2] > 0))
    assert {(OK, False, False), (OK, True, False), (OK, False, True), (FAIL, False, False),
            (COUNTS, False, False)} <= seen


def test_named_cases():
    S, k, m = 3, 6, 2  # class 0: data 0, 2, 4 and parity 6; class 1: data 1, 3, 5 and parity 7
    ones = np.ones((S, k + m), np.uint8)
    # a present item
    assert check(ones, S, k, m, [(1 << 8) | 4]) == (OK, 0, 0)
    # a lost item alone in its class: a rebuild-write
    bm = ones.copy()
    bm[1, 2] = 0
    assert check(bm, S, k, m, [(1 << 8) | 2]) == (OK, 1, 0)
    assert check(bm, S, k, m, [(1 << 8) | 0, (1 << 8) | 2, (1 << 8) | 3, (1 << 8) | 4]) == (OK, 1, 0)
    # a lost item with the parity lost
    bm = ones.copy()
    bm[2, 3] = bm[2, 7] = 0
    assert check(bm, S, k, m, [(2 << 8) | 3])[0] == FAIL
    # a lost item with another member lost
    bm = ones.copy()
    bm[1, 0] = bm[1, 2] = 0
    assert check(bm, S, k, m, [(1 << 8) | 0])[0] == FAIL
    # a present item in that doubly-lost class: delta, the lost members are not needed
    assert check(bm, S, k, m, [(1 << 8) | 4]) == (OK, 0, 0)
    # a member and the parity lost, a third, present member written: data-only
    bm = ones.copy()
    bm[0, 1] = bm[0, 7] = 0
    assert check(bm, S, k, m, [(0 << 8) | 3, (0 << 8) | 5]) == (OK, 0, 2)
    # the parity lost with a present item: data-only; items, not classes, are counted
    bm = ones.copy()
    bm[2, 6] = 0
    assert check(bm, S, k, m, [(2 << 8) | 0]) == (OK, 0, 1)
    assert check(bm, S, k, m, [(2 << 8) | 0, (2 << 8) | 1, (2 << 8) | 2, (2 << 8) | 4]) == (OK, 0, 3)
    # both kinds in one list
    bm[0, 5] = 0
    assert check(bm, S, k, m, [5, (2 << 8) | 0]) == (OK, 1, 1)
    # a broken item rule after an unservable item outranks it, wherever it stands
    bad = ones.copy()
    bad[1, 0] = bad[1, 2] = 0
    lost = (1 << 8) | 0
    assert check(bad, S, k, m, [lost])[0] == FAIL
    assert check(bad, S, k, m, [lost, (S << 8) | 0])[0] == COUNTS            # c == S
    assert check(bad, S, k, m, [lost, (2 << 8) | k])[0] == COUNTS            # i == k: parity is no item
    assert check(bad, S, k, m, [lost, (2 << 8) | 1, (2 << 8) | 1])[0] == COUNTS  # a duplicate
    assert check(bad, S, k, m, [lost, (2 << 8) | 1, (2 << 8) | 0])[0] == COUNTS  # descending
    assert check(bad, S, k, m, [(0 << 8) | k, lost])[0] == COUNTS
    # a NULL bitmap: everything is present
    assert check(None, S, k, m, [(1 << 8) | 0, (1 << 8) | 2, (2 << 8) | 5]) == (OK, 0, 0)
    assert check(None, S, k, m, [(S << 8) | 0])[0] == COUNTS
    # bitmap bytes 2 and 255 are present
    bm4 = np.full((S, k + m), 2, np.uint8)
    bm4[:, 1::2] = 255
    assert check(bm4, S, k, m, [(c << 8) | i for c in range(S) for i in range(k)]) == (OK, 0, 0)
    # nothing asked; invalid k, m as xec_check_args; NULL items
    assert check(ones, S, k, m, []) == (OK, 0, 0)
    assert check(ones, S, 6, 4, [0])[0] == COUNTS
    assert xec.check_write_items(None, S, k, m, None, 3)[0] == COUNTS
    # either count pointer may be NULL
    it = np.array([5], np.uint32)
    one = ctypes.c_size_t(7)
    L = xec.lib()
    assert L.xec_check_write_items(bm.ctypes.data, S, k, m, it.ctypes.data, 1, None, None) == 0
    assert L.xec_check_write_items(bm.ctypes.data, S, k, m, it.ctypes.data, 1, ctypes.byref(one),
                                   None) == 0 and one.value == 1
    assert L.xec_check_write_items(bm.ctypes.data, S, k, m, it.ctypes.data, 1, None,
                                   ctypes.byref(one)) == 0 and one.value == 0


def test_write_scratch_bytes_holds_items_and_two_bits_each():
    prev = 0
    for n in list(range(0, 200)) + [1023, 1024, 1025, 1040, 1041, 4096, 1 << 20, (1 << 24) + 5]:
        b = xec.write_scratch_bytes(n)
        assert b >= prev and b % 4 == 0
        assert b == 4 * (n + (n + 15) // 16)
        prev = b
    assert xec.write_scratch_bytes(0) == 0 and xec.write_scratch_bytes(1025) == 4 * (1025 + 65)


def test_write_signatures_are_bound_and_declared():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_write.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, vp, sz, sz, sz, vp, vp, sz,
                                          vp]
    assert list(L.xec_write_device.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, vp, sz, sz, vp, vp,
                                                 vp]
    assert L.xec_write.restype is ctypes.c_int and L.xec_write_device.restype is ctypes.c_int
    assert list(L.xec_write_scratch_bytes.argtypes) == [sz] and L.xec_write_scratch_bytes.restype is sz
    assert list(L.xec_check_write_items.argtypes) == [vp, sz, sz, sz, vp, sz, ctypes.POINTER(sz),
                                                      ctypes.POINTER(sz)]
    assert L.xec_check_write_items.restype is ctypes.c_int
    assert list(L.xec_write_tiling_used.argtypes) == [] and L.xec_write_tiling_used.restype is ctypes.c_int
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("write", "write_device", "write_scratch_bytes", "check_write_items",
                 "write_tiling_used"):
        assert name in xec.__all__ and callable(getattr(xec, name))
    header = (ROOT / "include" / "xec.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, ret, nargs in (("xec_write", "xec_status", 16), ("xec_write_scratch_bytes", "size_t", 1),
                             ("xec_write_device", "xec_status", 14),
                             ("xec_check_write_items", "xec_status", 8)):
        mt = re.search(rf"\b{ret}\s+{name}\(([^)]*)\)\s*;", code)
        assert mt, f"{name} is not declared in include/xec.h"
        assert len(mt.group(1).split(",")) == nargs, name
    assert re.search(r"\bint\s+xec_write_tiling_used\(void\)\s*;", code)
    # the kernel-events list names both calls
    assert re.search(r"xec_write or\s+\*?\s*xec_write_device call", header)


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import xec
NI = xec.Status.NOT_INITIALIZED
S, k, m, bs = 2, 4, 1, 4096
items = np.array([0, (1 << 8) | 3], np.uint32)
bm = np.ones(S * (k + m), np.uint8)
new, dbm, mask, dig, stat, scr = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29
w, wd = xec.write, xec.write_device
assert w(64, 128, new, S, bs, k, m, bm, items, 2, 0, 256) == NI
assert w(64, 128, new, S, bs, k, m, None, items, 2, 16, 16, dig) == NI
assert wd(64, 128, new, S, bs, k, m, dbm, mask, 0, 256, dig, stat) == NI
assert wd(64, 128, new, S, bs, k, m, None, mask, 0, 256, None, stat) == NI
# ... also with arguments that would be rejected: initialisation is asked first
assert w(65, 128, new, S, 100, 6, 4, bm, items, 2, 0, 256) == NI          # xec_check_args
assert w(64, 128, new, 0, bs, k, m, bm, items, 0, 0, 256) == NI           # nothing to do
assert w(64, 128, new, 1 << 25, bs, 260, 4, bm, items, 2, 0, 256) == NI   # the packing
assert w(64, 128, new, S, bs, k, m, bm, items, 2, 8, 0) == NI             # the range
assert w(64, 128, new, S, bs, k, m, bm, items, 2, bs, 16) == NI
assert w(64, 128, None, S, bs, k, m, bm, None, 2, 0, 256) == NI           # NULL
assert w(64, 128, new + 8, S, bs, k, m, bm, items, 2, 0, 256, dig + 4) == NI  # alignment
assert w(64, 128, 64, S, bs, k, m, bm, items, 2, 0, 256) == NI            # overlap
bad = np.array([(S << 8), k], np.uint32)
assert w(64, 128, new, S, bs, k, m, bm, bad, 2, 0, 256) == NI             # the items
assert w(64, 128, new, S, bs, k, m, np.zeros_like(bm), items, 2, 0, 256) == NI  # servability
many = np.arange(1100, dtype=np.uint32)
assert w(64, 128, new, 1100, bs, k, m, None, many << 8, 1100, 0, 256, None, scr + 2, 0) == NI
assert wd(65, 128, new, S, 100, 6, 4, None, mask, 0, 256, None, stat) == NI
assert wd(64, 128, new, 0, bs, k, m, None, mask, 0, 256, None, stat) == NI
assert wd(64, 128, new, S, bs, k, m, None, mask, 8, 0, None, stat) == NI
assert wd(64, 128, None, S, bs, k, m, None, None, 0, 256, None, stat) == NI
assert wd(64, 128, new + 8, S, bs, k, m, None, mask, 0, 256, dig + 4, stat) == NI
assert wd(64, 128, 64, S, bs, k, m, None, mask, 0, 256, None, stat) == NI
assert wd(64, 128, new, S, bs, k, m, None, mask, 0, 256, None, None) == NI
assert wd(64, 128, new, S, bs, k, m, None, mask, 0, 256, None, stat + 2) == NI
assert xec.write_tiling_used() == 0
# the host scan needs no initialisation
assert xec.check_write_items(bm, S, k, m, items, 2) == (xec.Status.SUCCESS, 0, 0)
print("not-initialised-first")
"""


def test_write_calls_before_init_are_not_initialized():
    """In a fresh child process that never calls xec_init: both calls answer
    XEC_NOT_INITIALIZED whatever else is wrong with their arguments."""
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(CHILD).format(pkg=str(PKG_DIR))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "not-initialised-first" in r.stdout, r.stderr[-2000:]
