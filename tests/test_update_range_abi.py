"""xec_update_range / xec_update_range_device / xec_digest_range_host without a
device: what the host alone decides (CPU only).  A process that never
initialised the library gets XEC_NOT_INITIALIZED from both device calls before
any other check; the statuses behind it need xec_init and are asserted in
tests/test_gpu_update_range.py.  xec_digest_range_host needs neither, and the
identities the digest upkeep rests on are checked here against xec_digest_host.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

import xec

from conftest import ROOT

NEW = ("xec_update_range", "xec_update_range_device", "xec_digest_range_host")
MASK = (1 << 64) - 1


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "xec.h").read_text()
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert name in xec.EXPORTED
        assert hasattr(L, name)
    for name in ("update_range", "update_range_device", "digest_range_host"):
        assert name in xec.__all__ and callable(getattr(xec, name))
    assert list(L.xec_update_range.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz, sz, vp,
                                                 vp, sz, vp]
    assert list(L.xec_update_range_device.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz,
                                                        vp, vp]
    assert L.xec_update_range.restype is ctypes.c_int
    assert L.xec_update_range_device.restype is ctypes.c_int
    assert list(L.xec_digest_range_host.argtypes) == [vp, sz, sz]
    assert L.xec_digest_range_host.restype is ctypes.c_uint64
    # as declared: the argument lists of the header, in order
    decl = re.search(r"xec_status xec_update_range\((.*?)\);", header, re.S).group(1)
    assert [a.split()[-1] for a in decl.split(",")] == [
        "d_data", "d_parity", "d_new", "S", "bs", "k", "m", "h_items", "n_items", "offset", "len",
        "d_digests", "d_scratch", "scratch_bytes", "stream"]
    decl = re.search(r"xec_status xec_update_range_device\((.*?)\);", header, re.S).group(1)
    assert [a.split()[-1] for a in decl.split(",")] == [
        "d_data", "d_parity", "d_new", "S", "bs", "k", "m", "d_mask", "offset", "len", "d_digests",
        "stream"]


def test_range_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == xec.Status.DEVICE_ERROR
    S, k, m, bs = 2, 4, 1, 4096
    items = np.array([1, (1 << 8) | 3], dtype=np.uint32)
    NI = xec.Status.NOT_INITIALIZED
    D, P, N, G, M = 64, 1 << 16, 1 << 20, 1 << 22, 256  # data, parity, new, digests, mask

    def host(d=D, p=P, new=N, S_=S, bs_=bs, k_=k, m_=m, it=items, n=2, off=16, ln=32, dig=G,
             scr=None, scr_bytes=0):
        return xec.update_range(d, p, new, S_, bs_, k_, m_, it, n, off, ln, dig, scr, scr_bytes)

    def dev(d=D, p=P, new=N, S_=S, bs_=bs, k_=k, m_=m, mask=M, off=16, ln=32, dig=G):
        return xec.update_range_device(d, p, new, S_, bs_, k_, m_, mask, off, ln, dig)

    assert host() == NI and dev() == NI
    assert host(dig=None) == NI and dev(dig=None) == NI
    # ... also with arguments that each later check would reject, in its order
    assert host(d=65) == NI and dev(d=65) == NI                  # 2 xec_check_args
    assert host(bs_=100, k_=6, m_=4) == NI and dev(bs_=100, k_=6, m_=4) == NI
    assert host(n=0) == NI and host(S_=0) == NI and dev(S_=0) == NI   # 3 nothing to do
    assert host(k_=264, m_=4) == NI and host(S_=(1 << 24) + 1) == NI  # 4 the packing
    for off, ln in ((16, 0), (8, 32), (16, 24), (bs - 16, 32), (bs + 16, 16)):  # 5 the range
        assert host(off=off, ln=ln) == NI and dev(off=off, ln=ln) == NI
    assert host(new=None) == NI and dev(new=None) == NI          # 6 NULL pointers
    assert host(it=None) == NI and dev(mask=None) == NI
    assert host(new=N + 8) == NI and dev(new=N + 8) == NI        # 7 alignment
    assert host(dig=G + 4) == NI and dev(dig=G + 4) == NI
    assert host(new=D + 64) == NI and dev(new=D) == NI           # 8 overlaps
    assert host(new=P) == NI and dev(new=P) == NI
    assert host(dig=D + 8) == NI and dev(dig=P) == NI and host(dig=N) == NI
    assert host(it=items[::-1].copy()) == NI                     # 9 the item rules
    assert host(n=1025) == NI and host(n=1025, scr=2, scr_bytes=1) == NI  # 10 the scratch
    assert xec.update_tiling_used() == 0


# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[256, 4352])
def block(request):
    bs = request.param
    rng = np.random.default_rng(bs)
    return (rng.integers(0, 256, size=bs, dtype=np.uint8),
            rng.integers(0, 256, size=bs, dtype=np.uint8))


def test_range_over_the_whole_block_is_the_digest(block):
    old, _ = block
    assert xec.digest_range_host(old, 0) == xec.digest_host(old)
    assert xec.digest_range_host(old, 0, old.size) == xec.digest_host(old)
    assert xec.digest_range_host(old.tobytes(), 0) == xec.digest_host(old)
    assert xec.digest_range_host(old, 0, 0) == 0
    assert xec.digest_range_host(old[8:], 8, 0) == 0


def test_range_is_additive_over_every_split(block):
    old, _ = block
    bs = old.size
    whole = xec.digest_host(old)
    for cut in range(0, bs + 1, 8):
        lo = xec.digest_range_host(old[:cut], 0, cut) if cut else 0
        hi = xec.digest_range_host(old[cut:], cut, bs - cut) if cut < bs else 0
        assert (lo + hi) & MASK == whole, cut
    # and of an inner range, split in three
    a, b, c, d = 16, 48, bs // 2, bs - 24
    parts = sum(xec.digest_range_host(old[x:y], x, y - x) for x, y in ((a, b), (b, c), (c, d)))
    assert parts & MASK == xec.digest_range_host(old[a:d], a, d - a)


def test_upkeep_identity_on_the_host(block):
    """digest(patched) = digest(old) + range(new) - range(old), mod 2^64: at the
    start, at the end and in the middle of the block."""
    old, new = block
    bs = old.size
    for off, ln in ((0, 16), (0, 64), (bs - 16, 16), (bs - 80, 80), (bs // 2 - 8, 48), (16, bs - 32),
                    (0, bs)):
        patched = old.copy()
        patched[off:off + ln] = new[:ln]
        delta = (xec.digest_range_host(new[:ln], off, ln)
                 - xec.digest_range_host(old[off:off + ln], off, ln))
        assert xec.digest_host(patched) == (xec.digest_host(old) + delta) & MASK, (off, ln)


def test_the_offset_is_part_of_the_term(block):
    old, _ = block
    piece = np.ascontiguousarray(old[32:96])
    seen = {xec.digest_range_host(piece, off, 64) for off in (0, 8, 32, 64, old.size - 64)}
    assert len(seen) == 5
    # the tail of len % 8 bytes is ignored, as in xec_digest_host
    assert xec.digest_range_host(piece, 32, 61) == xec.digest_range_host(piece, 32, 56)
