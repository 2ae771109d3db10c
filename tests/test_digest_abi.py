"""Block digests without a device: xec_digest_host against the formula, and
what the host alone decides of xec_digest / xec_locate (CPU only).

    digest(block) = sum over its little-endian u64 words w[n] of
                    splitmix_at(w[n], n)                       (mod 2^64)

splitmix_at(seed, n) is the splitmix64 finaliser of seed + (n+1)*golden.  The
numpy restatement below is the reference of this file and of
tests/test_gpu_digest.py; nothing here is computed by the library and then
compared with itself.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import xec

NEW = ("xec_digest_host", "xec_digest", "xec_locate", "xec_locate_work_bytes")
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def np_digest(blocks: np.ndarray) -> np.ndarray:
    """Digest of every row of a (..., bs) uint8 array, in numpy (uint64 wraps)."""
    blocks = np.ascontiguousarray(blocks)
    w = blocks.view("<u8")
    n = np.arange(1, w.shape[-1] + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = w + n * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return z.sum(axis=-1, dtype=np.uint64)


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


@pytest.mark.parametrize("block,want", [
    (np.zeros(256, np.uint8), 0x437C59C2797BD0CB),
    (np.arange(256, dtype=np.uint8), 0x0308856E007DF973),
    (np.zeros(8, np.uint8), 0xE220A8397B1DCDAF),  # splitmix64's first output from state 0
], ids=["256-zero-bytes", "bytes-0-to-255", "8-zero-bytes"])
def test_known_answers(block, want):
    assert xec.digest_host(block) == want
    assert int(np_digest(block)) == want  # the restatement agrees with the issue's table
    assert xec.digest_host(block.tobytes()) == want


@pytest.mark.parametrize("bs", [8, 256, 1280, 4352])
def test_host_digest_equals_the_formula(bs):
    rng = np.random.default_rng(bs)
    blocks = rng.integers(0, 256, size=(16, bs), dtype=np.uint8)
    want = np_digest(blocks)
    for row, w in zip(blocks, want):
        assert xec.digest_host(row) == int(w)
    # the position of a word matters: swapping two different words changes the sum
    sw = blocks[0].copy()
    if bs >= 16 and not np.array_equal(sw[:8], sw[8:16]):
        sw[:8], sw[8:16] = blocks[0][8:16], blocks[0][:8]
        assert xec.digest_host(sw) != int(want[0])


def test_every_single_bit_flip_changes_the_digest():
    rng = np.random.default_rng(2048)
    block = rng.integers(0, 256, size=256, dtype=np.uint8)
    base = xec.digest_host(block)
    assert base == int(np_digest(block))
    seen = set()
    for bit in range(2048):
        block[bit >> 3] ^= 1 << (bit & 7)
        d = xec.digest_host(block)
        block[bit >> 3] ^= 1 << (bit & 7)
        assert d != base, f"bit {bit}"
        seen.add(d)
    assert len(seen) == 2048  # and no two flips collide
    assert xec.digest_host(block) == base


@pytest.mark.parametrize("S,k,m", [(0, 4, 1), (1, 4, 1), (23, 66, 2), (65536, 32, 1),
                                   (1 << 24, 255, 1)])
def test_locate_work_bytes_is_eight_per_block(S, k, m):
    assert xec.locate_work_bytes(S, k, m) == 8 * S * (k + m)


def test_digest_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == xec.Status.DEVICE_ERROR
    S, k, m, bs = 2, 4, 1, 4096
    NI = xec.Status.NOT_INITIALIZED
    wb = 8 * S * (k + m)
    assert xec.digest(64, 128, S, bs, k, m, 1 << 20) == NI
    assert xec.digest(64, 128, S, bs, k, m, 1 << 20, 1 << 21) == NI
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, None, 1 << 21, 1 << 22, 1 << 23, wb) == NI
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, 1 << 19, 1 << 21, None, 1 << 23, wb) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    assert xec.digest(65, 128, S, 100, 6, 4, 1 << 20) == NI                  # xec_check_args
    assert xec.digest(64, 128, S, bs, k, m, None) == NI                      # NULL digests
    assert xec.digest(64, 128, S, bs, k, m, (1 << 20) + 4) == NI             # misaligned digests
    assert xec.digest(64, 128, 0, bs, k, m, None) == NI                      # even an empty batch
    assert xec.locate(65, 128, S, 100, 6, 4, 1 << 20, None, 1 << 21, None, 1 << 23, wb) == NI
    assert xec.locate(64, 128, S, bs, k, m, None, None, 1 << 21, None, 1 << 23, wb) == NI
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, None, 1 << 21, None, None, wb) == NI
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, None, 1 << 21, None, 1 << 23, wb - 1) == NI
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, None, 1 << 21, (1 << 22) + 2,
                      (1 << 23) + 4, wb) == NI                               # misaligned
    assert xec.locate(64, 128, S, bs, k, m, 1 << 20, None, None, None, 1 << 23, wb) == NI
    assert xec.locate(64, 128, 0, bs, k, m, None, None, None, None, None, 0) == NI
    # the host digest needs no initialisation
    assert xec.digest_host(np.zeros(8, np.uint8)) == 0xE220A8397B1DCDAF


def test_digest_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_digest_host.argtypes) == [vp, sz]
    assert L.xec_digest_host.restype is ctypes.c_uint64
    assert list(L.xec_digest.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, vp]
    assert list(L.xec_locate.argtypes) == [vp, vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, sz, vp]
    assert L.xec_digest.restype is ctypes.c_int and L.xec_locate.restype is ctypes.c_int
    assert list(L.xec_locate_work_bytes.argtypes) == [sz, sz, sz]
    assert L.xec_locate_work_bytes.restype is sz
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("digest", "locate", "locate_work_bytes", "digest_host"):
        assert name in xec.__all__ and callable(getattr(xec, name))
