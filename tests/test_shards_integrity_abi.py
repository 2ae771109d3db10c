"""xec_digest_shards, xec_locate_shards and xec_read_shards_device without a
device: the binding, the prototypes of include/xec.h, and the calls before
xec_init.
"""
from __future__ import annotations

import ctypes

import pytest

import xec
from conftest import ROOT

NEW = ("xec_digest_shards", "xec_locate_shards", "xec_read_shards_device")
St = xec.Status
BASE = 1 << 32  # fabricated device addresses: only their values are looked at


def test_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    table = [vp, sz, sz, sz, sz, sz, sz]
    assert list(L.xec_digest_shards.argtypes) == table + [vp, vp, vp]
    assert list(L.xec_locate_shards.argtypes) == table + [vp, vp, vp, vp, vp, sz, vp]
    assert list(L.xec_read_shards_device.argtypes) == table + [vp, vp, sz, sz, sz, vp, vp, vp]
    for name in NEW:
        assert getattr(L, name).restype is ctypes.c_int
        assert name in xec.EXPORTED
    for name in ("digest_shards", "locate_shards", "read_shards_device"):
        assert name in xec.__all__ and callable(getattr(xec, name))


def test_the_header_declares_them():
    text = " ".join((ROOT / "include" / "xec.h").read_text().split())
    table = "const void* const* h_shards, size_t data_stride, size_t parity_stride, size_t S, " \
            "size_t bs, size_t k, size_t m"
    assert (f"xec_status xec_digest_shards({table}, const uint8_t* d_select, uint64_t* d_digests, "
            "hipStream_t stream);") in text
    assert (f"xec_status xec_locate_shards({table}, const uint64_t* d_digests, "
            "const uint8_t* d_flags, uint8_t* d_bitmap, uint32_t* d_count, void* d_work, "
            "size_t work_bytes, hipStream_t stream);") in text
    assert (f"xec_status xec_read_shards_device({table}, const uint8_t* d_bitmap, "
            "const uint32_t* d_items, size_t n_items, size_t offset, size_t len, void* d_out, "
            "int32_t* d_status, hipStream_t stream);") in text
    # declared after xec_verify_shards, and named where the kernel events list their calls
    assert text.index("xec_status xec_verify_shards(") < text.index("xec_status xec_digest_shards(")
    events = text[text.index("the calling thread's NEXT xec_encode"):
                  text.index("xec_status xec_set_kernel_events(")]
    for name in NEW:
        assert name in events, name


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == St.DEVICE_ERROR
    S, bs, k, m = 2, 4096, 4, 1
    NI = St.NOT_INITIALIZED
    good = [BASE + i * (1 << 20) for i in range(k + m)]
    dig, flags, bm, count, work, items, out, status = (BASE + (n << 24) for n in range(8, 16))
    wb = xec.locate_work_bytes(S, k, m)
    assert wb == 8 * S * (k + m)

    def all_three(*table):
        assert xec.digest_shards(*table, dig) == NI
        assert xec.digest_shards(*table, dig, flags) == NI
        assert xec.locate_shards(*table, dig, None, bm, count, work, wb) == NI
        assert xec.locate_shards(*table, dig, flags, bm, None, work, wb) == NI
        assert xec.read_shards_device(*table, bm, items, 3, 0, 256, out, status) == NI
        assert xec.read_shards_device(*table, None, items, 3, 0, 256, out, status) == NI
        assert xec.shards_arg_capacity_used() == 0

    all_three(good, bs, bs, S, bs, k, m)
    # ... also with arguments that would be rejected: initialisation is asked first
    for table in ((good, bs, bs, S, 100, k, m), (good, bs, bs, S, bs, 6, 4),
                  (None, bs, bs, S, bs, k, m), (good, bs, bs, 0, bs, k, m),
                  (good, 8, bs, S, bs, k, m), ([good[0]] * (k + m), bs, bs, S, bs, k, m),
                  ([BASE + i * (1 << 20) for i in range(257)], bs, bs, S, bs, 256, 1)):
        all_three(*table)
    t = (good, bs, bs, S, bs, k, m)
    assert xec.digest_shards(*t, None) == NI and xec.digest_shards(*t, dig + 4) == NI
    assert xec.locate_shards(*t, None, None, None, count + 2, None, 0) == NI
    assert xec.read_shards_device(*t, bm, None, 3, 8, 24, None, None) == NI
    assert xec.read_shards_device(*t, bm, items, 0, 0, 0, out, status + 2) == NI
    assert xec.read_shards_device(*t, bm, items, 3, 0, 256, good[0], status) == NI  # d_out on a shard
    assert xec.shards_arg_capacity_used() == 0
