"""xec_update / xec_update_device without a device: what the host alone
decides (CPU only).  A process that never initialised the library gets
XEC_NOT_INITIALIZED from each call before any other check; the statuses behind
it need xec_init and are asserted in tests/test_gpu_update.py."""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

import xec

NEW = ("xec_update", "xec_update_device", "xec_update_scratch_bytes", "xec_update_tiling_used")


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_update_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == xec.Status.DEVICE_ERROR
    S, k, m, bs = 2, 4, 1, 4096
    items = np.array([1, (1 << 8) | 3], dtype=np.uint32)
    NI = xec.Status.NOT_INITIALIZED
    assert xec.update(64, 128, 1 << 20, S, bs, k, m, items, 2) == NI
    assert xec.update_device(64, 128, 1 << 20, S, bs, k, m, 256) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    assert xec.update(65, 128, 1 << 20, S, 100, 6, 4, items, 2) == NI       # xec_check_args
    assert xec.update(64, 128, (1 << 20) + 8, S, bs, k, m, items, 2) == NI  # d_new misaligned
    assert xec.update(64, 128, 64, S, bs, k, m, items, 2) == NI             # d_new on the data
    assert xec.update(64, 128, 1 << 20, S, bs, k, m, items[::-1].copy(), 2) == NI  # unsorted
    assert xec.update(64, 128, 1 << 20, S, bs, 264, 4, items, 2) == NI      # k beyond the packing
    assert xec.update(64, 128, 1 << 20, S, bs, k, m, items, 0) == NI        # even an empty list
    assert xec.update_device(64, 128, 1 << 20, S, bs, k, m, 0) == NI        # NULL mask
    assert xec.update_device(64, 128, (1 << 20) + 8, S, 100, k, m, 256) == NI
    assert xec.update_tiling_used() == 0


@pytest.mark.parametrize("n", [0, 1, 64, 1024, 1025, 1 << 24, (1 << 32) + 3])
def test_update_scratch_bytes_is_four_per_item(n):
    assert xec.update_scratch_bytes(n) == 4 * n


def test_update_tiling_used_is_per_thread_and_starts_at_zero():
    seen = {}

    def worker():
        seen["fresh"] = xec.update_tiling_used()

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert seen == {"fresh": 0}
    assert xec.update_tiling_used() == 0
    assert xec.decode_tiling_used() == 0  # its neighbours are untouched
    assert xec.repair_tiling_used() == 0


def test_update_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_update.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, sz, vp, sz, vp]
    assert list(L.xec_update_device.argtypes) == [vp, vp, vp, sz, sz, sz, sz, vp, vp]
    assert L.xec_update.restype is ctypes.c_int and L.xec_update_device.restype is ctypes.c_int
    assert list(L.xec_update_scratch_bytes.argtypes) == [sz]
    assert L.xec_update_scratch_bytes.restype is sz
    assert list(L.xec_update_tiling_used.argtypes) == []
    assert L.xec_update_tiling_used.restype is ctypes.c_int
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("update", "update_device", "update_scratch_bytes", "update_tiling_used"):
        assert name in xec.__all__ and callable(getattr(xec, name))
