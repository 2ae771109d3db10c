"""xec_repair / xec_repair_device / xec_verify without a device: the order of
the checks the host can decide (CPU only).  A process that never initialised
the library gets XEC_NOT_INITIALIZED from each call before anything else; the
argument statuses behind it need xec_init and are checked in
tests/test_gpu_repair.py and tests/test_gpu_verify.py -- here the same codes
are pinned through the host-only pieces the calls are made of."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import xec


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_new_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == xec.Status.DEVICE_ERROR
    S, k, m, bs = 1, 4, 1, 4096
    bm = np.ones(5, dtype=np.uint8)
    NI = xec.Status.NOT_INITIALIZED
    assert xec.repair(64, 128, S, bs, k, m, bm, 256) == NI
    assert xec.repair_device(64, 128, S, bs, k, m, 256, 512) == NI
    assert xec.verify(64, 128, S, bs, k, m, 256, 512) == NI
    assert xec.verify(64, 128, S, bs, k, m, 256, None) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    assert xec.repair(65, 128, S, 100, 6, 4, bm, 0) == NI
    assert xec.repair_device(64, 128, S, bs, k, m, 0, 0) == NI
    assert xec.verify(64, 128, S, bs, k, m, 0, 2) == NI
    assert xec.repair_tiling_used() == 0


def test_repair_tiling_used_is_per_thread_and_starts_at_zero():
    import threading
    seen = {}

    def worker():
        seen["fresh"] = xec.repair_tiling_used()

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert seen == {"fresh": 0}
    assert xec.repair_tiling_used() == 0
    assert xec.decode_tiling_used() == 0  # its neighbour is untouched


@pytest.mark.parametrize("args,want", [
    ((4096, 8192, 4096, 4, 1), 0),
    ((4096 + 16, 8192, 4096, 4, 1), 2),   # data not 64-B aligned
    ((4096, 8192 + 32, 4096, 4, 1), 2),   # parity not 64-B aligned
    ((4096, 8192, 100, 4, 1), 1),         # bs not a multiple of 256
    ((4096, 8192, 4096, 6, 4), 3),        # k % m
    ((4096, 8192, 4096, 0, 1), 3),
])
def test_argument_statuses_are_xec_check_args(args, want):
    """The three calls check (data, parity, bs, k, m) with xec_check_args, as
    xec_decode does; these are the codes they then return."""
    assert xec.check_args(*args) == want


def test_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    nine = [vp, vp, sz, sz, sz, sz, vp, vp, vp]
    for name in ("xec_repair", "xec_repair_device", "xec_verify"):
        fn = getattr(L, name)
        assert list(fn.argtypes) == nine and fn.restype is ctypes.c_int, name
    assert L.xec_repair_tiling_used.argtypes == [] or list(L.xec_repair_tiling_used.argtypes) == []
    for name in ("xec_repair", "xec_repair_device", "xec_verify", "xec_repair_tiling_used"):
        assert name in xec.EXPORTED
