"""xec_write_shards_device and xec_readv_shards_device without a device: the
binding, the prototypes of include/xec.h, and the calls before xec_init.
"""
from __future__ import annotations

import ctypes
import subprocess
import sys
import textwrap

import xec
from conftest import PKG_DIR, ROOT

NEW = ("xec_write_shards_device", "xec_readv_shards_device")


def test_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    table = [vp, sz, sz, sz, sz, sz, sz]
    assert list(L.xec_write_shards_device.argtypes) == table + [vp, vp, sz, sz, sz, vp, vp, vp, vp]
    assert list(L.xec_readv_shards_device.argtypes) == table + [vp, vp, sz, vp, sz, vp, sz, vp, vp]
    for name in NEW:
        assert getattr(L, name).restype is ctypes.c_int
        assert name in xec.EXPORTED
    for name in ("write_shards_device", "readv_shards_device"):
        assert name in xec.__all__ and callable(getattr(xec, name))


def test_the_header_declares_them():
    text = " ".join((ROOT / "include" / "xec.h").read_text().split())
    table = "const void* const* h_shards, size_t data_stride, size_t parity_stride, size_t S, " \
            "size_t bs, size_t k, size_t m"
    assert (f"xec_status xec_write_shards_device({table}, const uint8_t* d_bitmap, "
            "const uint32_t* d_items, size_t n_items, size_t offset, size_t len, "
            "const void* d_new, uint64_t* d_digests, int32_t* d_status, "
            "hipStream_t stream);") in text
    assert (f"xec_status xec_readv_shards_device({table}, const uint8_t* d_bitmap, "
            "const xec_iov* d_iov, size_t n_items, void* d_out, size_t out_bytes, void* d_work, "
            "size_t work_bytes, int32_t* d_status, hipStream_t stream);") in text
    # the write stands with the shard calls, the read after the xec_iov it takes
    assert text.index("xec_status xec_read_shards_device(") < text.index(
        "xec_status xec_write_shards_device(") < text.index("int xec_shards_arg_capacity_used(")
    assert text.index("} xec_iov;") < text.index("xec_status xec_readv_shards_device(")
    # named where the kernel events, the rotation and the capacity list their calls
    events = text[text.index("the calling thread's NEXT xec_encode"):
                  text.index("xec_status xec_set_kernel_events(")]
    rotation = text[text.index("column rotation of the encode"):
                    text.index("xec_status xec_set_rotation(")]
    capacity = text[text.index("thread's most recent shard call"):
                    text.index("int xec_shards_arg_capacity_used(")]
    for name in NEW:
        assert name in events and name in rotation and name in capacity, name


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import xec
NI = xec.Status.NOT_INITIALIZED
BASE = 1 << 32  # fabricated device addresses: only their values are looked at
S, bs, k, m = 2, 4096, 4, 1
good = [BASE + i * (1 << 20) for i in range(k + m)]
dig, bm, items, new, out, work, status, iov = (BASE + (n << 24) for n in range(8, 16))
wb = xec.readv_device_work_bytes(3)

def both(*table):
    assert xec.write_shards_device(*table, bm, items, 3, 0, 256, new, dig, status) == NI
    assert xec.write_shards_device(*table, None, items, 3, 16, 16, new, None, status) == NI
    assert xec.readv_shards_device(*table, bm, iov, 3, out, 4096, work, wb, status) == NI
    assert xec.readv_shards_device(*table, None, iov, 3, out, 4096, work, wb, status) == NI
    assert xec.shards_arg_capacity_used() == 0

both(good, bs, bs, S, bs, k, m)
# ... also with arguments that would be rejected: initialisation is asked first
for table in ((good, bs, bs, S, 100, k, m), (good, bs, bs, S, bs, 6, 4),
              (None, bs, bs, S, bs, k, m), (good, bs, bs, 0, bs, k, m),
              (good, 8, bs, S, bs, k, m), ([good[0]] * (k + m), bs, bs, S, bs, k, m),
              ([BASE + i * (1 << 20) for i in range(257)], bs, bs, S, bs, 256, 1)):
    both(*table)
t = (good, bs, bs, S, bs, k, m)
w, r = xec.write_shards_device, xec.readv_shards_device
assert w(*t, bm, None, 3, 8, 24, None, dig + 4, None) == NI
assert w(*t, bm, items, 0, 0, 0, new, None, status + 2) == NI
assert w(*t, bm, items + 2, 3, 0, 256, new + 8, None, status) == NI
assert w(*t, bm, items, 3, 0, 256, good[0], None, status) == NI      # d_new on a shard
assert w(*t, bm, items, 3, 0, 256, new, good[1], status) == NI       # d_digests on a shard
assert w(*t, bm, items, (1 << 64) // 256, 0, 256, new, None, status) == NI
assert r(*t, bm, None, 3, None, 0, None, 0, None) == NI
assert r(*t, bm, iov + 2, 3, out + 8, 4096, work + 4, wb - 1, status + 2) == NI
assert r(*t, bm, iov, 0, out, 4096, work, wb, status) == NI
assert r(*t, bm, iov, 3, good[0], 4096, work, wb, status) == NI      # d_out on a shard
assert xec.shards_arg_capacity_used() == 0
# neither call reports through the batch calls' diagnostics
assert xec.write_tiling_used() == 0 and xec.readv_tiling_used() == 0
print("not-initialised-first")
"""


def test_calls_before_init_are_not_initialized():
    """In a fresh child process that never calls xec_init: both calls answer
    XEC_NOT_INITIALIZED whatever else is wrong with their arguments."""
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(CHILD).format(pkg=str(PKG_DIR))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "not-initialised-first" in r.stdout, r.stderr[-2000:]
