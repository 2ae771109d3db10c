"""The shard-major layout without a device: the binding, xec_check_shards on
fabricated pointer values -- every rejection of its steps 1 to 7 in order, the
interleave rule at its edges, the capacity limit -- the compute calls before
xec_init, and the capacity mapping of csrc/xec_dispatch.h as a host program.

The rule (include/xec.h): shard x covers the hull [p_x, p_x + (S-1)*s_x + bs);
a pair of shards is accepted if the hulls are disjoint, or if both have the
same stride s and d = (p_y - p_x) mod s leaves d >= bs and s - d >= bs.
"""
from __future__ import annotations

import ctypes
import shutil
import subprocess

import pytest

import xec
from conftest import ROOT

NEW = ("xec_check_shards", "xec_encode_shards", "xec_repair_shards_device", "xec_verify_shards",
       "xec_shards_arg_capacity_used")
St = xec.Status
OK, SIZE, ALIGN, COUNTS = St.SUCCESS, St.INVALID_SIZE, St.INVALID_ALIGNMENT, St.INVALID_COUNTS

BASE = 1 << 32  # fabricated device addresses: only their values are looked at


def batch_table(d, p, bs, k, m):
    """The batch layout as a shard table: (pointers, data_stride, parity_stride)."""
    return [d + i * bs for i in range(k)] + [p + j * bs for j in range(m)], k * bs, m * bs


def separate(n, span, base=BASE):
    """n shards `span` bytes apart."""
    return [base + i * span for i in range(n)]


def check(ptrs, ds, ps, S, bs, k, m):
    return xec.check_shards(ptrs, ds, ps, S, bs, k, m)


def test_signatures_are_bound():
    L = xec.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert list(L.xec_check_shards.argtypes) == [vp, sz, sz, sz, sz, sz, sz]
    assert list(L.xec_encode_shards.argtypes) == [vp, sz, sz, sz, sz, sz, sz, vp]
    assert list(L.xec_repair_shards_device.argtypes) == [vp, sz, sz, sz, sz, sz, sz, vp, vp, vp]
    assert list(L.xec_verify_shards.argtypes) == [vp, sz, sz, sz, sz, sz, sz, vp, vp, vp]
    assert list(L.xec_shards_arg_capacity_used.argtypes) == []
    for name in NEW[:4]:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.xec_shards_arg_capacity_used.restype is ctypes.c_int
    for name in NEW:
        assert name in xec.EXPORTED
    for name in ("check_shards", "encode_shards", "repair_shards_device", "verify_shards",
                 "shards_arg_capacity_used", "shard_table"):
        assert name in xec.__all__ and callable(getattr(xec, name))
    # the header declares them with these parameter lists
    text = " ".join((ROOT / "include" / "xec.h").read_text().split())
    table = "const void* const* h_shards, size_t data_stride, size_t parity_stride, size_t S, " \
            "size_t bs, size_t k, size_t m"
    assert f"xec_status xec_check_shards({table});" in text
    assert f"xec_status xec_encode_shards({table}, hipStream_t stream);" in text
    assert (f"xec_status xec_repair_shards_device({table}, const uint8_t* d_bitmap, "
            "int32_t* d_status, hipStream_t stream);") in text
    assert (f"xec_status xec_verify_shards({table}, uint8_t* d_flags, uint32_t* d_count, "
            "hipStream_t stream);") in text
    assert "int xec_shards_arg_capacity_used(void);" in text


def test_shard_table_builds_a_pointer_array():
    t = xec.shard_table([64, 128, None])
    assert isinstance(t, ctypes.Array) and len(t) == 3 and list(t) == [64, 128, None]
    assert xec.shard_table(t) is t and xec.shard_table(None) is None

    class Tensorish:
        def data_ptr(self):
            return 4096

    assert list(xec.shard_table([Tensorish()])) == [4096]


@pytest.mark.parametrize("k,m", [(4, 1), (6, 2), (4, 4)])
@pytest.mark.parametrize("S", [1, 2, 9])
def test_the_batch_layout_is_accepted(k, m, S):
    bs = 4352
    ptrs, ds, ps = batch_table(BASE, BASE + (1 << 30), bs, k, m)
    assert check(ptrs, ds, ps, S, bs, k, m) == OK
    # ... and parity right behind the data, touching it
    ptrs, ds, ps = batch_table(BASE, BASE + S * k * bs, bs, k, m)
    assert check(ptrs, ds, ps, S, bs, k, m) == OK
    # separate allocations at stride bs and at a padded stride
    assert check(separate(k + m, S * bs), bs, bs, S, bs, k, m) == OK
    assert check(separate(k + m, S * (bs + 4096)), bs + 4096, bs + 4096, S, bs, k, m) == OK
    # shards in any address order
    shuffled = separate(k + m, S * bs)[::-1]
    assert check(shuffled, bs, bs, S, bs, k, m) == OK


def test_rejections_in_order():
    """Each step's rejection, and an earlier step outranking every later one:
    the table handed to step n also breaks steps n+1.. wherever it can."""
    S, bs, k, m = 3, 512, 4, 1
    good = separate(k + m, 1 << 20)
    assert check(good, bs, bs, S, bs, k, m) == OK
    null_entry = good[:2] + [None] + good[3:]
    misaligned = good[:2] + [good[2] + 32] + good[3:]
    same = [good[0]] * (k + m)  # every pair overlaps
    wide = separate(257, 1 << 20)
    # 1. bs, then k and m, as xec_check_args
    for bad_bs in (0, 100, 255, 257, 768 + 64):
        assert check(None, 8, 8, S, bad_bs, 0, 0) == SIZE, bad_bs
        assert check(wide, 32, 32, S, bad_bs, 256, 1) == SIZE
    for bad_k, bad_m in ((0, 1), (1, 0), (6, 4), (3, 2)):
        assert check(None, 8, 8, S, bs, bad_k, bad_m) == COUNTS, (bad_k, bad_m)
    assert check(None, 8, 8, S, 100, 6, 4) == SIZE  # the size first
    # 2. no stripes: success whatever the table
    assert check(None, 8, 8, 0, bs, k, m) == OK
    assert check(same, 32, 32, 0, bs, 300, 100) == OK
    assert check(None, 8, 8, 0, 100, k, m) == SIZE and check(None, 8, 8, 0, bs, 6, 4) == COUNTS
    # 3. more than 256 shards, before the table is looked at
    assert check(None, 8, 8, S, bs, 256, 1) == SIZE
    assert check(wide, bs, bs, S, bs, 256, 1) == SIZE
    assert check(None, 8, 8, S, bs, 1 << 40, 1 << 20) == SIZE
    # 4. a NULL table or entry, before alignment, strides and overlap
    assert check(None, 8, 8, S, bs, k, m) == SIZE
    assert check(null_entry, bs, bs, S, bs, k, m) == SIZE
    assert check([None] + misaligned[1:], 32, bs, S, bs, k, m) == SIZE
    # 5. alignment of an entry or a stride, before the strides' sizes and overlap
    assert check(misaligned, bs, bs, S, bs, k, m) == ALIGN
    assert check(good[:-1] + [good[-1] + 8], bs, bs, S, bs, k, m) == ALIGN  # a parity shard
    assert check(good, bs + 32, bs, S, bs, k, m) == ALIGN
    assert check(good, bs, bs + 16, S, bs, k, m) == ALIGN
    assert check(misaligned, 64, 64, S, bs, k, m) == ALIGN      # stride < bs as well
    assert check([good[0] + 8] * (k + m), bs, bs, S, bs, k, m) == ALIGN  # overlapping as well
    assert check(same, 8, bs, S, bs, k, m) == ALIGN             # stride misaligned, < bs, overlap
    # 6. a stride below bs, or a hull past 64 bits, before overlap
    assert check(good, bs - 64, bs, S, bs, k, m) == SIZE
    assert check(good, bs, 64, S, bs, k, m) == SIZE
    assert check(good, 0, bs, S, bs, k, m) == SIZE
    assert check(good, bs - 64, bs, 1, bs, k, m) == SIZE        # even where no second block exists
    assert check(good, 1 << 62, bs, 5, bs, k, m) == SIZE        # (S-1)*stride overflows
    assert check(good, bs, 1 << 63, 3, bs, k, m) == SIZE
    assert check(good, (1 << 64) - 64, bs, 2, bs, k, m) == SIZE  # ... + bs overflows
    assert check(good, bs, bs, 1 << 60, bs, k, m) == SIZE
    assert check([(1 << 64) - 4096] + good[1:], bs, bs, 16, bs, k, m) == SIZE  # wraps the address space
    assert check(same, bs - 64, bs, S, bs, k, m) == SIZE
    # 7. overlap
    assert check(same, bs, bs, S, bs, k, m) == SIZE
    assert check(good[:-1] + [good[0]], bs, bs, S, bs, k, m) == SIZE      # parity aliases data
    assert check(good[:3] + [good[2] + bs] + good[4:], bs, bs, S, bs, k, m) == SIZE  # stride bs, one block on
    assert check(good[:3] + [good[2] + S * bs] + good[4:], bs, bs, S, bs, k, m) == OK  # hulls touch


def test_a_single_stripe():
    bs, k, m = 256, 4, 1
    touching = separate(k + m, bs)
    for stride in (bs, 64 * bs, 1 << 40):  # with one stripe the stride moves nothing
        assert check(touching, stride, stride, 1, bs, k, m) == OK
    assert check(touching, bs, bs, 2, bs, k, m) == SIZE  # a second stripe lands on the neighbour
    assert check(touching[:-1] + [touching[0] + 64], bs, bs, 1, bs, k, m) == SIZE
    assert check(touching, 2 * bs, 2 * bs, 1, bs, k, m) == OK


def test_interleaved_shards():
    S, bs, k, m = 5, 1024, 2, 1
    p, par = BASE, BASE + (1 << 30)
    s2 = 2 * bs
    assert check([p, p + bs, par], s2, bs, S, bs, k, m) == OK
    assert check([p + bs, p, par], s2, bs, S, bs, k, m) == OK        # y below x
    assert check([p, p + bs - 64, par], s2, bs, S, bs, k, m) == SIZE  # d = bs - 64
    assert check([p, p + bs + 64, par], s2, bs, S, bs, k, m) == SIZE  # s - d = bs - 64
    assert check([p + bs + 64, p, par], s2, bs, S, bs, k, m) == SIZE
    assert check([p, p + s2, par], s2, bs, S, bs, k, m) == SIZE       # d = 0: one stripe on
    assert check([p, p + 3 * bs, par], s2, bs, S, bs, k, m) == OK     # d = bs again
    # room for a third shard in a stride of 3 blocks, not in one of 2
    assert check([p, p + bs, p + 2 * bs], 3 * bs, 3 * bs, S, bs, k, m) == OK
    assert check([p, p + bs, p + 2 * bs], s2, s2, S, bs, k, m) == SIZE
    # a gap in the stride: blocks need not fill it
    assert check([p, p + bs + 64, par], s2 + 128, bs, S, bs, k, m) == OK


def test_different_strides_need_disjoint_hulls():
    S, bs, k, m = 4, 512, 2, 1
    p = BASE
    data = [p, p + (1 << 20)]
    # the parity shard starts inside data shard 0's hull; its blocks do not touch
    # that shard's blocks, and the conservative rule still refuses the pair
    inside = p + bs
    assert check(data + [inside], 4 * bs, 2 * bs, S, bs, k, m) == SIZE
    assert check(data + [inside], 4 * bs, 4 * bs, S, bs, k, m) == OK   # same stride: interleaved
    assert check(data + [p + 3 * 4 * bs + bs], 4 * bs, 2 * bs, S, bs, k, m) == OK  # just past the hull
    assert check(data + [p + 3 * 4 * bs + bs - 64], 4 * bs, 2 * bs, S, bs, k, m) == SIZE
    assert check(data + [p - (3 * 2 * bs + bs)], 4 * bs, 2 * bs, S, bs, k, m) == OK  # just before it
    assert check(data + [p - (3 * 2 * bs + bs) + 64], 4 * bs, 2 * bs, S, bs, k, m) == SIZE


def test_the_capacity_limit():
    S, bs = 2, 256
    for k, m in ((255, 1), (128, 128), (254, 2)):
        assert check(separate(k + m, S * bs), bs, bs, S, bs, k, m) == OK, (k, m)
    for k, m in ((256, 1), (255, 5), (129, 129)):
        assert check(separate(k + m, S * bs), bs, bs, S, bs, k, m) == SIZE, (k, m)
    # 256 interleaved shards in one stride: the batch layout at 255 + 1
    ptrs, ds, ps = batch_table(BASE, BASE + S * 255 * bs, bs, 255, 1)
    assert check(ptrs, ds, ps, S, bs, 255, 1) == OK
    ptrs[200] += 64
    assert check(ptrs, ds, ps, S, bs, 255, 1) == SIZE


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the process-level GPU tests")


def test_shard_calls_before_init_are_not_initialized():
    _no_gpu()
    assert xec.init(0) == St.DEVICE_ERROR
    S, bs, k, m = 2, 4096, 4, 1
    NI = St.NOT_INITIALIZED
    good = separate(k + m, 1 << 20)
    bm, status, flags, count = 1 << 24, 1 << 25, 1 << 26, 1 << 27
    assert xec.encode_shards(good, bs, bs, S, bs, k, m) == NI
    assert xec.repair_shards_device(good, bs, bs, S, bs, k, m, bm, status) == NI
    assert xec.verify_shards(good, bs, bs, S, bs, k, m, flags, count) == NI
    assert xec.verify_shards(good, bs, bs, S, bs, k, m, flags, None) == NI
    # ... also with arguments that would be rejected: initialisation is asked first
    for args in ((good, bs, bs, S, 100, k, m), (good, bs, bs, S, bs, 6, 4), (None, bs, bs, S, bs, k, m),
                 (good, bs, bs, 0, bs, k, m), (good, 8, bs, S, bs, k, m),
                 ([good[0]] * (k + m), bs, bs, S, bs, k, m),
                 (separate(257, 1 << 20), bs, bs, S, bs, 256, 1)):
        assert xec.encode_shards(*args) == NI
        assert xec.repair_shards_device(*args, bm, status) == NI
        assert xec.verify_shards(*args, flags, count) == NI
    assert xec.repair_shards_device(good, bs, bs, S, bs, k, m, None, status) == NI
    assert xec.repair_shards_device(good, bs, bs, S, bs, k, m, bm, status + 2) == NI
    assert xec.repair_shards_device(good, bs, bs, S, bs, k, m, bm, None) == NI
    assert xec.verify_shards(good, bs, bs, S, bs, k, m, None, count + 1) == NI
    assert xec.shards_arg_capacity_used() == 0
    # the host check needs no initialisation
    assert check(good, bs, bs, S, bs, k, m) == OK


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shard_capacity_map_asan_ubsan(tmp_path):
    """The capacity mapping of csrc/xec_dispatch.h as a host program of its own:
    64 pointers up to k + m = 64, 256 beyond; the older mappings unchanged."""
    exe = tmp_path / "shard_capacity_map"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'erasure-code-benchmark_amd' / 'csrc'}",
                    str(ROOT / "tests" / "host" / "shard_capacity_map.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shard_capacity_map ok" in p.stdout
