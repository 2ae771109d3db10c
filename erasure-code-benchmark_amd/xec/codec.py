"""Thin Python view of the C ABI (include/xec.h) for tests and bench.py.

Every function forwards to libxec_hip.so and returns the :class:`Status` the
library returned -- the same 0..4 codes as the reference XorecResult
(src/xorec/xorec_utils.hpp:26-32).  Device buffers are passed as integer
addresses or as torch tensors (``.data_ptr()``); streams as a
``torch.cuda.Stream``, a raw ``hipStream_t`` integer or ``None`` (null stream).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import Status, lib

#: xec_iov (include/xec.h): one entry of a vectored read, 12 bytes
IOV = np.dtype([("item", "<u4"), ("offset", "<u4"), ("len", "<u4")])


def _ptr(x) -> int:
    if x is None:
        return 0
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    if hasattr(x, "ctypes"):  # numpy array (host memory)
        return int(x.ctypes.data)
    return int(x)


def _stream(s) -> int:
    if s is None:
        return 0
    if hasattr(s, "cuda_stream"):
        return int(s.cuda_stream)
    return int(s)


def init(device_id: int = 0) -> Status:
    """xec_init -- replaces xorec_gpu_init + xorec_init (xorec_gpu_cmp.cu:7-27)."""
    return Status(lib().xec_init(int(device_id)))


def encode(d_data, d_parity, S: int, bs: int, k: int, m: int, stream=None) -> Status:
    """xec_encode -- replaces xorec_gpu_encode (xorec_gpu_cmp.cu:29-55)."""
    return Status(lib().xec_encode(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _stream(stream)))


def decode(d_data, d_parity, S: int, bs: int, k: int, m: int, h_bitmap, d_bitmap,
           stream=None) -> Status:
    """xec_decode -- replaces xorec_gpu_decode (xorec_gpu_cmp.cu:57-115); parity read-only."""
    return Status(lib().xec_decode(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _ptr(h_bitmap),
                                   _ptr(d_bitmap), _stream(stream)))


def decode_per_stripe(d_data, d_parity, S: int, bs: int, k: int, m: int, h_bitmap, d_bitmap,
                      h_codes=None, stream=None) -> Status:
    """xec_decode_per_stripe -- the reference CPU plugin's per-stripe semantics
    (xorec_bm.cpp:43-58): recoverable stripes are rebuilt, unrecoverable ones
    left alone; h_codes (S host bytes, optional) gets each stripe's 0 / 4."""
    return Status(lib().xec_decode_per_stripe(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                              _ptr(h_bitmap), _ptr(d_bitmap),
                                              _ptr(h_codes) if h_codes is not None else None,
                                              _stream(stream)))


def decode_device(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, d_status,
                  stream=None) -> Status:
    """xec_decode_device -- bitmap already on the device; batch verdict lands in
    d_status (int32 device tensor: 0 or 4) in stream order, nothing is synchronised."""
    return Status(lib().xec_decode_device(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                          _ptr(d_bitmap), _ptr(d_status), _stream(stream)))


def decode_device_list(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, d_work,
                       work_bytes: int, d_status, stream=None) -> Status:
    """xec_decode_device_list -- as decode_device, but the check kernel lists the
    lost data blocks into d_work (device scratch of device_list_bytes(S, k, m)
    bytes) and only those are rebuilt: for batches where few stripes lost blocks."""
    return Status(lib().xec_decode_device_list(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                               _ptr(d_bitmap), _ptr(d_work), work_bytes,
                                               _ptr(d_status), _stream(stream)))


def device_list_bytes(S: int, k: int, m: int) -> int:
    """xec_decode_device_list_bytes: scratch decode_device_list needs."""
    return int(lib().xec_decode_device_list_bytes(S, k, m))


def repair(d_data, d_parity, S: int, bs: int, k: int, m: int, h_bitmap, d_bitmap,
           stream=None) -> Status:
    """xec_repair -- every lost block, data or parity, rebuilt from the other
    members of its class (host bitmap; all-or-nothing; k + m <= 256)."""
    return Status(lib().xec_repair(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _ptr(h_bitmap),
                                   _ptr(d_bitmap), _stream(stream)))


def repair_device(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, d_status,
                  stream=None) -> Status:
    """xec_repair_device -- the same with the bitmap on the device; the batch
    verdict lands in d_status (int32 device tensor: 0 or 4) in stream order."""
    return Status(lib().xec_repair_device(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                          _ptr(d_bitmap), _ptr(d_status), _stream(stream)))


def repair_tiling_used() -> int:
    """xec_repair_tiling_used: the tiling this thread's last repair launched
    (0 none, 2 class tiles, 3 list in d_bitmap, 4 list in the kernel arguments)."""
    return int(lib().xec_repair_tiling_used())


def verify(d_data, d_parity, S: int, bs: int, k: int, m: int, d_flags, d_count=None,
           stream=None) -> Status:
    """xec_verify -- the scrub: d_flags[c*m + j] (S*m device bytes) = 1 where
    class j of stripe c no longer XORs to zero; d_count (device uint32,
    optional) = how many classes are flagged."""
    return Status(lib().xec_verify(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _ptr(d_flags),
                                   _ptr(d_count) if d_count is not None else None,
                                   _stream(stream)))


def shard_table(shards):
    """The host array of device pointers the shard calls take (h_shards): a
    ctypes ``c_void_p`` array built from a sequence of tensors or integer
    addresses, k data shards then m parity shards.  None stays None (a NULL
    table); an array built here before is passed through."""
    if shards is None or isinstance(shards, ctypes.Array):
        return shards
    return (ctypes.c_void_p * len(shards))(*[_ptr(s) for s in shards])


def check_shards(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int,
                 m: int) -> Status:
    """xec_check_shards -- the host-only check of a shard table (no GPU, no init):
    sizes, alignment, strides and the overlap rule of include/xec.h."""
    return Status(lib().xec_check_shards(shard_table(shards), data_stride, parity_stride, S, bs,
                                         k, m))


def encode_shards(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int, m: int,
                  stream=None) -> Status:
    """xec_encode_shards -- xec_encode over one buffer per shard: block c of
    shard i at shards[i] + c*stride (data_stride for the first k, parity_stride
    for the m parity shards)."""
    return Status(lib().xec_encode_shards(shard_table(shards), data_stride, parity_stride, S, bs,
                                          k, m, _stream(stream)))


def repair_shards_device(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int,
                         m: int, d_bitmap, d_status, stream=None) -> Status:
    """xec_repair_shards_device -- xec_repair_device over shards: every lost block
    (d_bitmap byte 0), data or parity, rebuilt; the verdict lands in d_status."""
    return Status(lib().xec_repair_shards_device(shard_table(shards), data_stride, parity_stride,
                                                 S, bs, k, m, _ptr(d_bitmap), _ptr(d_status),
                                                 _stream(stream)))


def verify_shards(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int, m: int,
                  d_flags, d_count=None, stream=None) -> Status:
    """xec_verify_shards -- the scrub over shards: d_flags[c*m + j] = 1 where
    class j of stripe c no longer XORs to zero; d_count (optional) = how many."""
    return Status(lib().xec_verify_shards(shard_table(shards), data_stride, parity_stride, S, bs,
                                          k, m, _ptr(d_flags),
                                          _ptr(d_count) if d_count is not None else None,
                                          _stream(stream)))


def digest_shards(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int, m: int,
                  d_digests, d_select=None, stream=None) -> Status:
    """xec_digest_shards -- xec_digest over shards: d_digests (S*(k+m) device
    uint64, the bitmap's layout) = the digest of every block, or of those
    d_select (S*(k+m) device bytes, nonzero = digest) picks."""
    return Status(lib().xec_digest_shards(shard_table(shards), data_stride, parity_stride, S, bs,
                                          k, m, _ptr(d_select) if d_select is not None else None,
                                          _ptr(d_digests), _stream(stream)))


def locate_shards(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int, m: int,
                  d_digests, d_flags, d_bitmap, d_count, d_work, work_bytes: int,
                  stream=None) -> Status:
    """xec_locate_shards -- xec_locate over shards: d_bitmap = 0 where a block's
    digest differs from d_digests, else 1 (d_flags None: every block, else the
    classes verify_shards flagged); what repair_shards_device takes."""
    return Status(lib().xec_locate_shards(shard_table(shards), data_stride, parity_stride, S, bs,
                                          k, m, _ptr(d_digests),
                                          _ptr(d_flags) if d_flags is not None else None,
                                          _ptr(d_bitmap),
                                          _ptr(d_count) if d_count is not None else None,
                                          _ptr(d_work), work_bytes, _stream(stream)))


def read_shards_device(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int,
                       m: int, d_bitmap, d_items, n_items: int, offset: int, length: int, d_out,
                       d_status, stream=None) -> Status:
    """xec_read_shards_device -- xec_read_device over shards: bytes [offset,
    offset + length) of the blocks the device items c << 8 | i name go to d_out,
    lost ones (d_bitmap byte 0; None = all present) reconstructed; the verdict
    (0, 3 or 4) lands in d_status.  Capturable."""
    return Status(lib().xec_read_shards_device(shard_table(shards), data_stride, parity_stride, S,
                                               bs, k, m,
                                               _ptr(d_bitmap) if d_bitmap is not None else None,
                                               _ptr(d_items) if d_items is not None else None,
                                               n_items, offset, length, _ptr(d_out),
                                               _ptr(d_status), _stream(stream)))


def write_shards_device(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int,
                        m: int, d_bitmap, d_items, n_items: int, offset: int, length: int, d_new,
                        d_digests, d_status, stream=None) -> Status:
    """xec_write_shards_device -- xec_write over shards with the list on the
    device: the blocks the ascending device items c << 8 | i (i < k) name take
    bytes [offset, offset + length) from d_new (item t at d_new + t*length) and
    parity follows, in the delta, data-only or rebuild-write mode d_bitmap (byte
    0 = lost; None = all present, the ranged update) asks for; d_digests (uint64
    device tensor or None) is kept current; the verdict (0, 3 or 4) lands in
    d_status.  Capturable."""
    return Status(lib().xec_write_shards_device(shard_table(shards), data_stride, parity_stride,
                                                S, bs, k, m,
                                                _ptr(d_bitmap) if d_bitmap is not None else None,
                                                _ptr(d_items) if d_items is not None else None,
                                                n_items, offset, length,
                                                _ptr(d_new) if d_new is not None else None,
                                                _ptr(d_digests) if d_digests is not None else None,
                                                _ptr(d_status), _stream(stream)))


def readv_shards_device(shards, data_stride: int, parity_stride: int, S: int, bs: int, k: int,
                        m: int, d_bitmap, d_iov, n_items: int, d_out, out_bytes: int, d_work,
                        work_bytes: int, d_status, stream=None) -> Status:
    """xec_readv_shards_device -- xec_readv_device over shards: each device entry
    (item, offset, len) delivers its range, packed in list order, to d_out;
    d_work of readv_device_work_bytes(n_items) device bytes; the verdict (0, 1,
    3 or 4) lands in d_status.  Capturable."""
    return Status(lib().xec_readv_shards_device(shard_table(shards), data_stride, parity_stride,
                                                S, bs, k, m,
                                                _ptr(d_bitmap) if d_bitmap is not None else None,
                                                _ptr(d_iov) if d_iov is not None else None,
                                                n_items, _ptr(d_out), out_bytes, _ptr(d_work),
                                                work_bytes, _ptr(d_status), _stream(stream)))


def shards_arg_capacity_used() -> int:
    """xec_shards_arg_capacity_used: the pointer capacity (64 or 256) of this
    thread's last shard call's kernel arguments; 0 if it launched nothing."""
    return int(lib().xec_shards_arg_capacity_used())


def update(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, h_items, n_items: int,
           d_scratch=None, scratch_bytes: int = 0, stream=None) -> Status:
    """xec_update -- in place: block i of stripe c takes the t-th block of d_new
    and parity[c][i % m] ^= old ^ new, for the n_items host items c << 8 | i
    (uint32, strictly ascending).  d_scratch (update_scratch_bytes(n_items)
    device bytes) is needed only past 1,024 items."""
    return Status(lib().xec_update(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs, k, m,
                                   _ptr(h_items), n_items, _ptr(d_scratch), scratch_bytes,
                                   _stream(stream)))


def update_device(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, d_mask,
                  stream=None) -> Status:
    """xec_update_device -- the same with a device mask (S*k bytes, NONZERO =
    take the block) and d_new a shadow of d_data's layout; capturable."""
    return Status(lib().xec_update_device(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs, k, m,
                                          _ptr(d_mask), _stream(stream)))


def update_scratch_bytes(n_items: int) -> int:
    """xec_update_scratch_bytes: 4 * n_items."""
    return int(lib().xec_update_scratch_bytes(n_items))


def update_tiling_used() -> int:
    """xec_update_tiling_used: the tiling this thread's last update launched
    (0 none, 2 class tiles, 3 list in d_scratch, 4 list in the kernel arguments)."""
    return int(lib().xec_update_tiling_used())


def digest_host(block) -> int:
    """xec_digest_host -- the digest of one block in host memory (a C-contiguous
    numpy array or bytes whose length is a multiple of 8): the sum over its
    little-endian u64 words w[n] of splitmix_at(w[n], n), mod 2^64.  Host only."""
    if isinstance(block, (bytes, bytearray)):
        buf = (ctypes.c_char * len(block)).from_buffer_copy(block)
        return int(lib().xec_digest_host(ctypes.addressof(buf), len(block)))
    return int(lib().xec_digest_host(_ptr(block), block.nbytes))


def digest_range_host(data, offset: int, length: int | None = None) -> int:
    """xec_digest_range_host -- the digest terms of a range: the sum over the
    little-endian u64 words w[n] of `data` (bytes or a C-contiguous numpy array
    holding the range itself) of splitmix_at(w[n], offset/8 + n), mod 2^64;
    `offset` is where the range starts in its block.  Host only."""
    if isinstance(data, (bytes, bytearray)):
        n = len(data) if length is None else length
        buf = (ctypes.c_char * len(data)).from_buffer_copy(data)
        return int(lib().xec_digest_range_host(ctypes.addressof(buf), offset, n))
    n = data.nbytes if length is None else length
    return int(lib().xec_digest_range_host(_ptr(data), offset, n))


def update_range(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, h_items,
                 n_items: int, offset: int, length: int, d_digests=None, d_scratch=None,
                 scratch_bytes: int = 0, stream=None) -> Status:
    """xec_update_range -- xec_update over bytes [offset, offset + length) of
    each named block: item t's new bytes are the `length` bytes at
    d_new + t*length.  With d_digests (S*(k+m) device uint64, xec_digest's
    layout) the slots of the touched data and parity blocks follow in the same
    pass; None touches no digest."""
    return Status(lib().xec_update_range(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs, k, m,
                                         _ptr(h_items), n_items, offset, length,
                                         _ptr(d_digests), _ptr(d_scratch), scratch_bytes,
                                         _stream(stream)))


def update_range_device(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, d_mask,
                        offset: int, length: int, d_digests=None, stream=None) -> Status:
    """xec_update_range_device -- the same with a device mask (S*k bytes,
    NONZERO = take the block) and d_new a shadow of d_data's layout; capturable."""
    return Status(lib().xec_update_range_device(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs,
                                                k, m, _ptr(d_mask), offset, length,
                                                _ptr(d_digests), _stream(stream)))


def write(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, h_bitmap, h_items,
          n_items: int, offset: int, length: int, d_digests=None, d_scratch=None,
          scratch_bytes: int = 0, stream=None) -> Status:
    """xec_write -- xec_update_range under a loss bitmap (h_bitmap byte 0 = lost;
    None = all present): a lost block is never read and never written.  A class
    whose parity is lost takes the new bytes only; a lost written block's bytes
    go into its class's parity, recomputed over the range, for a later repair to
    reconstruct.  An item that is lost with another block of its class lost is
    DECODE_FAILURE and nothing changes.  d_scratch (write_scratch_bytes(n_items)
    device bytes) is needed only past 1,024 items."""
    return Status(lib().xec_write(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs, k, m,
                                  _ptr(h_bitmap) if h_bitmap is not None else None,
                                  _ptr(h_items) if h_items is not None else None, n_items,
                                  offset, length, _ptr(d_digests), _ptr(d_scratch), scratch_bytes,
                                  _stream(stream)))


def write_device(d_data, d_parity, d_new, S: int, bs: int, k: int, m: int, d_bitmap, d_mask,
                 offset: int, length: int, d_digests, d_status, stream=None) -> Status:
    """xec_write_device -- the same with bitmap (None = all present) and mask on
    the device and d_new a shadow of d_data's layout; the verdict lands in
    d_status (int32 device tensor: 0, or 4 a marked block not servable) in
    stream order; capturable."""
    return Status(lib().xec_write_device(_ptr(d_data), _ptr(d_parity), _ptr(d_new), S, bs, k, m,
                                         _ptr(d_bitmap) if d_bitmap is not None else None,
                                         _ptr(d_mask), offset, length, _ptr(d_digests),
                                         _ptr(d_status), _stream(stream)))


def write_scratch_bytes(n_items: int) -> int:
    """xec_write_scratch_bytes: 4 * (n_items + ceil(n_items / 16))."""
    return int(lib().xec_write_scratch_bytes(n_items))


def check_write_items(h_bitmap, S: int, k: int, m: int, h_items,
                      n_items: int) -> tuple[Status, int, int]:
    """xec_check_write_items -- the host scan xec_write runs (no GPU, no init):
    (status, items that are lost, items whose class lost its parity)."""
    n_rebuild, n_data_only = ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = Status(lib().xec_check_write_items(_ptr(h_bitmap) if h_bitmap is not None else None,
                                            S, k, m,
                                            _ptr(h_items) if h_items is not None else None,
                                            n_items, ctypes.byref(n_rebuild),
                                            ctypes.byref(n_data_only)))
    return st, int(n_rebuild.value), int(n_data_only.value)


def write_tiling_used() -> int:
    """xec_write_tiling_used: the tiling this thread's last write launched (0 none,
    2 class tiles, 3 list in d_scratch, 4 list in the kernel arguments)."""
    return int(lib().xec_write_tiling_used())


def digest(d_data, d_parity, S: int, bs: int, k: int, m: int, d_digests, d_select=None,
           stream=None) -> Status:
    """xec_digest -- d_digests (S*(k+m) device uint64, the bitmap's layout) =
    the digest of every block, or with d_select (S*(k+m) device bytes, NONZERO =
    digest this block) of the selected ones only; other slots are untouched."""
    return Status(lib().xec_digest(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                   _ptr(d_select) if d_select is not None else None,
                                   _ptr(d_digests), _stream(stream)))


def locate_work_bytes(S: int, k: int, m: int) -> int:
    """xec_locate_work_bytes: 8 * S * (k+m)."""
    return int(lib().xec_locate_work_bytes(S, k, m))


def locate(d_data, d_parity, S: int, bs: int, k: int, m: int, d_digests, d_flags, d_bitmap,
           d_count, d_work, work_bytes: int, stream=None) -> Status:
    """xec_locate -- d_bitmap (S*(k+m) device bytes) = 0 where a block's digest
    differs from d_digests, else 1; d_flags None checks every block, else only
    the classes xec_verify flagged; d_count (device uint32, optional) = the
    zeros written.  d_bitmap is what repair_device takes."""
    return Status(lib().xec_locate(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _ptr(d_digests),
                                   _ptr(d_flags) if d_flags is not None else None,
                                   _ptr(d_bitmap),
                                   _ptr(d_count) if d_count is not None else None,
                                   _ptr(d_work), work_bytes, _stream(stream)))


def read(d_data, d_parity, S: int, bs: int, k: int, m: int, h_bitmap, h_items, n_items: int,
         offset: int, length: int, d_out, d_scratch=None, scratch_bytes: int = 0,
         stream=None) -> Status:
    """xec_read -- bytes [offset, offset + length) of the block each of the n_items
    host items c << 8 | i names (uint32; i >= k: parity block i - k; any order,
    repeats allowed) go to d_out + t*length; a lost block (h_bitmap byte 0;
    h_bitmap None = all present) is reconstructed from the rest of its class.
    Nothing but d_out is written.  d_scratch (read_scratch_bytes(n_items) device
    bytes) is needed only past 1,024 items."""
    return Status(lib().xec_read(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                 _ptr(h_bitmap) if h_bitmap is not None else None,
                                 _ptr(h_items) if h_items is not None else None, n_items,
                                 offset, length, _ptr(d_out), _ptr(d_scratch), scratch_bytes,
                                 _stream(stream)))


def read_device(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, d_items,
                n_items: int, offset: int, length: int, d_out, d_status, stream=None) -> Status:
    """xec_read_device -- the same with bitmap (None = all present) and items on
    the device; the verdict lands in d_status (int32 device tensor: 0, 3 an item
    out of range, 4 an item not servable) in stream order; capturable."""
    return Status(lib().xec_read_device(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                        _ptr(d_bitmap) if d_bitmap is not None else None,
                                        _ptr(d_items) if d_items is not None else None, n_items,
                                        offset, length, _ptr(d_out), _ptr(d_status),
                                        _stream(stream)))


def read_scratch_bytes(n_items: int) -> int:
    """xec_read_scratch_bytes: 4 * (n_items + ceil(n_items / 32))."""
    return int(lib().xec_read_scratch_bytes(n_items))


def check_read_items(h_bitmap, S: int, k: int, m: int, h_items, n_items: int) -> tuple[Status, int]:
    """xec_check_read_items -- the host scan xec_read runs (no GPU, no init):
    (status, items that need a reconstruction)."""
    n_lost = ctypes.c_size_t(0)
    st = Status(lib().xec_check_read_items(_ptr(h_bitmap) if h_bitmap is not None else None,
                                           S, k, m,
                                           _ptr(h_items) if h_items is not None else None,
                                           n_items, ctypes.byref(n_lost)))
    return st, int(n_lost.value)


def read_tiling_used() -> int:
    """xec_read_tiling_used: the tiling this thread's last read launched (0 none,
    3 list on the device, 4 list in the kernel arguments)."""
    return int(lib().xec_read_tiling_used())


def readv(d_data, d_parity, S: int, bs: int, k: int, m: int, h_bitmap, h_iov, n_items: int,
          d_out, out_bytes: int, d_scratch=None, scratch_bytes: int = 0, stream=None) -> Status:
    """xec_readv -- xec_read with a range per entry: h_iov is a host array of
    n_items IOV entries (item c << 8 | i, offset, len), and entry t's bytes go to
    d_out + the sum of len over the entries before it (out_bytes = d_out's
    capacity).  d_scratch (readv_scratch_bytes(n_items) device bytes) is needed
    only past 256 entries."""
    return Status(lib().xec_readv(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                  _ptr(h_bitmap) if h_bitmap is not None else None,
                                  _ptr(h_iov) if h_iov is not None else None, n_items,
                                  _ptr(d_out), out_bytes, _ptr(d_scratch), scratch_bytes,
                                  _stream(stream)))


def readv_device(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, d_iov,
                 n_items: int, d_out, out_bytes: int, d_work, work_bytes: int, d_status,
                 stream=None) -> Status:
    """xec_readv_device -- the same with bitmap (None = all present) and entries on
    the device, d_work of readv_device_work_bytes(n_items) device bytes; the
    verdict lands in d_status (int32 device tensor: 0, 1 a bad range or an
    output past out_bytes, 3 an entry out of range, 4 an entry not servable) in
    stream order; capturable."""
    return Status(lib().xec_readv_device(_ptr(d_data), _ptr(d_parity), S, bs, k, m,
                                         _ptr(d_bitmap) if d_bitmap is not None else None,
                                         _ptr(d_iov) if d_iov is not None else None, n_items,
                                         _ptr(d_out), out_bytes, _ptr(d_work), work_bytes,
                                         _ptr(d_status), _stream(stream)))


def readv_scratch_bytes(n_items: int) -> int:
    """xec_readv_scratch_bytes: 4 * (6 * n_items + 1 + ceil(n_items / 32)), 0 at 0."""
    return int(lib().xec_readv_scratch_bytes(n_items))


def readv_device_work_bytes(n_items: int) -> int:
    """xec_readv_device_work_bytes: 12 * (n_items + 1) rounded up to 8, 0 at 0."""
    return int(lib().xec_readv_device_work_bytes(n_items))


def check_readv(h_bitmap, S: int, bs: int, k: int, m: int, h_iov,
                n_items: int) -> tuple[Status, int, int]:
    """xec_check_readv -- the host plan check xec_readv runs (no GPU, no init):
    (status, entries that need a reconstruction, sum of len)."""
    n_lost, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = Status(lib().xec_check_readv(_ptr(h_bitmap) if h_bitmap is not None else None,
                                      S, bs, k, m,
                                      _ptr(h_iov) if h_iov is not None else None, n_items,
                                      ctypes.byref(n_lost), ctypes.byref(total)))
    return st, int(n_lost.value), int(total.value)


def readv_tiling_used() -> int:
    """xec_readv_tiling_used: the tiling this thread's last readv launched (0 none,
    3 table on the device, 4 table in the kernel arguments)."""
    return int(lib().xec_readv_tiling_used())


def erase(d_data, d_parity, S: int, bs: int, k: int, m: int, d_bitmap, stream=None) -> Status:
    """xec_erase -- device-side simulate_data_loss (abstract_bm.cpp:20-39)."""
    return Status(lib().xec_erase(_ptr(d_data), _ptr(d_parity), S, bs, k, m, _ptr(d_bitmap),
                                  _stream(stream)))


def fill_splitmix64(d_buf, S: int, stripe_bytes: int, seed_base: int, stream=None) -> Status:
    return Status(lib().xec_fill_splitmix64(_ptr(d_buf), S, stripe_bytes, seed_base,
                                            _stream(stream)))


def write_validation_pattern(d_data, nblocks: int, bs: int, seed: int, stream=None) -> Status:
    """xec_write_validation_pattern -- utils.cpp:35-69 on the device."""
    return Status(lib().xec_write_validation_pattern(_ptr(d_data), nblocks, bs, seed,
                                                     _stream(stream)))


def validate_blocks(d_data, nblocks: int, bs: int, d_bad, stream=None) -> Status:
    """xec_validate_blocks -- utils.cpp:72-97 on the device; *d_bad = failing blocks."""
    return Status(lib().xec_validate_blocks(_ptr(d_data), nblocks, bs, _ptr(d_bad),
                                            _stream(stream)))


def check_bitmap(h_bitmap, S: int, k: int, m: int) -> tuple[Status, bool]:
    """Host-only recoverability scan; returns (status, needs_recovery)."""
    needs = ctypes.c_int(0)
    st = Status(lib().xec_check_bitmap(_ptr(h_bitmap), S, k, m, ctypes.byref(needs)))
    return st, bool(needs.value)


def select_lost_blocks(k: int, m: int, lost: int, h_bitmap, seed: int) -> Status:
    """xec_select_lost_blocks -- utils.cpp:100-127 with an explicit seed, on one
    stripe's (k+m)-byte host bitmap (host only)."""
    return Status(lib().xec_select_lost_blocks(k, m, lost, _ptr(h_bitmap), seed))


def check_args(data_addr: int, parity_addr: int, bs: int, k: int, m: int) -> Status:
    """Host-only xorec_check_args (xorec_utils.hpp:61-86)."""
    return Status(lib().xec_check_args(data_addr, parity_addr, bs, k, m))


def set_launch(unroll: int = 0, max_grid: int = 0, cache_policy: int = 0,
               block_threads: int = 0) -> Status:
    """xec_set_launch; 0 = default for each; cache_policy 1 = nt, 2 = default policy;
    block_threads 64 or 256."""
    return Status(lib().xec_set_launch(unroll, max_grid, cache_policy, block_threads))


def set_occupancy(waves_per_simd: int = 0) -> Status:
    """xec_set_occupancy; resident encode/decode waves per SIMD (1..8, 8 = no cap),
    0 = automatic (measured per member count; the default)."""
    return Status(lib().xec_set_occupancy(waves_per_simd))


def set_decode_tiling(tiling: int = 0) -> Status:
    """xec_set_decode_tiling; 0 = automatic (default), 1 = stripe tiles, 2 = class tiles
    (m > 1 only), 3 = work-list tiles where the list fits, 4 = kernel-argument mask
    tiles where they apply (S <= 1,024, k <= 32) (identical results)."""
    return Status(lib().xec_set_decode_tiling(tiling))


def set_rotation(tiles: int = 0) -> Status:
    """xec_set_rotation: column rotation of the tile kernels (this thread)."""
    return Status(lib().xec_set_rotation(tiles))


def set_validate_kernel(mode: int = 0) -> Status:
    """xec_set_validate_kernel; 0 = automatic (default), 1 = lane per block,
    2 = wave per block (identical results)."""
    return Status(lib().xec_set_validate_kernel(mode))


#: xec_decode_tiling_used values (include/xec.h)
DECODE_KERNELS = {1: "xec::decode_kernel", 2: "xec::decode_class_kernel",
                  3: "xec::decode_list_kernel", 4: "xec::decode_arglist_kernel",
                  5: "xec::decode_argmask_kernel", 6: "xec::decode_argmask_kernel"}


def decode_tiling_used() -> int:
    """xec_decode_tiling_used: the tiling this thread's last xec_decode launched
    (0 none, 1 stripe, 2 class, 3 device list, 4 kernel-argument list,
    5 kernel-argument masks over class tiles, 6 the same over stripe tiles)."""
    return int(lib().xec_decode_tiling_used())


def set_kernel_events(start, stop) -> Status:
    """xec_set_kernel_events: the calling thread's next codec call launches its
    kernel with these events, recorded by the kernel's own dispatch
    (hipExtLaunchKernel); `start` / `stop` are torch.cuda.Event objects (or
    None).  torch creates an event's HIP handle at its first record(), so each
    must have been recorded once before."""
    def handle(ev):
        if ev is None:
            return None
        h = int(ev.cuda_event)
        if not h:
            raise ValueError("record the torch.cuda.Event once before handing it over")
        return ctypes.c_void_p(h)
    return Status(lib().xec_set_kernel_events(handle(start), handle(stop)))


def decode_arg_capacity_used() -> int:
    """xec_decode_arg_capacity_used: after a kernel-argument list decode, the
    capacity its arguments carried (64, 256 or 1024 entries); else 0."""
    return int(lib().xec_decode_arg_capacity_used())


def status_string(st: int) -> str:
    return lib().xec_status_string(int(st)).decode()


def build_info() -> str:
    return lib().xec_build_info().decode()


class Pipeline:
    """Host-in / host-out encoder-decoder (xec_pipeline_*, include/xec.h).

    Owns ``nstreams`` device slots of ``chunk_stripes`` stripes on the current
    device; host buffers (numpy arrays, pinned torch tensors or addresses) are
    streamed through them.  Use as a context manager or call :meth:`close`."""

    def __init__(self, chunk_stripes: int, bs: int, k: int, m: int, nstreams: int = 2):
        self.bs, self.k, self.m = bs, k, m
        h = ctypes.c_void_p()
        st = Status(lib().xec_pipeline_create(ctypes.byref(h), chunk_stripes, bs, k, m, nstreams))
        if st != Status.SUCCESS:
            raise RuntimeError(f"xec_pipeline_create failed: {st!r}")
        self._h = h

    def encode(self, h_data, h_parity, S: int) -> Status:
        return Status(lib().xec_pipeline_encode(self._h, _ptr(h_data), _ptr(h_parity), S))

    def decode(self, h_data, h_parity, S: int, h_bitmap) -> Status:
        return Status(lib().xec_pipeline_decode(self._h, _ptr(h_data), _ptr(h_parity), S,
                                                _ptr(h_bitmap)))

    def close(self) -> None:
        if self._h:
            lib().xec_pipeline_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter teardown
            pass
