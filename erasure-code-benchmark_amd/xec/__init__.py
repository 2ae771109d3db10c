"""xec -- MI355X-native XOR-EC encode / single-erasure decode (Python view).

The hot path is libxec_hip.so (hand-written gfx950 HIP kernels behind the C ABI
of include/xec.h).  This package only binds it for tests, bench.py and the
multi-GPU partitioning helpers; it never computes parity itself.
"""
from ._lib import EXPORTED, LIB_PATH, Status, XecLibraryError, lib
from .codec import (DECODE_KERNELS, Pipeline, build_info, check_args, check_bitmap, decode,
                    decode_arg_capacity_used, decode_device, decode_device_list,
                    decode_per_stripe, decode_tiling_used,
                    device_list_bytes, digest, digest_host, encode, erase,
                    fill_splitmix64, init, locate, locate_work_bytes, repair, repair_device, repair_tiling_used,
                    check_read_items, read, read_device, read_scratch_bytes, read_tiling_used,
                    IOV, check_readv, readv, readv_device, readv_device_work_bytes,
                    readv_scratch_bytes, readv_tiling_used,
                    select_lost_blocks, set_decode_tiling, set_kernel_events, set_launch,
                    set_occupancy,
                    set_rotation, set_validate_kernel,
                    status_string, update, update_device, update_scratch_bytes,
                    update_tiling_used, validate_blocks, verify, write_validation_pattern,
                    digest_range_host, update_range, update_range_device,
                    check_write_items, write, write_device, write_scratch_bytes,
                    write_tiling_used,
                    check_shards, encode_shards, repair_shards_device, shard_table,
                    shards_arg_capacity_used, verify_shards,
                    digest_shards, locate_shards, read_shards_device,
                    readv_shards_device, write_shards_device)
from .partition import stripe_range

__all__ = [
    "DECODE_KERNELS", "EXPORTED", "LIB_PATH", "Pipeline", "Status", "XecLibraryError", "lib",
    "build_info", "check_args", "check_bitmap", "decode", "decode_arg_capacity_used",
    "decode_device", "decode_device_list",
    "decode_per_stripe", "decode_tiling_used", "device_list_bytes", "digest", "digest_host",
    "encode", "erase", "fill_splitmix64", "init", "locate", "locate_work_bytes", "repair",
    "repair_device",
    "repair_tiling_used", "check_read_items", "read", "read_device", "read_scratch_bytes",
    "read_tiling_used", "IOV", "check_readv", "readv", "readv_device",
    "readv_device_work_bytes", "readv_scratch_bytes", "readv_tiling_used", "select_lost_blocks", "set_decode_tiling",
    "set_kernel_events",
    "set_launch",
    "set_occupancy", "set_rotation", "set_validate_kernel", "status_string", "stripe_range",
    "update", "update_device", "update_scratch_bytes", "update_tiling_used", "validate_blocks",
    "verify", "write_validation_pattern",
    "digest_range_host", "update_range", "update_range_device",
    "check_write_items", "write", "write_device", "write_scratch_bytes", "write_tiling_used",
    "check_shards", "encode_shards", "repair_shards_device", "shard_table",
    "shards_arg_capacity_used", "verify_shards",
    "digest_shards", "locate_shards", "read_shards_device",
    "readv_shards_device", "write_shards_device",
]
