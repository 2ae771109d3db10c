// xec_internal.h -- host-side helpers shared inside libxec_hip.so (plain C++,
// no HIP types, so xec_scan.cpp still builds without the HIP device pass).
// Not part of the public boundary (include/xec.h).
#pragma once

#include <cstddef>
#include <cstdint>

#include "xec.h"

// One decode work item: a lost data block, stripe c, block i (i < k <= 256,
// c < 2^24), packed as c << 8 | i (xec_kernels.hip decode_list_kernel).
constexpr size_t kWorkItemMaxK = 256;
constexpr size_t kWorkItemMaxStripes = size_t(1) << 24;
inline uint32_t xec_work_item(size_t c, size_t i) {
  return static_cast<uint32_t>(c << 8) | static_cast<uint32_t>(i);
}

// What one host pass over a batch bitmap finds (xec_scan_bitmap).
struct XecScan {
  int needs_recovery = 0;     // require_recovery over the batch (bit 0 of a data byte clear)
  uint64_t lost_data = 0;     // zero data bytes
  uint64_t stripes_lost = 0;  // stripes with at least one zero data byte
  int64_t lost_class = -1;    // the parity class every lost data block is in, or -1
                              // (none lost, or several classes): one failed device
  uint64_t listed = 0;        // work items written; the list is whole iff == lost_data
};

// xec_check_bitmap plus the counts above (out may be null) and, when `items`
// is non-null, the first `cap` lost data blocks as work items in batch order
// (requires k <= kWorkItemMaxK and S <= kWorkItemMaxStripes).  `speculative`:
// the caller may not need the list at all, so listing stops once the losses
// seen so far, projected over the batch, say it will not be used -- more than
// `cap` of them, or a batch dense enough for class tiles (lost > S and
// 2 * lost >= S * m, xec_api.cpp use_class_tiles) -- and out->listed tells how
// many were written.  Defined in xec_scan.cpp.
xec_status xec_scan_bitmap(const uint8_t* h_bitmap, size_t S, size_t k, size_t m, XecScan* out,
                           uint32_t* items, uint64_t cap, bool speculative = false);

// Per-stripe form (the reference CPU plugin's loop, xorec_bm.cpp:43-58 over
// xorec_decode, xorec.cpp:62-111): codes[c] (if non-null) = 0 or 4
// (DecodeFailure) for every stripe; *failures = stripes with 4; work items
// (first `cap` to `items`) and *n_items only for stripes that need recovery
// and are recoverable.  XEC_INVALID_COUNTS as xec_check_args, else success.
xec_status xec_scan_stripes(const uint8_t* h_bitmap, size_t S, size_t k, size_t m,
                            uint8_t* codes, uint32_t* items, uint64_t cap, uint64_t* n_items,
                            uint64_t* failures);

// Repair scan (xec_repair): lists EVERY lost block of the batch, data and
// parity alike, as work items c << 8 | i with i in [0, k+m) -- i >= k is parity
// block i - k -- in batch order; the first `cap` go to `items` (may be null with
// cap 0) and *n_items is their total.  A block is lost iff its byte is 0; the
// bit-0 rule of require_recovery plays no part.  XEC_DECODE_FAILURE if some
// class of some stripe lost two blocks (is_recoverable; items and *n_items are
// then unspecified), XEC_INVALID_COUNTS as xec_check_args, XEC_INVALID_SIZE
// unless k + m <= kRepairItemMaxRow and S <= kWorkItemMaxStripes.  Defined in
// xec_scan.cpp.
constexpr size_t kRepairItemMaxRow = 256;
xec_status xec_scan_repair(const uint8_t* h_bitmap, size_t S, size_t k, size_t m, uint32_t* items,
                           uint64_t cap, uint64_t* n_items);

// Read scan (xec_read; xec_check_read_items is this with lost_bits null): the
// verdict over the n_items REQUESTED items c << 8 | i, i in [0, k+m).  An item
// is servable if its block is present (byte != 0, or bm null), or lost with
// every other block of its class present; other classes and stripes play no
// part.  XEC_INVALID_COUNTS if any item has c >= S or i >= k + m (or k, m as
// xec_check_args, or items null with n_items > 0), else XEC_DECODE_FAILURE if
// any is not servable.  On success *n_lost (may be null) = the items that need
// a reconstruction (a repeated item counts each time) and, when lost_bits is
// non-null, bit t of word t / 32 of its (n_items + 31) / 32 words = item t is
// lost.  Defined in xec_scan.cpp.
xec_status xec_scan_read_items(const uint8_t* bm, size_t S, size_t k, size_t m,
                               const uint32_t* items, size_t n_items, uint32_t* lost_bits,
                               size_t* n_lost);

// Vectored read plan (xec_readv, xec_check_readv): the verdict over n entries
// that each bring their own range, and the table the readv kernels walk
// (xec_kernels.hip).  A tile is (entry, chunk of tile_bytes of the entry's
// range), tile_bytes = 16 * threads * unroll of the call's launch shape.
//
// The table is u32 words in six columns of `cap` >= n entries each, so that
// the copy in the kernel arguments (cap = the compiled capacity) and the
// uploaded one (cap = n) are read by the same code:
//   [0, cap]                 tile start: exclusive prefix of ceil(len / tile_bytes),
//                            word n = the total (n + 1 values; the rest 0)
//   [cap + 1, 2 cap + 1)     item   c << 8 | i
//   [2 cap + 1, 3 cap + 1)   offset
//   [3 cap + 1, 4 cap + 1)   len
//   [4 cap + 1, 5 cap + 1)   output start, low word   (exclusive prefix of len)
//   [5 cap + 1, 6 cap + 1)   output start, high word
//   [6 cap + 1, + ceil(cap / 32))  bit t of word t / 32 = entry t is lost
// xec_readv_table_words(cap) words in all; columns past n are zeroed.
constexpr size_t xec_readv_table_words(size_t cap) {
  return cap ? 6 * cap + 1 + (cap + 31) / 32 : 0;
}

struct XecReadvPlan {
  xec_status range_status = XEC_SUCCESS;  // XEC_INVALID_SIZE if an entry has len == 0, offset or
                                          // len % 16 != 0, or offset + len > bs (64-bit sum)
  xec_status items_status = XEC_SUCCESS;  // else XEC_INVALID_COUNTS (c >= S or i >= k + m), else
                                          // XEC_DECODE_FAILURE (xec_scan_read_items' rule)
  size_t n_lost = 0;          // entries that need a reconstruction, a repeat counted each time
  uint64_t total_bytes = 0;   // sum of len
  uint64_t total_tiles = 0;   // sum of ceil(len / tile_bytes); may pass 32 bits (the table's
                              // tile column is then truncated and must not be used)
};

// Returns the first of range_status and items_status that is not success (k, m
// invalid as xec_check_args, or iov null with n > 0: XEC_INVALID_COUNTS with
// both fields set to it).  The totals are valid when range_status is success,
// n_lost and the table when the return value is.  `table` may be null (verdict
// and totals only); else it holds xec_readv_table_words(cap) words, cap >= n.
// tile_bytes > 0.  Defined in xec_scan.cpp.
xec_status xec_plan_readv(const uint8_t* bm, size_t S, size_t bs, size_t k, size_t m,
                          const xec_iov* iov, size_t n, size_t tile_bytes, size_t cap,
                          uint32_t* table, XecReadvPlan* plan);

// Write scan (xec_write; xec_check_write_items is this with bits null): the
// verdict over the n_items WRITTEN items c << 8 | i, i < k, strictly ascending.
// XEC_INVALID_COUNTS if any item breaks xec_update's item rules (i >= k,
// c >= S, not ascending; or k, m as xec_check_args, or items null with
// n_items > 0) anywhere in the list, else XEC_DECODE_FAILURE if any item is not
// servable (xec_scan_read_items' rule).  On success *n_rebuild (may be null) =
// the lost items, *n_data_only (may be null) = the items whose class lost its
// parity block, and, when bits is non-null, its (n_items + 15) / 16 words hold
// two bits per item, item t at bits 2*(t % 16) of word t / 16: bit 0 = the
// block is lost, bit 1 = its class's parity block is lost.  Defined in
// xec_scan.cpp.
xec_status xec_scan_write_items(const uint8_t* bm, size_t S, size_t k, size_t m,
                                const uint32_t* items, size_t n_items, uint32_t* bits,
                                size_t* n_rebuild, size_t* n_data_only);

// masks[c] = bit i set iff data byte i of stripe c's row is 0 (lost), for the
// kernel-argument mask decode (xec_kernels.hip decode_argmask_kernel).
// Requires k <= 32; the rows must already have passed xec_scan_bitmap (no
// checks here).  Defined in xec_scan.cpp.
void xec_loss_masks(const uint8_t* h_bitmap, size_t S, size_t k, size_t m, uint32_t* masks);
