// xec_kernels.h -- internal interface between the C ABI (xec_api.cpp) and the
// gfx950 kernels (xec_kernels.hip).  Not part of the public boundary.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <cstdint>

#include "xec_dispatch.h"

namespace xec {

// Batch geometry.  A tile is one class of one stripe over threads*unroll
// 16-byte granules of the block.
struct Geometry {
  uint64_t S;                // stripes
  uint64_t k, m, nm;         // data blocks, parity blocks, members per class (k/m)
  uint64_t bs;               // bytes per block
  uint64_t tiles_per_block;  // ceil(bs / (16 * threads * unroll))
  uint64_t total_tiles;      // S * m * tiles_per_block
  const int32_t* gate;       // decode only: skip all work if *gate != 0 (nullptr = no gate)
  uint64_t rot;              // column rotation: stripe c's chunk q covers column chunk
                             // (q + c*rot) mod tiles_per_block (0 = none; xec_set_rotation)
};

struct LaunchShape {
  int threads;        // workgroup size: 64 (one wave) or 256
  int unroll;         // granules per lane per class member: 1 or 2
  uint32_t max_grid;  // 0 = one workgroup per tile, else grid-stride over tiles
  bool nt;            // non-temporal loads/stores
  uint32_t lds_bytes; // LDS reserved per workgroup to cap residency (0 = none)
  uint32_t rot = 0;   // column rotation in tiles per stripe (Geometry::rot)
};

inline Geometry make_geometry(uint64_t S, uint64_t bs, uint64_t k, uint64_t m,
                              const LaunchShape& ls) {
  Geometry g;
  g.S = S;
  g.k = k;
  g.m = m;
  g.nm = k / m;
  g.bs = bs;
  const uint64_t tile_bytes = 16ull * (uint64_t)ls.threads * (uint64_t)ls.unroll;
  g.tiles_per_block = (bs + tile_bytes - 1) / tile_bytes;
  g.total_tiles = S * m * g.tiles_per_block;
  g.gate = nullptr;
  g.rot = g.tiles_per_block > 1 ? ls.rot % g.tiles_per_block : 0;
  return g;
}

// Workgroups for `work_items` tiles of a grid-stride kernel: one per tile up
// to max_grid (0 = no cap of the caller's) and never beyond what HIP accepts,
// gridDim.x * blockDim.x <= 2^32 - 1; the kernels' grid-stride loops cover the
// rest.
inline uint32_t grid_for(uint64_t work_items, uint32_t max_grid, uint32_t threads) {
  const uint64_t hw = 0xFFFFFFFFull / (threads ? threads : 1);
  const uint64_t cap = max_grid && max_grid < hw ? (uint64_t)max_grid : hw;
  const uint64_t grid = work_items < cap ? work_items : cap;
  return (uint32_t)(grid ? grid : 1);
}

// splitmix64.  splitmix_at(seed, n) is output n of the stream whose state
// starts at `seed` (xec_fill_splitmix64), and the term of word n of a block in
// its digest (xec_digest, include/xec.h): for fixed n a bijection of `seed`.
// splitmix_mix is the finaliser alone, for callers that keep (n+1)*golden as a
// running sum.  Host and device: xec_digest_host is the same code.
constexpr uint64_t kSplitmixGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t splitmix_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t n) {
  return splitmix_mix(seed + (n + 1) * kSplitmixGolden);
}

// Test hook: XEC_TEST_FAIL_LAUNCH=1 in the environment (read once) makes every
// kernel launch of the library invalid (2048 threads per workgroup), so that a
// test sees the wrappers report a genuine launch failure while an error of the
// caller's with the same code is pending (tests/host/error_preserve.cpp).
bool fail_launch_for_test();

// xec_set_kernel_events: events the next codec kernel launch of this thread
// records from its own dispatch (hipExtLaunchKernel), then forgets.  Set by
// the ABI call, cleared when the codec call that follows returns
// (KernelEventsScope, xec_api.cpp), consumed by launch_codec below.
struct KernelEvents {
  hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local KernelEvents t_kernel_events;

template <typename T>
struct NoDeduce {
  using type = T;
};

// Launches `kernel` and returns THIS launch's status, from hipLaunchKernel
// itself.  The thread's pending error is neither read nor cleared: one the
// caller left unread stays theirs (a successful launch does not touch it,
// tools/lab/last_error_probe.hip, profiles/r05b), and a failed launch is
// reported whatever was pending before (comparing the pending
// error before and after took a failure with the caller's code for success).
template <typename... P>
hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, uint32_t lds, hipStream_t s,
                  typename NoDeduce<P>::type... args) {
  void* argv[] = {static_cast<void*>(&args)...};
  if (fail_launch_for_test()) block = dim3(2048);
  return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, argv, lds, s);
}

// The codec kernels (encode, every decode, repair and update tiling, verify,
// digest, read, ranged update, degraded write, the shard-layout kernels) go through this: as launch(), but with the thread's pending kernel events,
// if any, recorded by the kernel's dispatch itself and then cleared.
template <typename... P>
hipError_t launch_codec(void (*kernel)(P...), dim3 grid, dim3 block, uint32_t lds, hipStream_t s,
                        typename NoDeduce<P>::type... args) {
  const KernelEvents ev = t_kernel_events;
  if (ev.start == nullptr && ev.stop == nullptr)
    return launch(kernel, grid, block, lds, s, args...);
  t_kernel_events = KernelEvents{};
  void* argv[] = {static_cast<void*>(&args)...};
  if (fail_launch_for_test()) block = dim3(2048);
  return hipExtLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, argv, lds, s,
                            ev.start, ev.stop, 0);
}

hipError_t launch_encode(const void* d_data, void* d_parity, const Geometry& g,
                         const LaunchShape& ls, hipStream_t s);
// Decode tilings.  Stripe: one tile per (stripe, chunk), d_bitmap = the batch
// bitmap.  Class: one per (stripe, class, chunk), d_bitmap = the bitmap.
// List: one per (work item, chunk), d_bitmap = n_items u32 work items
// (xec_internal.h xec_work_item), 4-byte aligned.
// ArgList: list tiles over up to kArgItems work items passed by value in the
// kernel arguments (h_items, host memory, read at launch): no copy at all.
// ArgMask (below): class or stripe tiles, the losses by value in the kernel
// arguments.
constexpr int kDecodeStripeTiles = 0;
constexpr int kDecodeClassTiles = 1;
constexpr int kDecodeListTiles = 2;
constexpr int kDecodeArgListTiles = 3;
// DevList: list tiles over a list the device built (launch_scan_list):
// d_bitmap = the u32 list, [0] = entry count, entries from [kDevListHeader];
// n_items = the most entries there can be (sizes the grid with ls.max_grid;
// g.gate must be set).
constexpr int kDecodeDevListTiles = 4;
constexpr uint32_t kDevListHeader = 1;  // u32 words before the first entry
// ArgMask: class tiles (stripe, class, chunk) over S <= kArgItems stripes whose
// losses travel in the kernel arguments as one mask per stripe (h_items[c] bit
// i = data block i lost; k <= kArgMaskMaxK), n_items = S: a small decode with
// any number of losses copies nothing to the device.  ArgMaskStripe: the same
// masks over stripe tiles (stripe, chunk).
constexpr int kDecodeArgMaskTiles = 5;
constexpr int kDecodeArgMaskStripeTiles = 6;
constexpr uint64_t kArgMaskMaxK = 32;
// The list travels in the kernel arguments, so a launch ships the whole array
// whatever the list's length: each kernel that takes one is compiled for three
// capacities and the launch picks the smallest that holds the list
// (arg_items_capacity and with_capacity, xec_dispatch.h).
// A kernel with 4 KiB of arguments costs 0.15-0.4 us more per synchronous call
// than the same kernel with 256 B (tools/latency, profiles/r06b): small, but
// free to avoid.
constexpr uint64_t kArgItems = 1024;  // the largest capacity
template <uint32_t N>
struct ArgItems {
  uint32_t v[N];
};
hipError_t launch_decode(void* d_data, const void* d_parity, const uint8_t* d_bitmap,
                         const Geometry& g, const LaunchShape& ls, int tiling, hipStream_t s,
                         uint64_t n_items = 0, const uint32_t* h_items = nullptr);
// Repair tilings (xec_repair, xec_repair_device): every lost block, data or
// parity, is rebuilt from the other members of its class.  Class: one tile per
// (stripe, class, chunk), d_bitmap = the batch bitmap (any k, m; g.gate set by
// xec_repair_device).  List / ArgList: one per (work item, chunk) as the decode
// tilings of the same name, an item c << 8 | i with i in [0, k+m), i >= k
// naming parity block i - k (k + m <= 256).
constexpr int kRepairClassTiles = 0;
constexpr int kRepairListTiles = 1;
constexpr int kRepairArgListTiles = 2;
hipError_t launch_repair(void* d_data, void* d_parity, const uint8_t* d_bitmap,
                         const Geometry& g, const LaunchShape& ls, int tiling, hipStream_t s,
                         uint64_t n_items = 0, const uint32_t* h_items = nullptr);
// Update tilings (launch_update_range, launch_write): data block i of stripe c
// takes new bytes and parity[c][i % m] ^= old ^ new; one tile folds every
// updated member of its (stripe, class, chunk), so each parity granule has one
// writer.  Class: one tile per (stripe, class, chunk), d_sel = the S*k mask
// bytes (nonzero = take the block), d_new mirrors d_data (any k, S).  List /
// ArgList: one per (list position, chunk) over items c << 8 | i (i < k <= 256),
// strictly ascending (the caller checked), d_new = the new bytes packed in list
// order; d_sel = the n_items u32 items on the device (4-byte aligned), or
// h_items passed by value (at most kArgItems).  No member-count template
// parameter.
constexpr int kUpdateClassTiles = 0;
constexpr int kUpdateListTiles = 1;
constexpr int kUpdateArgListTiles = 2;
// Scrub (xec_verify): class tiles; d_flags[c*m + j] = 1 where the XOR of class
// j's data blocks and its parity block is nonzero anywhere (the caller zeroes
// d_flags first, stream-ordered).  Reads the batch, writes only those bytes.
hipError_t launch_verify(const void* d_data, const void* d_parity, uint8_t* d_flags,
                         const Geometry& g, const LaunchShape& ls, hipStream_t s);
// *d_count += the nonzero bytes among d_flags[0, n) (the caller zeroes it first).
hipError_t launch_count_flags(const uint8_t* d_flags, uint64_t n, uint32_t* d_count,
                              hipStream_t s);
// Block digests (xec_digest, xec_locate): d_out[c*(k+m) + i] = the digest of
// block i of stripe c (i >= k: parity block i - k) for every wanted block;
// other slots are neither read nor written.  The wanted slots are zeroed here
// first (a memset for kDigestAll, else a small kernel), then one kernel over
// (block, segment) tiles adds each segment's sum into its slot with one
// atomicAdd.  Of ls only threads, nt, max_grid and lds_bytes apply.
//   kDigestAll     every block (d_gate unused);
//   kDigestSelect  d_gate = S*(k+m) bytes, nonzero = wanted;
//   kDigestFlags   d_gate = xec_verify's S*m flags, a block is wanted iff its
//                  class's flag is nonzero.
// The segment size was swept once (16, 64 and 256 KiB; the figures stand with
// the launch shape in xec_api.cpp digest_launch_shape, DESIGN.md §3 *Locate*).
constexpr int kDigestAll = 0;
constexpr int kDigestSelect = 1;
constexpr int kDigestFlags = 2;
constexpr uint64_t kDigestSegmentBytes = 64u << 10;
hipError_t launch_digest(const void* d_data, const void* d_parity, const uint8_t* d_gate, int mode,
                         uint64_t* d_out, const Geometry& g, const LaunchShape& ls, hipStream_t s);
// d_bitmap[b] = 0 where slot b was checked (d_flags == nullptr: every slot,
// else its class's flag nonzero) and d_fresh[b] != d_stored[b], else 1;
// *d_count (may be nullptr; the caller zeroes it first) += the zeros written.
hipError_t launch_locate_compare(const uint64_t* d_fresh, const uint64_t* d_stored,
                                 const uint8_t* d_flags, uint8_t* d_bitmap, uint32_t* d_count,
                                 const Geometry& g, hipStream_t s);
// Degraded read (xec_read, xec_read_device): bytes [offset, offset + len) of
// the block each item names (c << 8 | i, i in [0, k+m), i >= k parity block
// i - k; any order, repeats allowed) go to d_out + t*len for the t-th item.  A
// tile is (item, chunk of the RANGE), chunks of 16*threads*unroll bytes; a
// present block's tile copies, a lost block's tile runs its class's reduction
// over the same range of the other k/m blocks straight into d_out.  Nothing
// but d_out is written, and a lost block is never read.  offset, len % 16 == 0,
// offset + len <= bs, k + m <= 256.  Of g only S, k, m, nm, bs and gate are
// used (the tile counts are the range's, and there is no column rotation: an
// item's chunks are one short run, not a walk down every stripe's column).
// Where the verdict (copy or reconstruct) comes from:
//   kReadArgListTiles  h_items and h_lost (bit t of word t / 32 = item t is
//                      lost) by value in the kernel arguments, n <= kArgItems;
//   kReadListTiles     d_items = n u32 items followed by (n + 31) / 32 u32 words
//                      of the same bits (read_list_words(n) words in all);
//   kReadDevTiles      d_items = n u32 items, d_bitmap = the batch bitmap (byte
//                      0 = lost) or nullptr (everything present); g.gate set.
constexpr int kReadListTiles = 0;
constexpr int kReadArgListTiles = 1;
constexpr int kReadDevTiles = 2;
inline uint64_t read_list_words(uint64_t n) { return n + (n + 31) / 32; }
hipError_t launch_read(const void* d_data, const void* d_parity, void* d_out, const Geometry& g,
                       const LaunchShape& ls, int tiling, uint64_t offset, uint64_t len,
                       uint64_t n_items, const uint32_t* d_items, const uint8_t* d_bitmap,
                       const uint32_t* h_items, const uint32_t* h_lost, hipStream_t s);
// xec_read_device's verdict: *d_status = max over the n items of 0 (servable),
// 3 (c >= S or i >= k + m; never dereferenced) and 4 (lost, and another block
// of its class lost too).  The caller zeroes *d_status first, stream-ordered.
hipError_t launch_read_check(const uint8_t* d_bitmap, const uint32_t* d_items, uint64_t n,
                             const Geometry& g, int32_t* d_status, hipStream_t s);
// Vectored read (xec_readv, xec_readv_device): launch_read with a range and an
// output start per entry.  A tile is (entry, chunk of the entry's range), and
// entry e owns tiles [tile[e], tile[e + 1]); n entries, n < 2^32.  Of g only S,
// k, m, nm, bs and gate are used.  Where the schedule comes from:
//   kReadArgListTiles  h_table = the table of xec_plan_readv (xec_internal.h)
//                      laid out for cap = readv_capacity(n), by value in the
//                      kernel arguments, n <= kReadvArgEntries;
//   kReadListTiles     d_table = the same table laid out for cap = n,
//                      xec_readv_table_words(n) words;
//   kReadDevTiles      d_table = the n entries themselves (xec_iov: item,
//                      offset, len), d_bitmap = the batch bitmap or nullptr,
//                      d_work = readv_work_words(n) words, 8-byte aligned: n + 1
//                      64-bit output starts, then n + 1 tile starts, [n] = the
//                      totals (launch_readv_check, then launch_readv_scan);
//                      g.gate set.
// `tiles` sizes the grid (with ls.max_grid): the total of the table, or for
// kReadDevTiles the most the device's total can be.
constexpr uint64_t kReadvArgEntries = 256;  // the largest capacity (xec_dispatch.h)
inline uint64_t readv_work_words(uint64_t n) { return 3 * (n + 1); }
hipError_t launch_readv(const void* d_data, const void* d_parity, void* d_out, const Geometry& g,
                        const LaunchShape& ls, int tiling, uint64_t n, uint64_t tiles,
                        const uint32_t* d_table, const uint32_t* h_table, hipStream_t s,
                        const uint8_t* d_bitmap = nullptr, const uint32_t* d_work = nullptr);
// xec_readv_device's verdict and schedule.  Check: *d_status = max over the n
// entries of 0 (servable), 1 (a broken range), 3 (c >= S or i >= k + m) and 4
// (not servable), and each entry's length and tile count (of tile_bytes) into
// d_work.  Scan: those into exclusive prefixes in list order with the totals at
// [n], and *d_status raised to 1 if the bytes exceed out_bytes.  The caller
// zeroes *d_status first, stream-ordered.
hipError_t launch_readv_check(const uint8_t* d_bitmap, const uint32_t* d_iov, uint64_t n,
                              const Geometry& g, uint64_t tile_bytes, uint32_t* d_work,
                              int32_t* d_status, hipStream_t s);
hipError_t launch_readv_scan(uint32_t* d_work, uint64_t n, uint64_t out_bytes, int32_t* d_status,
                             hipStream_t s);
// Update and ranged update (xec_update, xec_update_device, xec_update_range,
// xec_update_range_device): the delta fold over bytes [offset, offset + len) of
// each named block only -- offset = 0, len = bs and no digests for the
// whole-block calls -- with tilings and d_sel / h_items as kUpdate*Tiles
// describes; a tile is (list position or class, chunk of the RANGE), chunks of
// 16*threads*unroll bytes.  List forms: item t's new bytes are the len bytes at
// d_new + t*len; class form: d_new mirrors d_data.
// d_digests != nullptr (S*(k+m) u64, xec_digest's layout) adds
// mix(new) - mix(old) over the range's words to the slot of every updated data
// block and of the parity block of every class with an item, one 64-bit
// atomicAdd per wave and slot; nullptr launches instantiations without any of
// it.  offset, len % 16 == 0, len > 0, offset + len <= bs.  Of g only S, k, m,
// nm and bs are used; no column rotation.
hipError_t launch_update_range(void* d_data, void* d_parity, const void* d_new, const void* d_sel,
                               uint64_t* d_digests, const Geometry& g, const LaunchShape& ls,
                               int tiling, uint64_t offset, uint64_t len, hipStream_t s,
                               uint64_t n_items = 0, const uint32_t* h_items = nullptr);
// Degraded write (xec_write, xec_write_device): launch_update_range under a
// loss bitmap -- a lost block is never read and never written.  Tilings, d_sel,
// h_items, d_new's packing, the range and d_digests as there (kUpdate*Tiles).
// The tile that owns a (stripe, class) runs it in one of three modes: delta
// (parity present, no written member lost: the ranged update), data-only
// (parity lost: written members take their bytes, parity untouched) or
// rebuild (one written member lost, the rest of the class present: parity's
// range recomputed from new and unwritten members, the lost block untouched).
// Where the mode comes from:
//   kUpdateArgListTiles  h_bits by value beside h_items: two bits per item, 16
//                        items per word, bit 0 = this block is lost, bit 1 =
//                        its class's parity block is lost (n <= kArgItems);
//   kUpdateListTiles     d_sel = n u32 items followed by (n + 15) / 16 words of
//                        the same bits (write_list_words(n) words in all);
//   kUpdateClassTiles    d_sel = the S*k mask bytes, d_bitmap = the batch bitmap
//                        (byte 0 = lost) or nullptr (everything present); g.gate
//                        must be set (launch_write_check's verdict).
// Every item must be servable (the caller or the check kernel saw to it).
inline uint64_t write_list_words(uint64_t n) { return n + (n + 15) / 16; }
hipError_t launch_write(void* d_data, void* d_parity, const void* d_new, const void* d_sel,
                        const uint8_t* d_bitmap, uint64_t* d_digests, const Geometry& g,
                        const LaunchShape& ls, int tiling, uint64_t offset, uint64_t len,
                        hipStream_t s, uint64_t n_items = 0, const uint32_t* h_items = nullptr,
                        const uint32_t* h_bits = nullptr);
// xec_write_device's verdict: *d_status = 4 if a marked block is lost while
// another block of its class is lost.  The caller zeroes *d_status first,
// stream-ordered; d_bitmap == nullptr launches nothing.
hipError_t launch_write_check(const uint8_t* d_bitmap, const uint8_t* d_mask, const Geometry& g,
                              int32_t* d_status, hipStream_t s);
// Shard-major layout (xec_encode_shards, xec_repair_shards_device,
// xec_verify_shards): encode, the class-tile repair and the scrub over one
// buffer per shard instead of the batch layout.  h_shards = k + m device
// pointers in host memory, the k data shards then the m parity shards, read at
// launch and passed by value in the kernel arguments (ShardTab, capacity 64 or
// 256 by shard_tab_capacity, xec_dispatch.h; k + m <= kShardPtrs): nothing is
// copied.  Data block i of stripe c is at h_shards[i] + c*dstride, parity block
// j at h_shards[k + j] + c*pstride; the caller checked alignment, strides and
// overlap (xec_check_shards).  Tiles, g and ls as launch_encode / launch_repair
// with kRepairClassTiles (g.gate must be set; d_bitmap = the batch bitmap) /
// launch_verify (the caller zeroes d_flags first).
constexpr uint64_t kShardPtrs = 256;  // the largest capacity
template <uint32_t N>
struct ShardTab {
  uint8_t* v[N];
};
hipError_t launch_encode_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const Geometry& g, const LaunchShape& ls, hipStream_t s);
hipError_t launch_repair_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const uint8_t* d_bitmap, const Geometry& g, const LaunchShape& ls,
                                hipStream_t s);
hipError_t launch_verify_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                uint8_t* d_flags, const Geometry& g, const LaunchShape& ls,
                                hipStream_t s);
// launch_digest and launch_read with kReadDevTiles (g.gate must be set) over a
// shard table: arguments, zeroing, tiles and grid as there, a block's address
// from the table.  launch_locate_compare and launch_read_check touch no block
// and serve both layouts.
hipError_t launch_digest_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const uint8_t* d_gate, int mode, uint64_t* d_out,
                                const Geometry& g, const LaunchShape& ls, hipStream_t s);
hipError_t launch_read_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                              void* d_out, const Geometry& g, const LaunchShape& ls,
                              uint64_t offset, uint64_t len, uint64_t n_items,
                              const uint32_t* d_items, const uint8_t* d_bitmap, hipStream_t s);
// Shard-major degraded write (xec_write_shards_device): launch_write's list
// tiles over a shard table with list and bitmap on the device.  d_items = n_items
// u32 items c << 8 | i, d_new = their new bytes packed in list order, d_bitmap
// the batch bitmap or nullptr (everything present), d_digests as launch_write;
// the owning tile reads its class's two loss bytes from the bitmap.  g.gate
// must be set to the verdict of launch_write_items_check, which leaves
// *d_status = max over the items of 0, 3 (c >= S, i >= k, or not above its
// predecessor) and 4 (lost with another block of its class lost); the caller
// zeroes *d_status first, stream-ordered.  The check runs with d_bitmap ==
// nullptr too (the order rule).  No cap on n_items.
hipError_t launch_write_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                               const void* d_new, const uint32_t* d_items,
                               const uint8_t* d_bitmap, uint64_t* d_digests, const Geometry& g,
                               const LaunchShape& ls, uint64_t offset, uint64_t len,
                               uint64_t n_items, hipStream_t s);
hipError_t launch_write_items_check(const uint8_t* d_bitmap, const uint32_t* d_items, uint64_t n,
                                    const Geometry& g, int32_t* d_status, hipStream_t s);
// launch_readv with kReadDevTiles over a shard table: d_iov, d_bitmap, d_work,
// n, tiles and g.gate as there (launch_readv_check and launch_readv_scan touch
// no block and serve both layouts).
hipError_t launch_readv_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                               void* d_out, const Geometry& g, const LaunchShape& ls, uint64_t n,
                               uint64_t tiles, const uint32_t* d_iov, const uint8_t* d_bitmap,
                               const uint32_t* d_work, hipStream_t s);
// Device-side recoverability check (xorec_utils.hpp:160-175 over the batch):
// *d_status |= 4 if some class of some stripe lost two or more blocks.  The
// caller zeroes *d_status first (stream-ordered).
hipError_t launch_check(const uint8_t* d_bitmap, const Geometry& g, int32_t* d_status,
                        hipStream_t s);
// The same check, and the list of lost data blocks for kDecodeDevListTiles
// into d_list (header zeroed here with *d_status first; at most S*m entries).
hipError_t launch_scan_list(const uint8_t* d_bitmap, const Geometry& g, int32_t* d_status,
                            uint32_t* d_list, hipStream_t s);
hipError_t launch_erase(void* d_data, void* d_parity, const uint8_t* d_bitmap, const Geometry& g,
                        hipStream_t s);
hipError_t launch_fill(void* d_buf, uint64_t S, uint64_t words, uint64_t seed_base,
                       hipStream_t s);
// Gather (xec_pipeline's small-block decode): block i of stripe c of a chunk
// (item c << 8 | i, at most kArgItems items, k <= 256) is copied from
// d_data + (c*k + i)*bs to d_out + g*bs for the g-th item, so the chunk's
// rebuilt blocks leave in one D2H copy.  bs % 16 == 0.
hipError_t launch_gather(const void* d_data, void* d_out, uint64_t k, uint64_t bs,
                         const uint32_t* h_items, uint64_t n, hipStream_t s);
// xec_set_validate_kernel: 0 auto, 1 lane per block, 2 wave per block.
extern thread_local int g_validate_mode;
hipError_t launch_pattern(void* d_data, uint64_t nblocks, uint64_t bs, uint64_t seed,
                          hipStream_t s);
hipError_t launch_validate(const void* d_data, uint64_t nblocks, uint64_t bs, uint32_t* d_bad,
                           hipStream_t s);
// Load each kernel file's code object onto the current device.  HIP loads a
// code object at the first launch of one of its kernels, ~10 ms on MI355X
// (tools/latency/first_call.py, profiles/r03z); xec_init does it instead, so
// the first codec call runs at the steady-state latency.
hipError_t preload_kernels();
hipError_t preload_validate();

}  // namespace xec
