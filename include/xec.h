/*
 * xec.h -- C ABI of the MI355X-native XOR-EC hot path (libxec_hip.so).
 *
 * This is the drop-in boundary.  It replaces the reference's GPU codec
 * functions (kenji-k6/erasure-code-benchmark, src/xorec/xorec_gpu_cmp.cuh:14-70)
 * with plain-C entry points that the reference's codec plugin layer
 * (src/algorithms/, class AbstractBenchmark, abstract_bm.hpp:18-88) can call
 * from a new XorecBenchmarkHip plugin; see INTEGRATION.md.
 *
 * Batch layout (identical to the reference, abstract_bm.cpp:4-18,
 * xorec_gpu_cmp.cu:135-144):
 *   data   : stripe c, data block i   at byte c*k*bs + i*bs
 *   parity : stripe c, parity block j at byte c*m*bs + j*bs
 *   bitmap : one byte per block, stripe c at c*(k+m): k data bytes then
 *            m parity bytes; 0 = lost, nonzero = present.
 * Parity class of data block i is i % m: parity[j] = XOR of data[i], i%m==j.
 *
 * Conventions (reference xorec_gpu_cmp.cu / xorec_gpu_cmp_bm.cpp):
 *   - the caller owns every buffer, the device bitmap scratch included; the
 *     codec allocates nothing per call;
 *   - compute calls are asynchronous on `stream` (NULL = the null stream); the
 *     caller synchronises (xorec_gpu_cmp_bm.cpp:50,67);
 *   - status codes 0..4 equal the reference XorecResult
 *     (xorec_utils.hpp:26-32); 5 and 6 are new; no exception crosses the ABI.
 *   - use before xec_init returns XEC_NOT_INITIALIZED (the reference throws,
 *     xorec_gpu_cmp.cu:39,67).
 */
#ifndef XEC_H
#define XEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;

typedef enum {
  XEC_SUCCESS = 0,           /* XorecResult::Success */
  XEC_INVALID_SIZE = 1,      /* XorecResult::InvalidSize   (bs < 256 or bs % 256) */
  XEC_INVALID_ALIGNMENT = 2, /* XorecResult::InvalidAlignment (data/parity not 64-B aligned) */
  XEC_INVALID_COUNTS = 3,    /* XorecResult::InvalidCounts (k < 1, m < 1, k % m) */
  XEC_DECODE_FAILURE = 4,    /* XorecResult::DecodeFailure (a class lost > 1 block) */
  XEC_NOT_INITIALIZED = 5,   /* new: xec_init not called / failed */
  XEC_DEVICE_ERROR = 6       /* new: a HIP runtime call or launch failed */
} xec_status;

/* Replaces xorec_gpu_init (xorec_gpu_cmp.cuh:14, .cu:7-27) and xorec_init
 * (xorec.hpp:39, xorec.cpp:16-22).  Selects `device_id` for the calling
 * thread, loads the library's kernels onto it (~10 ms once per device and
 * process, so the first codec call runs at steady-state latency) and marks
 * the library initialised.  Idempotent per device.  Unlike
 * the reference it takes no k: recovery checks are sized per call, so the
 * COMPLETE_DATA_BITMAP first-call sizing bug (xorec.cpp:16-22) cannot occur. */
xec_status xec_init(int device_id);

/* Replaces xorec_gpu_encode (xorec_gpu_cmp.cuh:28-37, .cu:29-55).
 * parity[c][j] = XOR_{i % m == j} data[c][i] for every stripe c < S.
 * Arguments are checked exactly like xorec_check_args (xorec_utils.hpp:61-86).
 * One kernel, no memset, no atomics; parity is fully overwritten.
 * The reference's num_gpu_blocks/threads_per_block launch arguments are gone:
 * the launch shape is chosen for gfx950 (see xec_set_launch). */
xec_status xec_encode(const void* d_data, void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, hipStream_t stream);

/* Replaces xorec_gpu_decode (xorec_gpu_cmp.cuh:57-68, .cu:57-115).
 * h_bitmap: S*(k+m) bytes of host memory (pinned for an asynchronous copy);
 * d_bitmap: S*(k+m) bytes of device scratch owned by the caller.
 * Host checks follow the reference: XEC_DECODE_FAILURE if ANY stripe is
 * unrecoverable (is_recoverable, xorec_utils.hpp:160-175) and then no data is
 * touched; XEC_SUCCESS without a kernel if no stripe needs recovery
 * (require_recovery, xorec_utils.hpp:144-149).  Otherwise every lost data
 * block is rebuilt:
 *   data[c][i] = parity[c][i%m] ^ XOR_{l%m == i%m, l != i} data[c][l].
 * What the kernel reads besides the batch -- a copy of h_bitmap, or the list
 * of lost data blocks the host scan found (4 bytes each; the list drives one
 * tile per lost block and 1 KiB chunk, xec_set_decode_tiling) -- is copied to
 * device buffers the library keeps, on a copy stream of its own that does not
 * wait for `stream`'s earlier work, when `stream` is busy at the call; `stream`
 * waits only for that copy before the decode kernel.  When `stream` is idle
 * (a synchronous caller) the copy goes into d_bitmap on `stream` itself, which
 * then starts at once without a cross-stream hand-off.  Up to 1,024 list
 * entries travel in the kernel arguments instead, and then nothing is copied;
 * so do batches of at most 1,024 stripes with k <= 32 that would otherwise
 * copy something (one loss mask per stripe).
 * d_bitmap is scratch for the call.  Not
 * capturable: the host scan reads h_bitmap at call time, so a graph would
 * replay this call's losses -- on a stream being captured a call with blocks
 * to rebuild returns XEC_DEVICE_ERROR with nothing queued (xec_decode_device
 * is the capturable form).  A batch that needs no recovery, or cannot be
 * recovered, returns XEC_SUCCESS / XEC_DECODE_FAILURE from the host scan
 * before any device call, capturing or not, as the reference decides before
 * its first CUDA call (xorec_gpu_cmp.cu:75-81).
 * Lost parity is not regenerated (xec_repair does that).  Parity is READ-ONLY here, as in the CPU
 * decode (xorec.cpp:62-111) -- deliberately unlike the reference GPU decode,
 * which folds all data into parity (xorec_gpu_cmp.cu:94-102).  The content of
 * lost data blocks on entry is irrelevant (no zeroing pre-condition).
 * The list is staged in pinned host memory the library keeps for reuse; the
 * pinned staging, the device buffers and one copy stream per device are the
 * only memory it holds across calls.  Bitmaps of 256 KiB and more are copied
 * before the host scan so the two overlap (into d_bitmap on the fallback path,
 * whatever the verdict).  h_bitmap must stay unchanged until the stream has
 * passed the call, as for any asynchronous copy. */
xec_status xec_decode(void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, const uint8_t* h_bitmap, uint8_t* d_bitmap, hipStream_t stream);

/* Per-stripe form of xec_decode: the semantics of the reference CPU plugin
 * (XorecBenchmark::decode, xorec_bm.cpp:43-58, xorec_decode per stripe,
 * xorec.cpp:62-111) rather than of its GPU path.  Every stripe that needs
 * recovery and is recoverable is rebuilt; an unrecoverable stripe is left
 * untouched and makes the call return XEC_DECODE_FAILURE after the others
 * are queued.  h_codes (S bytes of host memory, may be NULL) receives each
 * stripe's XorecResult (0, or 4 for that stripe), written before the call
 * returns.  Always work-list tiles (one per rebuilt block and 1 KiB chunk);
 * requires k <= 256 and S <= 2^24 (else XEC_INVALID_SIZE).  Other arguments,
 * checks and the scratch as xec_decode. */
xec_status xec_decode_per_stripe(void* d_data, const void* d_parity, size_t S, size_t bs,
                                 size_t k, size_t m, const uint8_t* h_bitmap, uint8_t* d_bitmap,
                                 uint8_t* h_codes, hipStream_t stream);

/* Device-resident form of xec_decode (no reference counterpart: the reference
 * always scans a host bitmap, xorec_gpu_cmp.cu:75-83).  For callers whose
 * erasure bitmap already lives in device memory: no host scan, no copy, no
 * host synchronisation, so the call can be captured in a hipGraph.
 * Enqueues on `stream`: *d_status = 0; a check kernel that sets *d_status = 4
 * (XEC_DECODE_FAILURE) if any stripe is unrecoverable (is_recoverable,
 * xorec_utils.hpp:160-175); then the decode kernel, which does nothing if
 * *d_status != 0 (all-or-nothing, like xec_decode) and otherwise rebuilds
 * every lost data block exactly as xec_decode does.  The return value covers
 * only what the host can check (argument errors as xec_decode, d_status
 * null or not 4-B aligned -> XEC_INVALID_ALIGNMENT, d_bitmap null with S > 0
 * -> XEC_INVALID_SIZE, launch failure); nothing is queued on `stream` when an
 * argument is rejected.  The batch verdict is *d_status (device int32), valid
 * once the stream reaches it.  Tiling: stripe tiles with the single-erasure
 * residency table (no host view of the loss count), unless
 * xec_set_decode_tiling(2). */
xec_status xec_decode_device(void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                             size_t m, const uint8_t* d_bitmap, int32_t* d_status,
                             hipStream_t stream);

/* Device-resident decode for batches where only some stripes lost blocks (no
 * reference counterpart; the device analogue of xec_decode's work-list tiles).
 * xec_decode_device launches a tile for every (stripe, 1 KiB chunk) of the
 * batch, so a batch where few stripes lost anything spends most of its
 * workgroups finding nothing to do.  Here the check kernel also lists the
 * lost data blocks into d_work (4-byte aligned device scratch of at least
 * xec_decode_device_list_bytes(S, k, m) bytes, owned by the caller), and the
 * decode is one tile per (listed block, chunk), walked by a grid fixed at
 * launch since the host never sees the count: one workgroup per 8 possible
 * tiles, between what the chip holds at once and 131,072 (xec_set_launch's
 * max_grid overrides it).  Sparse losses (1 stripe in 9): 1.7-3.9x faster
 * than xec_decode_device; losses in every stripe: 6-13 % slower, so there
 * xec_decode_device is the better call.  Everything else as xec_decode_device: no
 * host work (hipGraph-capturable), *d_status = 0 or 4 in stream order,
 * all-or-nothing, parity read-only, identical bytes.  Requires k <= 256 and
 * S <= 2^24 (else XEC_INVALID_SIZE), as does a too small work_bytes or a null
 * d_bitmap with S > 0; d_status or d_work null or not 4-B aligned ->
 * XEC_INVALID_ALIGNMENT; nothing is queued when an argument is rejected. */
xec_status xec_decode_device_list(void* d_data, const void* d_parity, size_t S, size_t bs,
                                  size_t k, size_t m, const uint8_t* d_bitmap, void* d_work,
                                  size_t work_bytes, int32_t* d_status, hipStream_t stream);

/* Scratch bytes xec_decode_device_list needs: 4 * (1 + S*m), a 4-byte count
 * and at most one 4-byte entry per parity class. */
size_t xec_decode_device_list_bytes(size_t S, size_t k, size_t m);

/* Full-stripe repair (no reference counterpart: neither reference decode puts
 * lost parity back).  The recoverability rule is symmetric -- a class has at
 * most one lost block among its k/m data blocks and its parity block -- so
 * EVERY lost block, data or parity, is rebuilt as the XOR of the other k/m
 * blocks of its class: a lost data block exactly as xec_decode rebuilds it, a
 * lost parity block as xec_encode computes it.  Unlike xec_decode, d_parity is
 * written (its lost blocks only).
 * A block is lost iff its bitmap byte is 0 (2, 3, 255 are present): there is
 * work iff some byte is 0 -- the bit-0 rule of require_recovery plays no part.
 * All-or-nothing like xec_decode: if any class of any stripe lost two blocks
 * the call returns XEC_DECODE_FAILURE and neither buffer is written.  What a
 * lost block holds on entry is irrelevant; blocks that are present are never
 * written.  h_bitmap, d_bitmap (scratch), argument checks and status codes as
 * xec_decode.  The host scan lists the lost blocks as work items c << 8 | i,
 * i in [0, k+m), i >= k naming parity block i - k, which requires k + m <= 256
 * and S <= 2^24 (else XEC_INVALID_SIZE), and the launch is always work-list
 * tiles: one per (listed block, 1 KiB chunk).  Up to 1,024 entries travel in
 * the kernel arguments (capacities 64 / 256 / 1024) and nothing is copied; a
 * longer list is staged in the pinned memory the library keeps and uploaded
 * on `stream` itself into d_bitmap, in pieces of what the scratch holds (no
 * copy stream of the library's is involved; a null d_bitmap is then
 * XEC_INVALID_SIZE).  Nothing lost: XEC_SUCCESS without any device call; an
 * unrecoverable batch: XEC_DECODE_FAILURE without any device call.  Not
 * capturable, as xec_decode: on a capturing stream a call with blocks to
 * rebuild returns XEC_DEVICE_ERROR with nothing queued. */
xec_status xec_repair(void* d_data, void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                      const uint8_t* h_bitmap, uint8_t* d_bitmap, hipStream_t stream);

/* Device-resident form of xec_repair: no host work, so it can be captured in
 * a hipGraph, and no limit on k + m or S.  Enqueues on `stream`: *d_status =
 * 0; the check kernel of xec_decode_device (*d_status = 4 if any class of any
 * stripe lost two blocks); then a repair kernel over class tiles (stripe,
 * class, 1 KiB chunk) that does nothing if *d_status != 0 and otherwise reads
 * its class's bitmap bytes and does the one reduction the class needs, or
 * none.  Arguments, checks and the meaning of the return value and of
 * *d_status as xec_decode_device; nothing is queued when an argument is
 * rejected.  Bytes identical to xec_repair's. */
xec_status xec_repair_device(void* d_data, void* d_parity, size_t S, size_t bs, size_t k,
                             size_t m, const uint8_t* d_bitmap, int32_t* d_status,
                             hipStream_t stream);

/* Diagnostics: which tiling the calling thread's most recent xec_repair or
 * xec_repair_device launched -- 0 none (an error, or nothing to rebuild),
 * XEC_TILING_CLASS (xec_repair_device), XEC_TILING_LIST or XEC_TILING_ARG_LIST
 * (xec_repair; enum below).  xec_decode_tiling_used is not affected. */
int xec_repair_tiling_used(void);

/* Device parity scrub (no reference counterpart): do data and parity still
 * agree?  d_flags: S*m bytes of device memory owned by the caller, index
 * c*m + j; d_count: one device uint32 (4-B aligned, else
 * XEC_INVALID_ALIGNMENT), or NULL.  Enqueues on `stream` (no host work:
 * capturable): d_flags zeroed by a stream-ordered memset; one kernel over
 * class tiles that XORs the class's k/m data blocks and its parity block and
 * sets d_flags[c*m + j] = 1 where any byte of the result is nonzero; then,
 * when d_count is not NULL, a small kernel that sums the flags into *d_count
 * (each class counted once).  Reads the whole batch once, (k+m)*bs*S bytes,
 * and writes nothing but d_flags and *d_count -- no second parity buffer.
 * A NULL d_flags with S > 0 is XEC_INVALID_SIZE; other checks as xec_encode;
 * nothing is queued when an argument is rejected.
 * Captured in a hipGraph the two memsets become memset nodes.  Open
 * observation (cause not found; tools/lab/graph_verify_probe.py, DESIGN.md §3
 * *Update*): where the process allocated device memory, uploaded from pageable
 * host memory or captured another graph around the capture, replays have left
 * d_flags and *d_count with bytes no kernel stores, on a batch that was right.
 * With every input on the device before the capture and only device-to-device
 * copies between replays the captured scrub has been exact.
 * What it cannot tell: WHICH block of a flagged class is at fault (a class's
 * blocks enter the XOR alike), and two errors of one class that cancel -- the
 * same bits flipped at the same offset of two of its blocks -- are invisible.
 * xec_locate with stored block digests (below) answers both. */
xec_status xec_verify(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, uint8_t* d_flags, uint32_t* d_count, hipStream_t stream);

/* ---- shard-major layout (no reference counterpart in its GPU codec; its
 * Leopard, ISA-L and cm256 plugins take blocks as pointer tables for the same
 * reason, src/algorithms/leopard_bm.cpp:24-47) -------------------------------
 * A parity store keeps one buffer per shard -- per disk, failure domain or
 * peer -- not the k + m blocks of a stripe side by side.  The calls below take
 * that memory as it is: h_shards is a HOST array of k + m device pointers, the
 * k data shards then the m parity shards, in the order of the bitmap's bytes,
 * and
 *   data block i   of stripe c : h_shards[i]     + c * data_stride     (i < k)
 *   parity block j of stripe c : h_shards[k + j] + c * parity_stride   (j < m)
 * The batch layout above is the special case h_shards[i] = d_data + i*bs,
 * data_stride = k*bs, h_shards[k+j] = d_parity + j*bs, parity_stride = m*bs
 * (hence two strides), and gives the bytes of the batch calls.  The table
 * travels by value in the kernel arguments (64 or 256 pointers, 512 B or
 * 2 KiB, the smaller that holds it): nothing is copied, no scratch is needed,
 * and h_shards is read before the call returns -- there is no other host
 * work, so every call is capturable, and a replay uses the pointers of the
 * capture.  Shard forms exist for encode, the device-bitmap repair, the
 * scrub, digest, locate, the device-resident degraded read and vectored read,
 * and the degraded write (xec_write_shards_device, which with a NULL bitmap is
 * the ranged update and with the whole block as its range the update): the
 * device-resident surface is complete.  Out of scope and batch-only: the
 * host-list forms (xec_read, xec_readv, xec_write, xec_update, xec_update_range,
 * xec_repair, xec_decode), a mask / shadow form of the write or the update, a
 * range per written item (a writev), and residency sweeps on this layout.
 * Every table entry must be
 * a valid shard in every call, a dead shard with no memory behind it included:
 * a lost block is never read, but its address must still pass xec_check_shards.
 * When to use which (tools/shards_bench.py on one MI355X, configs 2, 3 and 4 --
 * 8+1 x 64 KiB x 1,024, 16+1 x 1 MiB x 256, 32+1 x 4 KiB x 65,536; kernel
 * times, round-to-round spreads 0.04-1.5 % and one of 2.9 %; DESIGN.md §3
 * *Shard layout*): a caller whose bytes are already in the batch layout keeps
 * the batch calls -- through a table aliased into the same batch the shard
 * kernels took 0.99-1.01 of their time, except the scrub at config 2 and the
 * repair of one data block per stripe at config 4, 1.08 both.  A caller with
 * one buffer per shard uses these calls on that memory rather than copying into
 * a batch and back: k + m separate allocations at stride bs took 1.00-1.13 of
 * the batch calls' time, where the copy alone moves the same bytes twice more.
 * Padding the stride by 4 KiB is not advice that holds: against stride bs it
 * was 4-6 % faster at config 2, 15-17 % slower at config 3 and 6-9 % slower at
 * config 4 (3 % faster for the data-block repair there).  Column rotation
 * (xec_set_rotation(3)) on separate allocations made the scrub at config 3 4 %
 * faster and everything else 0-4 % slower: leave it off.
 * Digest, locate and read, same tool and configs (spreads 0.06-3.1 %, the batch
 * locate at config 2 8 % and the batch digest at config 4 4.6 %): the digest
 * and the locate over the flags of one class in 64 took 0.99-1.00 of the batch
 * kernels' time aliased and 0.95-1.06 on separate allocations, padded or not.
 * The read of one whole lost block per stripe took 1.01 / 0.97 / 1.09 aliased
 * at configs 2 / 3 / 4 and 1.00 / 1.07 / 1.12 on separate allocations; 4 KiB
 * from each of min(S, 1024) lost blocks 1.06 / 1.00 / 1.11 aliased (9.0, 5.8 and
 * 26 us) and 1.04 / 1.11 / 1.12 separate.  The 1.09-1.12 at config 4 is the
 * repair's 1.08 again: a tile there is 1 KiB of each of 32 members, and each
 * member's address is a scalar load from the kernel arguments with a wait of
 * its own where the batch kernel adds a stride.  A stride padded by 4 KiB,
 * against stride bs, made the 4 KiB reads 18 % faster at config 2 and both
 * reads 6-8 % slower at config 4.
 *
 * xec_check_shards: the host-only check the three compute calls run (no GPU
 * and no xec_init needed).  In this order:
 *  1. bs, then k and m, exactly as xec_check_args with both pointers NULL ->
 *     XEC_INVALID_SIZE, XEC_INVALID_COUNTS;
 *  2. S == 0 -> XEC_SUCCESS (h_shards is not looked at);
 *  3. k + m > 256 -> XEC_INVALID_SIZE;
 *  4. h_shards NULL, or an entry NULL -> XEC_INVALID_SIZE;
 *  5. an entry not 64-byte aligned, or a stride not a multiple of 64 ->
 *     XEC_INVALID_ALIGNMENT;
 *  6. a stride < bs, or (S-1)*stride + bs not representable in 64 bits (or a
 *     shard whose bytes would wrap the address space) -> XEC_INVALID_SIZE;
 *  7. overlap -> XEC_INVALID_SIZE.  The hull of shard x is
 *     [p_x, p_x + (S-1)*s_x + bs).  Every pair of shards must either have
 *     disjoint hulls, or have the same stride s and, with
 *     d = (p_y - p_x) mod s, both d >= bs and s - d >= bs: interleaved shards,
 *     the batch layout among them.  A pair with different strides (a data
 *     shard against a parity shard) must have disjoint hulls.
 * The rule is conservative by design: it refuses some tables whose blocks do
 * not in fact overlap (hulls that intersect at different strides, or at equal
 * strides for a stripe count too small for the blocks to meet), and it holds
 * encode's read-only data shards to the same rule, so that one rule covers
 * all three calls.  The pair check is quadratic in k + m; tools/shards_bench.py
 * reports what it costs per call at k + m = 17 and 256. */
xec_status xec_check_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                            size_t S, size_t bs, size_t k, size_t m);

/* xec_encode over shards: parity block j of stripe c = XOR of the data blocks
 * i % m == j of stripe c, for every c < S.  Checks, in this order:
 * XEC_NOT_INITIALIZED; xec_check_shards; S == 0 is XEC_SUCCESS with nothing
 * queued.  Reads the k data shards' blocks, fully overwrites the m parity
 * shards' blocks; bytes of a shard between its blocks (stride > bs) are never
 * touched.  One kernel over class tiles, encode's: same launch shape
 * (xec_set_launch, all four arguments), same column rotation (xec_set_rotation
 * -- a permutation of a block's chunks, independent of the layout), parity
 * stored nt, residency by xec_encode's table -- which was swept on the batch
 * layout and has not been swept on this one. */
xec_status xec_encode_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, hipStream_t stream);

/* xec_repair_device over shards (it covers decode, and puts lost parity back):
 * d_bitmap, d_status, the verdict and the all-or-nothing behaviour are
 * xec_repair_device's -- *d_status = 0, the same check kernel (*d_status = 4 if
 * a class of a stripe lost two blocks), then a repair kernel over class tiles
 * that does nothing if *d_status != 0 and otherwise rebuilds every lost block,
 * data or parity, from the other k/m blocks of its class.  Checks, in this
 * order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_status NULL or not 4-byte aligned -> XEC_INVALID_ALIGNMENT; d_bitmap
 *     NULL with S > 0 -> XEC_INVALID_SIZE;
 *  4. S == 0 -> XEC_SUCCESS with only *d_status = 0 queued;
 *  5. steps 3 to 7 of xec_check_shards.
 * A rejected call queues nothing.  Blocks that are present, the bytes between
 * blocks and the bitmap are never written; what a lost block holds on entry is
 * irrelevant.  Launch shape, rotation and residency as xec_encode_shards; a
 * rebuilt data block is stored sc1, a rebuilt parity block nt. */
xec_status xec_repair_shards_device(const void* const* h_shards, size_t data_stride,
                                    size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                    const uint8_t* d_bitmap, int32_t* d_status, hipStream_t stream);

/* xec_verify over shards: d_flags (S*m device bytes, index c*m + j), d_count
 * (device uint32 or NULL), what is flagged and what cannot be seen are
 * xec_verify's.  Checks, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_count not 4-byte aligned -> XEC_INVALID_ALIGNMENT; d_flags NULL with
 *     S > 0 -> XEC_INVALID_SIZE;
 *  4. S == 0 -> XEC_SUCCESS with only *d_count = 0 queued (when given);
 *  5. steps 3 to 7 of xec_check_shards.
 * A rejected call queues nothing.  Reads every block of every shard once and
 * writes nothing but d_flags and *d_count.  Residency by xec_verify's table,
 * swept on the batch layout only.
 * Captured in a hipGraph the two memsets become memset nodes.  Open
 * observation (cause not found; tools/lab/graph_verify_probe.py, DESIGN.md §3
 * *Update*): where the process allocated device memory, uploaded from pageable
 * host memory or captured another graph around the capture, replays have left
 * d_flags and *d_count with bytes no kernel stores, on a batch that was right.
 * Run the scrub on a plain stream. */
xec_status xec_verify_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, uint8_t* d_flags,
                             uint32_t* d_count, hipStream_t stream);

/* xec_digest over shards: d_digests (S*(k+m) device u64, the bitmap's layout),
 * d_select (NULL = every block, else S*(k+m) device bytes, nonzero = digest
 * this block; an unselected block is not read and its slot neither read nor
 * written), the digest itself -- bit-exact against xec_digest_host -- and what
 * zeroes the selected slots (a memset with d_select NULL, else a small kernel)
 * are xec_digest's.  Checks, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_digests NULL with S > 0 -> XEC_INVALID_SIZE; d_digests not 8-byte
 *     aligned -> XEC_INVALID_ALIGNMENT;
 *  4. S == 0 -> XEC_SUCCESS with nothing queued;
 *  5. steps 3 to 7 of xec_check_shards.
 * A rejected call queues nothing.  Reads each selected block once -- bytes of a
 * shard between its blocks (stride > bs) are never read -- and writes nothing
 * but d_digests; through a table aliased into a batch it leaves exactly
 * xec_digest's slots.  One kernel over (block, 64 KiB segment) tiles,
 * xec_digest's: same grid limit, xec_set_launch as there (max_grid,
 * cache_policy, block_threads), no column rotation, residency uncapped -- swept
 * on the batch layout only. */
xec_status xec_digest_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, const uint8_t* d_select,
                             uint64_t* d_digests, hipStream_t stream);

/* xec_locate over shards: d_digests (the stored digests), d_flags (NULL = check
 * every block, else xec_verify_shards' S*m flags: the gate -- a block of an
 * unflagged class is not read and reads 1), d_bitmap (S*(k+m) device bytes, 0 =
 * the digest differs), d_count and d_work (xec_locate_work_bytes(S, k, m)
 * bytes: the size serves both layouts) are xec_locate's, and so is what is
 * queued: *d_count zeroed by a memset, the checked slots of d_work zeroed (a
 * memset with d_flags NULL, else a small kernel), the digest kernel of
 * xec_digest_shards, the compare-and-count kernel of xec_locate.  Checks, in
 * this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_digests or d_work NULL with S > 0, or work_bytes too small ->
 *     XEC_INVALID_SIZE; d_digests or d_work not 8-byte aligned, or d_count not
 *     4-byte aligned -> XEC_INVALID_ALIGNMENT; d_bitmap NULL with S > 0 ->
 *     XEC_INVALID_SIZE;
 *  4. S == 0 -> XEC_SUCCESS with only *d_count = 0 queued (when given);
 *  5. steps 3 to 7 of xec_check_shards.
 * A rejected call queues nothing.  No shard is written and no byte between
 * blocks is read; aliased into a batch it leaves exactly xec_locate's bitmap
 * and count.  xec_verify_shards -> xec_locate_shards(flags) ->
 * xec_repair_shards_device runs on one stream with no host step and no copy;
 * the three outcomes for a flagged class are those listed at xec_locate.  A
 * capture contains memset nodes: the open observation recorded at xec_verify
 * applies, run the chain on a plain stream. */
xec_status xec_locate_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, const uint64_t* d_digests,
                             const uint8_t* d_flags, uint8_t* d_bitmap, uint32_t* d_count,
                             void* d_work, size_t work_bytes, hipStream_t stream);

/* xec_read_device over shards: serve reads from a store with a shard down.
 * d_bitmap (NULL = everything present, a pure gather), d_items (c << 8 | i, any
 * order, repeats allowed), the range rules, d_out (item t's bytes at d_out +
 * t*len), the verdicts 0 / 3 / 4 left as a maximum in *d_status, and the
 * all-or-nothing behaviour over the requested items are xec_read_device's, and
 * so is what is queued: *d_status = 0 (a memset), the same check kernel over
 * the items, then a read kernel that does nothing if *d_status != 0.  A lost
 * block is never read, and nothing but d_out and *d_status is written: a
 * reader needs no write access to the store.  Checks, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_status NULL or not 4-byte aligned -> XEC_INVALID_ALIGNMENT; n_items == 0
 *     or S == 0 -> XEC_SUCCESS with only *d_status = 0 queued; steps 4 to 7 of
 *     xec_read with d_items in h_items' place; d_items not 4-byte aligned ->
 *     XEC_INVALID_ALIGNMENT;
 *  4. steps 3 to 7 of xec_check_shards;
 *  5. d_out's n_items*len bytes intersect the hull [p_x, p_x + (S-1)*s_x + bs)
 *     of any shard -> XEC_INVALID_SIZE.  The conservative hull rule of
 *     xec_check_shards: a d_out placed in a gap between two blocks of one shard
 *     is refused; ranges that only touch are allowed.
 * A rejected call queues nothing.  Bytes of a shard between its blocks are
 * never read; aliased into a batch it delivers exactly xec_read_device's bytes.
 * Capturable (one memset node, for *d_status).  One kernel over (item, chunk of
 * the range) tiles, xec_read_device's: xec_set_launch as there, no column
 * rotation, residency by xec_read_device's table, swept on the batch layout
 * only. */
xec_status xec_read_shards_device(const void* const* h_shards, size_t data_stride,
                                  size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                  const uint8_t* d_bitmap, const uint32_t* d_items,
                                  size_t n_items, size_t offset, size_t len, void* d_out,
                                  int32_t* d_status, hipStream_t stream);

/* xec_write over shards, device-resident: a store with a shard down takes a
 * small write in place.  The semantics are xec_write's, word for word, over the
 * table: items c << 8 | i with i < k, strictly ascending; one range
 * [offset, offset + len) per call, multiples of 16; item t's new bytes at
 * d_new + t*len; every (stripe, class) with an item runs in the delta, data-only
 * or rebuild-write mode; servability is xec_read's rule, all-or-nothing over the
 * items; the digest upkeep in all three modes (d_digests may be NULL) is exactly
 * what xec_write describes; a lost block is never read and never written, and
 * bytes of a shard between its blocks are never touched.  d_bitmap == NULL
 * means everything is present: the call is then xec_update_range over shards,
 * and with offset = 0, len = bs xec_update -- one call covers update, ranged
 * update and degraded write, there are no separate update entry points.  It
 * takes what xec_read_shards_device takes on the read side, a device list and
 * the bytes packed in list order, not xec_write_device's mask over a shadow of
 * the whole data range: a shard store has no second copy of every shard.
 * Through a table aliased into a batch it leaves exactly xec_write's bytes and
 * digest slots, and is the capturable list form of the batch write.
 * Checks, all on the host before anything is queued, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. d_status NULL or not 4-byte aligned -> XEC_INVALID_ALIGNMENT;
 *  4. n_items == 0 or S == 0 -> XEC_SUCCESS with only *d_status = 0 queued;
 *  5. k + m > 256 or S > 2^24 -> XEC_INVALID_SIZE;
 *  6. the range, step 5 of xec_update_range;
 *  7. d_new or d_items NULL -> XEC_INVALID_SIZE;
 *  8. d_new not 16-byte aligned, d_items not 4-byte aligned, or d_digests not
 *     NULL and not 8-byte aligned -> XEC_INVALID_ALIGNMENT;
 *  9. n_items * len not representable -> XEC_INVALID_SIZE (the tile count is at
 *     most n_items * len / 16, so it fits whenever that does);
 * 10. steps 3 to 7 of xec_check_shards;
 * 11. d_new's n_items*len bytes or d_digests' 8*S*(k+m) bytes meet the hull of
 *     any shard (the rule of xec_read_shards_device step 5), or each other ->
 *     XEC_INVALID_SIZE; ranges that only touch are allowed.
 * A rejected call queues nothing.  Enqueues on `stream`, with no host work
 * beyond reading h_shards, so the call is capturable (one memset node) and a
 * replay applies whatever d_items, d_bitmap and d_new hold then: *d_status = 0
 * (a memset, as xec_read_shards_device); a check kernel, one thread per item,
 * that leaves *d_status at the MAXIMUM over the items of 0 (acceptable), 3
 * (c >= S, i >= k, or t > 0 and items[t-1] >= items[t], compared on the raw
 * words: disorder and repeats) and 4 (the block is lost and another block of
 * its class is lost too) -- an item with c >= S or i >= k never indexes the
 * bitmap, and the kernel runs with d_bitmap NULL as well, for the order rule;
 * then the write kernel over (list position, chunk of the range) tiles, which
 * does nothing if *d_status != 0.  NOTE the difference from the host form: in
 * xec_write a broken item rule (XEC_INVALID_COUNTS, 3) outranks an unservable
 * item (4) wherever they stand; here the verdict is the maximum, so a list with
 * both reports 4, as xec_read_device's does.  The first item of a (stripe,
 * class) owns that class's parity granules and reads its mode from the bitmap:
 * the item's own byte and the byte of its class's parity block.  New data is
 * stored sc1, parity nt.  There is no limit on n_items.  Of xec_set_launch all
 * four arguments apply, xec_set_rotation does not; residency is uncapped, as
 * for xec_write, swept on the batch layout only.  xec_write_tiling_used is not
 * affected, as xec_read_tiling_used is not by xec_read_shards_device.
 * Measured against xec_write on the same items (tools/shards_bench.py, one
 * MI355X, configs 2 / 3 / 4, kernel times, profiles/shards/write_readv_bench.json,
 * DESIGN.md §3 *Shard layout*; the check kernel is not in these times): 4 KiB into
 * each of min(S, 1,024) LOST blocks (rebuild-write) took 1.09 / 1.22 / 1.08 of
 * xec_write's kernel aliased into the batch (9.6, 8.0 and 26 us there) and 1.14 /
 * 1.26 / 1.19 on separate allocations; the same with the blocks present (delta)
 * 1.17 / 1.03 / 1.16 and 1.09 / 1.02 / 1.16 on kernels of 4-5 us whose rounds
 * spread up to 9 %; one whole lost block per stripe 1.03 / 1.00 / 1.00 and 1.03 /
 * 1.10 / 1.03; one whole present block per stripe 1.06 / 1.02 / 1.03 and 1.06 /
 * 1.10 / 0.99 (spreads 0.1-3 %). */
xec_status xec_write_shards_device(const void* const* h_shards, size_t data_stride,
                                   size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                   const uint8_t* d_bitmap, const uint32_t* d_items, size_t n_items,
                                   size_t offset, size_t len, const void* d_new,
                                   uint64_t* d_digests, int32_t* d_status, hipStream_t stream);

/* xec_readv_shards_device, the vectored read over shards, stands with
 * xec_readv_device below: it takes that call's xec_iov entries. */

/* Diagnostics: how many pointers the kernel-argument table of the calling
 * thread's most recent shard call (xec_encode_shards, xec_repair_shards_device,
 * xec_verify_shards, xec_digest_shards, xec_locate_shards,
 * xec_read_shards_device, xec_write_shards_device or
 * xec_readv_shards_device) could hold -- 64 or 256, the smaller capacity that holds
 * k + m; 0 when that call launched nothing (an error, S == 0, or no items). */
int xec_shards_arg_capacity_used(void);

/* In-place block update, the small write of a parity store (no reference
 * counterpart: its codec encodes and decodes whole stripes).  Data block i of
 * stripe c is replaced by a new block and the parity of its class follows by
 * the delta,
 *     parity[c][i % m] ^= data[c][i] ^ new;    data[c][i] = new
 * -- three block reads and two block writes per changed block, against the
 * k + m blocks per stripe of the xec_encode that would otherwise put parity
 * right (5/17 of its bytes for one block of a 16+1 stripe, and nothing for a
 * stripe nobody wrote).  Blocks that are not named are neither read nor
 * written, except the parity block of a class with an item, which is read and
 * written.  One workgroup owns a parity granule for the whole call and folds
 * every item of its class, so several items of one class in one call are fine.
 * The delta keeps a class's syndrome: a class whose data and parity disagreed
 * before the call disagrees after it, and xec_verify still flags it, where a
 * re-encode would silently bless the damage.
 * When not to use it: updating g members of one class reads 2g + 1 blocks, a
 * re-encode of that class k/m; past g > (k/m - 1) / 2 xec_encode moves fewer
 * bytes.  The library does not switch for the caller -- that would drop the
 * syndrome.
 *
 * h_items[t] = c << 8 | i with i < k and c < S, n_items of them, strictly
 * ascending (batch order; no duplicates); anything else is XEC_INVALID_COUNTS.
 * The packing needs k <= 256 and S <= 2^24, else XEC_INVALID_SIZE.  The new
 * content of item t is the bs bytes at d_new + t*bs (packed in list order);
 * d_new must be 64-byte aligned (XEC_INVALID_ALIGNMENT) and its n_items*bs
 * bytes must overlap neither the data nor the parity range (XEC_INVALID_SIZE,
 * as is a NULL d_new).  Order of the checks: XEC_NOT_INITIALIZED, then
 * xec_check_args; n_items == 0 or S == 0 is then XEC_SUCCESS without a device
 * call; then the above, all decided on the host before any device call, so a
 * rejected call queues nothing and changes nothing.  h_items is read before
 * the call returns; the call is asynchronous on `stream`.
 * Up to 1,024 items travel in the kernel arguments (capacities 64 / 256 /
 * 1024): nothing is copied and d_scratch may be NULL.  A longer list is staged
 * in the pinned memory the library keeps and uploaded on `stream` itself into
 * d_scratch in one copy: d_scratch must then be 4-byte aligned
 * (XEC_INVALID_ALIGNMENT), not NULL and of at least
 * xec_update_scratch_bytes(n_items) bytes (XEC_INVALID_SIZE).  Not capturable,
 * as xec_repair: on a capturing stream a call with work returns
 * XEC_DEVICE_ERROR with nothing queued.
 * Once its own checks above have passed, the call runs the kernels of
 * xec_update_range over offset = 0, len = bs without digests; of xec_set_launch
 * all four arguments apply, xec_set_rotation does not. */
xec_status xec_update(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                      size_t k, size_t m, const uint32_t* h_items, size_t n_items,
                      void* d_scratch, size_t scratch_bytes, hipStream_t stream);

/* Scratch bytes xec_update needs for a list of n_items: 4 * n_items. */
size_t xec_update_scratch_bytes(size_t n_items);

/* Device-resident form of xec_update: no host work, so it can be captured in a
 * hipGraph (a replay applies whatever the mask and d_new hold at replay
 * time), and no limit on k or S.  d_mask: S*k device bytes, index c*k + i;
 * NONZERO means "take the new block" -- the opposite sense of the loss
 * bitmaps, where 0 marks the block to act on.  d_new mirrors d_data's layout
 * (a shadow buffer of S*k*bs bytes, block i of stripe c at (c*k + i)*bs); only
 * its marked blocks are read.  One kernel over class tiles (stripe, class,
 * 1 KiB chunk): a tile scans its class's k/m mask bytes, folds the marked
 * members and writes nothing where none is marked.  There is no verdict: an
 * update cannot be unrecoverable.  A NULL d_mask with S > 0 is
 * XEC_INVALID_SIZE; d_new's alignment and overlap (over S*k*bs bytes),
 * xec_check_args and initialisation as xec_update; nothing is queued when an
 * argument is rejected.  Bytes identical to xec_update's with the same set of
 * blocks.  The kernel is xec_update_range_device's over offset = 0, len = bs
 * without digests; xec_set_rotation does not apply. */
xec_status xec_update_device(void* d_data, void* d_parity, const void* d_new, size_t S,
                             size_t bs, size_t k, size_t m, const uint8_t* d_mask,
                             hipStream_t stream);

/* Diagnostics: which tiling the calling thread's most recent xec_update or
 * xec_update_device launched -- 0 none (an error, or an empty update),
 * XEC_TILING_ARG_LIST or XEC_TILING_LIST (xec_update), XEC_TILING_CLASS
 * (xec_update_device; enum below).  xec_decode_tiling_used and
 * xec_repair_tiling_used are not affected. */
int xec_update_tiling_used(void);

/* Block digests (no reference counterpart: its only checksum lives inside its
 * validation payload).  XOR parity says THAT a class is damaged, never which
 * of its blocks; a parity store keeps a small checksum per block for that.
 * For a block of bs bytes read as bs/8 little-endian u64 words w[0..]:
 *     digest(block) = sum over n of splitmix_at(w[n], n)      (mod 2^64)
 * where splitmix_at(seed, n) is the splitmix64 finaliser of
 * seed + (n+1)*0x9E3779B97F4A7C15 (output n of xec_fill_splitmix64's stream
 * from state `seed`).
 *  - Bit-exact under any reduction order: the sum is modulo 2^64, associative
 *    and commutative, so the device's split over lanes, waves, workgroups and
 *    atomic adds gives the host's bits.
 *  - Detection: for fixed n the term is a bijection of w[n], so damage
 *    confined to ONE 8-byte word always changes the digest; wider damage goes
 *    unnoticed with probability about 2^-64.  Not cryptographic: it guards
 *    against corruption, not against an adversary.
 * xec_digest_host: host only, no GPU and no xec_init needed; bs % 8 == 0 (a
 * tail of bs % 8 bytes is ignored). */
uint64_t xec_digest_host(const void* block, size_t bs);

/* Digests of a batch's blocks on the device.  d_digests: S*(k+m) u64 of device
 * memory in the bitmap's layout -- stripe c at c*(k+m), its k data slots then
 * its m parity slots.  d_select == NULL digests every block; otherwise it is
 * S*(k+m) device bytes in the same layout and NONZERO means "digest this
 * block" (the sense of xec_update_device's mask): the slot of an unselected
 * block is neither read nor written, and the block itself is not read.  That
 * is the refresh after xec_update: select the changed data blocks and the
 * parity blocks of their classes, and the batch is not read again.
 * Enqueues on `stream` (no host work: capturable; asynchronous): the selected
 * slots zeroed (one memset when d_select is NULL, which a capture records as a
 * memset node -- see xec_verify; else a small kernel), then one kernel over
 * (block, 64 KiB segment) tiles, each adding its segment's sum to the block's
 * slot with one 64-bit atomic add; at most 131,072 workgroups walk the tiles
 * (xec_set_launch's max_grid overrides that; of its other arguments
 * cache_policy and block_threads apply, unroll does not).  Reads up to (k+m)*bs*S bytes once, writes
 * only d_digests.
 * Checks, all on the host before anything is queued, in this order:
 * XEC_NOT_INITIALIZED; xec_check_args; d_digests NULL with S > 0 ->
 * XEC_INVALID_SIZE; d_digests not 8-byte aligned -> XEC_INVALID_ALIGNMENT.
 * S == 0 is XEC_SUCCESS with nothing queued. */
xec_status xec_digest(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, const uint8_t* d_select, uint64_t* d_digests, hipStream_t stream);

/* Scratch bytes xec_locate needs: 8 * S * (k+m), one u64 per block. */
size_t xec_locate_work_bytes(size_t S, size_t k, size_t m);

/* Which block is damaged: recomputes digests into d_work (device scratch of at
 * least xec_locate_work_bytes(S, k, m) bytes, 8-byte aligned), compares them
 * with the stored d_digests and writes d_bitmap, S*(k+m) device bytes: 1 where
 * the digest matches or the block was not checked, 0 where it differs -- the
 * convention xec_repair_device and xec_erase read.  *d_count (device uint32,
 * 4-byte aligned, or NULL) = the number of 0 bytes written.  Neither data nor
 * parity is ever written.
 * d_flags == NULL checks every block; that also finds what xec_verify cannot
 * see, two errors of one class that cancel in the XOR.  Otherwise d_flags is
 * xec_verify's S*m flag bytes, and only the k/m + 1 blocks of the classes with
 * a nonzero flag are read and checked (a workgroup of an unflagged class
 * returns after one byte read): the gate.  A block of an unflagged class
 * reads 1 whatever its stored digest says.
 * The chain xec_verify -> xec_locate(flags) -> xec_repair_device runs on one
 * stream with no host step.  For a flagged class, one of:
 *  - exactly one block differs: xec_repair_device rebuilds it from the others
 *    and the class XORs to zero again;
 *  - two or more blocks differ: *d_status = 4 and nothing is written (repair
 *    is all-or-nothing over the batch);
 *  - no block differs: the digests are stale, or the damage is older than
 *    they are.  Nothing is repaired and the class stays flagged; *d_count
 *    smaller than xec_verify's count of flagged classes tells the caller.
 * Digests of rebuilt blocks need no refresh: a rebuilt block matches its
 * stored digest again.
 * Enqueues on `stream` (no host work: capturable on its own; asynchronous):
 * *d_count zeroed by a memset; the checked slots of d_work zeroed (a memset
 * with d_flags NULL, else a small kernel); the digest kernel of xec_digest;
 * a small kernel that compares and counts.  A captured xec_locate therefore
 * contains memset nodes, as a captured xec_verify does: the open observation
 * recorded at xec_verify applies, and the chain is meant for a plain stream.
 * Checks, all on the host before anything is queued, in this order:
 * XEC_NOT_INITIALIZED; xec_check_args; d_digests or d_work NULL with S > 0, or
 * work_bytes too small -> XEC_INVALID_SIZE; d_digests or d_work not 8-byte
 * aligned, or d_count not 4-byte aligned -> XEC_INVALID_ALIGNMENT; d_bitmap
 * NULL with S > 0 -> XEC_INVALID_SIZE.  S == 0 is XEC_SUCCESS, with
 * *d_count = 0 when d_count is given. */
xec_status xec_locate(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, const uint64_t* d_digests, const uint8_t* d_flags,
                      uint8_t* d_bitmap, uint32_t* d_count, void* d_work, size_t work_bytes,
                      hipStream_t stream);

/* Degraded read (no reference counterpart: its decode rebuilds whole blocks in
 * place): serve a read while a block is missing.  Item t names block i of
 * stripe c as h_items[t] = c << 8 | i, xec_repair's packing -- i in [0, k+m),
 * i >= k naming parity block i - k -- and bytes [offset, offset + len) of that
 * block arrive at d_out + t*len.  A present block is copied.  A lost block's
 * range is reconstructed from the same range of the other k/m blocks of its
 * class, straight into d_out: k/m * len bytes read and len written, where
 * xec_repair reads k/m * bs and writes bs, in place.  d_data, d_parity and the
 * bitmap are never written, so a reader needs no write access to the store;
 * the bytes a lost block holds on entry are never read.
 * Items may come in any order and may repeat (a read has no writer conflict).
 * A block is lost iff its bitmap byte is 0, xec_repair's rule; h_bitmap == NULL
 * means everything is present and the call is a pure gather.  An item is
 * servable if its block is present, or if it is lost and every other block of
 * its class is present (the k/m - 1 other data members and the parity block;
 * all k/m data members when the item is the parity block).
 * Unlike xec_repair, blocks of other classes and other stripes play no part:
 * a batch xec_repair refuses (XEC_DECODE_FAILURE, some class lost two blocks)
 * still serves every read that does not ask for a LOST block of such a class
 * -- its present blocks included.  All-or-nothing over the REQUESTED items: if
 * one is not servable nothing is written to d_out.
 * Checks, all on the host before any device call, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. xec_check_args;
 *  3. n_items == 0 or S == 0 -> XEC_SUCCESS, nothing queued;
 *  4. k + m > 256 or S > 2^24 -> XEC_INVALID_SIZE (the packing);
 *  5. len == 0, offset % 16, len % 16 or offset + len > bs -> XEC_INVALID_SIZE;
 *  6. d_out or h_items NULL -> XEC_INVALID_SIZE;
 *  7. d_out not 16-byte aligned -> XEC_INVALID_ALIGNMENT;
 *  8. d_out's n_items*len bytes overlap the data or the parity range ->
 *     XEC_INVALID_SIZE;
 *  9. an item with c >= S or i >= k + m -> XEC_INVALID_COUNTS;
 * 10. an item that is not servable -> XEC_DECODE_FAILURE;
 * 11. more than 1,024 items: d_scratch not 4-byte aligned ->
 *     XEC_INVALID_ALIGNMENT; NULL or fewer than xec_read_scratch_bytes(n_items)
 *     bytes -> XEC_INVALID_SIZE.
 * A rejected call queues nothing and writes nothing.  Up to 1,024 items travel
 * in the kernel arguments (capacities 64 / 256 / 1024) with one bit per item
 * saying "reconstruct" (the item word has no spare bit at S = 2^24): nothing
 * is copied and d_scratch may be NULL.  A longer list is staged in the pinned
 * memory the library keeps -- the items, then their bits -- and uploaded on
 * `stream` itself into d_scratch in one copy.  h_bitmap and h_items are read
 * before the call returns; the call is asynchronous on `stream`.  Not
 * capturable, as xec_repair: on a capturing stream a call with work returns
 * XEC_DEVICE_ERROR with nothing queued (xec_read_device is the capturable
 * form).  One kernel over (item, chunk of the range) tiles, chunks of 1 KiB at
 * the default launch shape; of xec_set_launch all four arguments apply,
 * xec_set_rotation does not. */
xec_status xec_read(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                    size_t m, const uint8_t* h_bitmap, const uint32_t* h_items, size_t n_items,
                    size_t offset, size_t len, void* d_out, void* d_scratch, size_t scratch_bytes,
                    hipStream_t stream);

/* Scratch bytes xec_read needs for a list of n_items: 4 * (n_items +
 * ceil(n_items / 32)), the items and one bit each.  Needed only past 1,024
 * items. */
size_t xec_read_scratch_bytes(size_t n_items);

/* Device-resident form of xec_read: bitmap and items in device memory, no host
 * work, so it can be captured in a hipGraph; a replay serves whatever d_items
 * and d_bitmap hold at replay time.  d_bitmap == NULL: everything present, a
 * pure gather.  Enqueues on `stream`: *d_status = 0 (a memset, as
 * xec_decode_device); a check kernel over the items that leaves *d_status at
 * the MAXIMUM over the items of 0 (servable), 3 (c >= S or i >= k + m; such an
 * item is never dereferenced) and 4 (in range but not servable); then the read
 * kernel, which does nothing if *d_status != 0 (all-or-nothing over the
 * requested items) and otherwise delivers the bytes xec_read delivers for the
 * same items.
 * Host checks, before anything is queued, in this order: XEC_NOT_INITIALIZED;
 * xec_check_args; d_status NULL or not 4-byte aligned -> XEC_INVALID_ALIGNMENT;
 * n_items == 0 or S == 0 -> XEC_SUCCESS with only *d_status = 0 queued;
 * steps 4 to 8 of xec_read with d_items in h_items' place; d_items not 4-byte
 * aligned -> XEC_INVALID_ALIGNMENT.  No limit on n_items and no scratch. */
xec_status xec_read_device(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                           size_t m, const uint8_t* d_bitmap, const uint32_t* d_items,
                           size_t n_items, size_t offset, size_t len, void* d_out,
                           int32_t* d_status, hipStream_t stream);

/* Host-only scan xec_read runs over its items (no GPU and no xec_init needed):
 * XEC_INVALID_COUNTS if an item has c >= S or i >= k + m (or k, m are invalid
 * as in xec_check_args, or h_items is NULL with n_items > 0), else
 * XEC_DECODE_FAILURE if an item is not servable, else XEC_SUCCESS with
 * *n_lost (may be NULL) = the number of items that need a reconstruction, a
 * repeated item counted each time.  h_bitmap == NULL: everything is present.
 * Only the blocks of the requested items' classes are looked at. */
xec_status xec_check_read_items(const uint8_t* h_bitmap, size_t S, size_t k, size_t m,
                                const uint32_t* h_items, size_t n_items, size_t* n_lost);

/* Diagnostics: which tiling the calling thread's most recent xec_read or
 * xec_read_device launched -- 0 none (an error, or nothing to read),
 * XEC_TILING_ARG_LIST or XEC_TILING_LIST (xec_read), XEC_TILING_LIST
 * (xec_read_device; enum below).  The other *_tiling_used values are not
 * affected. */
int xec_read_tiling_used(void);

/* Vectored degraded read: xec_read with a range per entry, the shape of a
 * store's read queue.  Everything xec_read says holds per entry, with the
 * entry's own [offset, offset + len): a present block's range is copied, a
 * lost block's range is reconstructed from the same range of the other k/m
 * blocks of its class straight into d_out; data, parity and the bitmap are
 * never written and the bytes a lost block holds are never read.  Entries may
 * come in any order and may repeat; h_bitmap == NULL means everything is
 * present; servability is xec_read's rule; the call is all-or-nothing over the
 * requested entries.
 * Output is packed in list order: entry t's bytes land at d_out + the sum of
 * len over the entries before it.  These offsets are 64-bit, the total may
 * pass 4 GiB.  out_bytes is the capacity of d_out; nothing past the total is
 * written.
 * When to use which (tools/readv_bench.py on one MI355X, 16+1 x 1 MiB x 256,
 * 1,024 lost entries; DESIGN.md §3 *Vectored read*): when the ranges differ,
 * one xec_readv replaces one xec_read per distinct range -- 1,024 entries over
 * 64 ranges took 120 us from call to sync against 668 us for the 64 xec_read
 * calls (44 against 613 us with every block present).  When every entry has
 * the same range use xec_read: its tile needs no search and 1,024 items still
 * travel in its kernel arguments, 7.9 us of kernel and 27 us from call to sync
 * against xec_readv's 12.9 and 53 us.
 * Checks, all on the host before anything is queued, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. xec_check_args;
 *  3. n_items == 0 or S == 0 -> XEC_SUCCESS, nothing queued;
 *  4. k + m > 256, S > 2^24 or bs >= 2^32 -> XEC_INVALID_SIZE;
 *  5. d_out or h_iov NULL -> XEC_INVALID_SIZE;
 *  6. d_out not 16-byte aligned -> XEC_INVALID_ALIGNMENT;
 *  7. an entry with len == 0, offset % 16, len % 16 or offset + len > bs (in 64
 *     bits) -> XEC_INVALID_SIZE;
 *  8. sum len > out_bytes, a total number of tiles (below) that does not fit 32
 *     bits, or d_out's sum len bytes overlapping the data or the parity range
 *     -> XEC_INVALID_SIZE;
 *  9. an entry with c >= S or i >= k + m -> XEC_INVALID_COUNTS;
 * 10. an entry that is not servable -> XEC_DECODE_FAILURE;
 * 11. more than 256 entries: d_scratch not 4-byte aligned ->
 *     XEC_INVALID_ALIGNMENT; NULL or fewer than xec_readv_scratch_bytes(n_items)
 *     bytes -> XEC_INVALID_SIZE.
 * A rejected call queues nothing and writes nothing.  The kernel walks a table
 * of six words per entry -- item, offset, len, the 64-bit output start and the
 * entry's first tile, a tile being (entry, chunk of 16 * block_threads * unroll
 * bytes of its range; 1 KiB at the default launch shape) -- plus one loss bit.
 * Up to 256 entries travel in the kernel arguments (capacities 64 / 256; 1,024
 * would ship 24 KiB with every launch) and d_scratch may be NULL.  A longer
 * table is staged in the pinned memory the library keeps and uploaded on
 * `stream` itself into d_scratch in one copy.  h_bitmap and h_iov are read
 * before the call returns; the call is asynchronous on `stream`.  Not
 * capturable, as xec_read: on a capturing stream a call with work returns
 * XEC_DEVICE_ERROR with nothing queued.  Of xec_set_launch all four arguments
 * apply, xec_set_rotation does not; xec_set_kernel_events times the read
 * kernel. */
typedef struct {
  uint32_t item;   /* c << 8 | i, xec_read's packing: i in [0, k+m), i >= k = parity block i-k */
  uint32_t offset; /* bytes into the block, multiple of 16 */
  uint32_t len;    /* bytes, multiple of 16, > 0; offset + len <= bs */
} xec_iov;         /* 12 bytes, 4-byte aligned */

xec_status xec_readv(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                     size_t m, const uint8_t* h_bitmap, const xec_iov* h_iov, size_t n_items,
                     void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes,
                     hipStream_t stream);

/* Scratch bytes xec_readv needs for a table of n_items entries:
 * 4 * (6 * n_items + 1 + ceil(n_items / 32)), 0 for n_items == 0.  Needed only
 * past 256 entries. */
size_t xec_readv_scratch_bytes(size_t n_items);

/* Device-resident form of xec_readv: bitmap and entries in device memory, no
 * host work and no limit on n_items, so it can be captured in a hipGraph; a
 * replay serves whatever d_iov and d_bitmap hold at replay time, lengths
 * included.  d_bitmap == NULL: everything present.
 * Host checks, before anything is queued, in this order: XEC_NOT_INITIALIZED;
 * xec_check_args; d_status NULL or not 4-byte aligned -> XEC_INVALID_ALIGNMENT;
 * n_items == 0 or S == 0 -> XEC_SUCCESS with only *d_status = 0 queued; step 4
 * of xec_readv; d_out, d_iov or d_work NULL -> XEC_INVALID_SIZE; work_bytes <
 * xec_readv_device_work_bytes(n_items) -> XEC_INVALID_SIZE; d_out not 16-byte,
 * d_iov not 4-byte or d_work not 8-byte aligned -> XEC_INVALID_ALIGNMENT;
 * d_out's out_bytes overlapping data or parity -> XEC_INVALID_SIZE;
 * n_items * ceil(bs / 1024) >= 2^32 -> XEC_INVALID_SIZE (a 32-bit tile count
 * cannot overflow at any launch shape).
 * Enqueues on `stream`: *d_status = 0 (a memset, as xec_read_device); a check
 * kernel, one thread per entry, that leaves *d_status at the MAXIMUM over the
 * entries of 0 (servable), 1 (a range that breaks step 7 of xec_readv), 3
 * (c >= S or i >= k + m) and 4 (in range but not servable) -- an entry with a
 * nonzero verdict is never dereferenced beyond its own 12 bytes -- and writes
 * each entry's tile count and length into d_work; a scan kernel that turns
 * those into exclusive prefixes in list order and raises *d_status to 1 if
 * the byte total exceeds out_bytes; then the read kernel, which does nothing
 * if *d_status != 0 and otherwise delivers the bytes xec_readv delivers.  Its
 * grid is fixed at launch from the bound the host knows, out_bytes / tile
 * bytes + n_items possible tiles, clamped as xec_decode_device_list clamps its
 * grid (xec_set_launch's max_grid overrides it). */
xec_status xec_readv_device(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                            size_t m, const uint8_t* d_bitmap, const xec_iov* d_iov,
                            size_t n_items, void* d_out, size_t out_bytes, void* d_work,
                            size_t work_bytes, int32_t* d_status, hipStream_t stream);

/* Work bytes xec_readv_device needs: 12 * (n_items + 1) rounded up to a
 * multiple of 8 (a 64-bit output start and a 32-bit tile start per entry, and
 * the totals), 0 for n_items == 0. */
size_t xec_readv_device_work_bytes(size_t n_items);

/* xec_readv_device over shards: serve a read queue whose ranges differ from a
 * store with a shard down.  d_bitmap (NULL = everything present), d_iov (item,
 * offset, len per entry; present and lost blocks, data and parity, repeats, any
 * order), d_out and out_bytes, d_work (xec_readv_device_work_bytes(n_items)
 * bytes: the size serves both layouts), the verdicts 0 / 1 / 3 / 4 left as a
 * maximum in *d_status and the all-or-nothing behaviour over the entries are
 * xec_readv_device's, and so is what is queued: *d_status = 0 (a memset), the
 * same check and scan kernels -- neither touches a block -- then a read kernel
 * that does nothing if *d_status != 0, its grid fixed from the same bound.  A
 * lost block is never read and nothing but d_out, d_work and *d_status is
 * written.  Checks, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. step 1 of xec_check_shards;
 *  3. xec_readv_device's own checks in its order, from d_status up to the
 *     alignments of d_out, d_iov and d_work;
 *  4. steps 3 to 7 of xec_check_shards;
 *  5. d_out's out_bytes meet the hull of any shard -> XEC_INVALID_SIZE (the
 *     rule of xec_read_shards_device step 5: a d_out in a gap between two
 *     blocks of one shard is refused, ranges that only touch are allowed);
 *  6. n_items * ceil(bs / 1024) >= 2^32 -> XEC_INVALID_SIZE.
 * A rejected call queues nothing.  Bytes of a shard between its blocks are
 * never read; aliased into a batch it delivers exactly xec_readv_device's
 * bytes.  Capturable (one memset node).  xec_set_launch as xec_readv_device, no
 * column rotation, residency by xec_read_device's table, swept on the batch
 * layout only.  xec_readv_tiling_used is not affected.  Measured against
 * xec_readv_device on the same entries (same tool, file and configs; the read
 * kernel alone): 4 KiB of each of min(S, 1,024) lost blocks took 1.06 / 0.95 /
 * 1.10 aliased (the batch kernel's rounds spread 12 % at config 3) and 1.08 /
 * 1.09 / 1.18 on separate allocations; of present blocks 1.02 / 1.05 / 1.07 and
 * 1.06 / 1.03 / 1.05; one whole lost block per stripe 1.02 / 1.00 / 1.24 and
 * 1.05 / 1.03 / 1.21 -- config 4 is the 32-member reconstruction whose member
 * addresses are scalar loads, as for xec_read_shards_device; one whole present
 * block per stripe 1.00 / 1.09 / 1.00 and 0.98 / 1.12 / 1.00. */
xec_status xec_readv_shards_device(const void* const* h_shards, size_t data_stride,
                                   size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                   const uint8_t* d_bitmap, const xec_iov* d_iov, size_t n_items,
                                   void* d_out, size_t out_bytes, void* d_work, size_t work_bytes,
                                   int32_t* d_status, hipStream_t stream);

/* Host-only plan check xec_readv runs over its entries (no GPU and no xec_init
 * needed): steps 7, 9 and 10 of xec_readv in that order.  k, m invalid as in
 * xec_check_args, or h_iov NULL with n_items > 0 -> XEC_INVALID_COUNTS, as
 * xec_check_read_items.  On success *n_lost (may be NULL) = the entries that
 * need a reconstruction, a repeat counted each time, and *total_bytes (may be
 * NULL) = sum len. */
xec_status xec_check_readv(const uint8_t* h_bitmap, size_t S, size_t bs, size_t k, size_t m,
                           const xec_iov* h_iov, size_t n_items, size_t* n_lost,
                           size_t* total_bytes);

/* Diagnostics: which tiling the calling thread's most recent xec_readv or
 * xec_readv_device launched -- 0 none (an error, or nothing to read),
 * XEC_TILING_ARG_LIST or XEC_TILING_LIST (xec_readv), XEC_TILING_LIST
 * (xec_readv_device).  The other *_tiling_used values are not affected. */
int xec_readv_tiling_used(void);

/* Ranged update with digest upkeep (no reference counterpart): xec_update
 * over bytes [offset, offset + len) of each named block only, following
 * xec_read's range rules.  For every named block i of stripe c,
 *     parity[c][i % m][range] ^= data[c][i][range] ^ new;
 *     data[c][i][range] = new
 * Bytes outside the range, blocks not named and parity blocks of classes
 * without an item are neither read nor written: per item the call reads 3*len
 * and writes 2*len bytes, where xec_update moves 5*bs.  The delta keeps a
 * class's syndrome, as xec_update does.
 * Items are xec_update's: h_items[t] = c << 8 | i, i < k, c < S, strictly
 * ascending, and everything xec_update says about them holds.  Item t's new
 * bytes are the len bytes at d_new + t*len -- xec_read's packing of d_out, on
 * the input side.  Up to 1,024 items travel in the kernel arguments
 * (capacities 64 / 256 / 1024); a longer list goes through the pinned staging
 * into d_scratch (xec_update_scratch_bytes(n_items) bytes) in one copy on
 * `stream`.  Not capturable, as xec_update: on a capturing stream a call with
 * work returns XEC_DEVICE_ERROR with nothing queued.
 *
 * Digest upkeep.  d_digests == NULL: no digest is touched, and the kernel that
 * runs has no digest code in it.  Otherwise d_digests is S*(k+m) u64 in
 * xec_digest's layout, 8-byte aligned, and in the same pass
 *  - the slot of each updated data block gets
 *        += sum_n splitmix_at(new w[n], n) - sum_n splitmix_at(old w[n], n)
 *    over the words n of the range (n counted from the start of the block);
 *  - the parity slot c*(k+m) + k + j of each class with an item gets the same
 *    difference over the parity bytes after and before;
 * so slots that held the digests of the blocks before the call hold the
 * digests of the blocks after it, bit-exact against xec_digest_host.  Slots of
 * other blocks are neither read nor written.  The adds are 64-bit atomics
 * (one per wave and slot, i.e. one per KiB of the range and slot at the
 * default launch shape), so the order of tiles does not matter.  With
 * offset = 0, len = bs this is the one-pass form of xec_update followed by
 * xec_digest(select).  A whole 1 MiB block then sends 1,024 adds to one slot,
 * which costs time (config 3: about 1.5x the same call without upkeep), but
 * the one pass still measured faster than the two at configs 2, 3 and 4
 * (DESIGN.md §3 *Ranged update*).
 *
 * What upkeep keeps, and what it cannot know.
 *  - A slot that disagreed with its block before the call disagrees by the
 *    same amount after it.  Upkeep never blesses damage, and a stale digest
 *    stays stale.
 *  - If the old bytes inside the range were already damaged, the delta is
 *    taken from the damaged bytes.  The data block now holds exactly the new
 *    bytes, the damage has moved into the parity block (its class stays
 *    flagged by xec_verify), and the data block's slot keeps disagreeing.
 *  - xec_locate then names the data block, and xec_repair_device would rebuild
 *    it from a parity that carries the damage.  A second xec_locate after the
 *    repair still counts the block: rebuilt blocks do not match their stored
 *    digest in this one case.
 *  - This is inherent in an incremental checksum.  A caller that cannot accept
 *    it passes d_digests = NULL and refreshes with xec_digest(select), at the
 *    price of reading the whole blocks.
 *
 * Checks, all on the host before anything is queued, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. xec_check_args;
 *  3. n_items == 0 or S == 0 -> XEC_SUCCESS, nothing queued;
 *  4. k > 256 or S > 2^24 -> XEC_INVALID_SIZE (the packing);
 *  5. len == 0, offset % 16, len % 16 or offset + len > bs -> XEC_INVALID_SIZE;
 *  6. d_new or h_items NULL -> XEC_INVALID_SIZE;
 *  7. d_new not 16-byte aligned, or d_digests not NULL and not 8-byte aligned
 *     -> XEC_INVALID_ALIGNMENT;
 *  8. d_new's n_items*len bytes overlap the data or the parity range, or
 *     d_digests' 8*S*(k+m) bytes overlap data, parity or d_new ->
 *     XEC_INVALID_SIZE (ranges that only touch are allowed);
 *  9. the item rules of xec_update -> XEC_INVALID_COUNTS;
 * 10. more than 1,024 items: the scratch rules of xec_update.
 * A rejected call queues nothing and changes nothing.  One kernel over (list
 * position, chunk of the range) tiles; xec_update_tiling_used reports as for
 * xec_update; of xec_set_launch all four arguments apply, xec_set_rotation
 * does not; residency is uncapped. */
xec_status xec_update_range(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                            size_t k, size_t m, const uint32_t* h_items, size_t n_items,
                            size_t offset, size_t len, uint64_t* d_digests, void* d_scratch,
                            size_t scratch_bytes, hipStream_t stream);

/* Device-resident form of xec_update_range: no host work, so it can be
 * captured in a hipGraph, and no limit on k or S.  d_mask is S*k device bytes,
 * NONZERO = take the block (xec_update_device's mask); d_new is a shadow
 * mirroring d_data's layout (S*k*bs bytes), of which only [offset,
 * offset + len) of the marked blocks is read.  One kernel over (stripe, class,
 * chunk of the range) tiles; xec_update_tiling_used reports XEC_TILING_CLASS.
 * Checks: 1, 2, S == 0 -> XEC_SUCCESS with nothing queued, then 5, d_new or
 * d_mask NULL -> XEC_INVALID_SIZE, 7 and 8 with d_new's extent S*k*bs. */
xec_status xec_update_range_device(void* d_data, void* d_parity, const void* d_new, size_t S,
                                   size_t bs, size_t k, size_t m, const uint8_t* d_mask,
                                   size_t offset, size_t len, uint64_t* d_digests,
                                   hipStream_t stream);

/* Degraded write (no reference counterpart): xec_update_range under a loss
 * bitmap, the write-side counterpart of xec_read.  It follows xec_read's rule:
 * a lost block (bitmap byte 0) is never read and never written.  Items, range,
 * d_new's packing and d_digests are xec_update_range's: h_items[t] = c << 8 | i,
 * i < k, strictly ascending; one range [offset, offset + len) per call,
 * multiples of 16; item t's new bytes at d_new + t*len; d_digests may be NULL.
 * h_bitmap == NULL means everything is present, and the call then leaves
 * exactly the bytes and digest slots xec_update_range leaves.
 *
 * Every (stripe, class) with at least one item runs in one of three modes; W is
 * the set of its written members, its blocks are its k/m data members and its
 * parity block.
 *  - Delta: the parity block is present and no member of W is lost.
 *    parity[range] ^= old ^ new per written member and data[range] = new,
 *    exactly as xec_update_range: 3*len read and 2*len written per item.  A
 *    lost member that is NOT written is not touched -- the delta never needs
 *    it.  The class's syndrome is kept.
 *  - Data-only: the parity block is lost.  Each written (present) member takes
 *    its new bytes; parity is neither read nor written, and a later xec_repair
 *    re-encodes it.  len read (the new bytes) and len written per item; with
 *    d_digests the old range is read as well.
 *  - Rebuild-write: one member x of W is lost and every other block of the
 *    class is present.
 *        parity[range] = new_x ^ XOR_{r != x} (new_r if r in W else data_r)[range]
 *    Present written members take their new bytes; block x is not touched.
 *    Outside the range nothing changes, so the bytes a later xec_repair
 *    reconstructs for x are its old (virtual) bytes outside the range and new_x
 *    inside it.  Old parity is read only with d_digests.  The parity's range is
 *    RECOMPUTED, so a syndrome the class carried inside the range is gone: this
 *    is the one mode that cannot keep it (outside the range it stays).
 *
 * Servability is xec_read's rule over the written items: an item is servable if
 * its block is present, or if it is lost and every other block of its class is
 * present.  All-or-nothing over the requested items: one unservable item gives
 * XEC_DECODE_FAILURE, nothing is queued and nothing changes.  As with xec_read,
 * blocks of other classes and other stripes play no part: a batch xec_repair
 * refuses still takes every write that does not target a LOST block of a
 * doubly-lost class -- with a data member and the parity both lost, a write to
 * a third, present member runs data-only.
 *
 * Digest upkeep (d_digests != NULL, xec_digest's layout).  Delta: as
 * xec_update_range.  Data-only: each written block's slot gets
 * += mix(new) - mix(old) over the range; the lost parity block's slot is
 * neither read nor written and is STALE after the repair: refresh it with
 * xec_digest(select) then.  Rebuild-write: written present blocks as data-only;
 * the lost block x gets += mix(new_x) - mix(P_old ^ XOR_{r != x} old_r), the
 * difference against the bytes it virtually held; the parity slot gets
 * += mix(P_new) - mix(P_old).  So with slots that held the digests of the
 * blocks before the loss, xec_write and then xec_repair under the same bitmap
 * leave a full xec_locate counting exactly the parity blocks of the data-only
 * classes, and none once those are refreshed.  xec_update_range's caveat
 * carries over: damaged old bytes inside the range move into parity (delta) or
 * stay in the slot.
 *
 * Checks, all on the host before anything is queued, in this order:
 *  1. XEC_NOT_INITIALIZED;
 *  2. xec_check_args;
 *  3. n_items == 0 or S == 0 -> XEC_SUCCESS, nothing queued;
 *  4. k > 256 or S > 2^24 -> XEC_INVALID_SIZE (the packing);
 *  5. to 8. steps 5 to 8 of xec_update_range (the range; d_new or h_items NULL;
 *     the alignments; the overlaps);
 *  9. the item rules of xec_update -> XEC_INVALID_COUNTS (anywhere in the list:
 *     it outranks step 10);
 * 10. an item that is not servable -> XEC_DECODE_FAILURE;
 * 11. more than 1,024 items: d_scratch not 4-byte aligned ->
 *     XEC_INVALID_ALIGNMENT; NULL or fewer than xec_write_scratch_bytes(n_items)
 *     bytes -> XEC_INVALID_SIZE.
 * A rejected call queues nothing and changes nothing.  The host scan attaches
 * two bits to each item -- "this block is lost", "this class's parity is lost"
 * -- and the tile that owns the class derives the mode from the bits of its
 * items.  Up to 1,024 items and their bits travel in the kernel arguments
 * (capacities 64 / 256 / 1024); a longer list is staged in pinned memory, items
 * then bits, and uploaded into d_scratch in one copy on `stream`.  h_bitmap and
 * h_items are read before the call returns.  Not capturable, as xec_update: on
 * a capturing stream a call with work returns XEC_DEVICE_ERROR with nothing
 * queued.  One kernel over (list position, chunk of the range) tiles; of
 * xec_set_launch all four arguments apply, xec_set_rotation does not; residency
 * is uncapped. */
xec_status xec_write(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                     size_t k, size_t m, const uint8_t* h_bitmap, const uint32_t* h_items,
                     size_t n_items, size_t offset, size_t len, uint64_t* d_digests,
                     void* d_scratch, size_t scratch_bytes, hipStream_t stream);

/* Scratch bytes xec_write needs for a list of n_items: 4 * (n_items +
 * ceil(n_items / 16)), the items and two bits each.  Needed only past 1,024
 * items. */
size_t xec_write_scratch_bytes(size_t n_items);

/* Device-resident form of xec_write: nothing happens on the host, so it can be
 * captured in a hipGraph, and there is no limit on k or S.  d_mask and the
 * shadow d_new are xec_update_range_device's; d_bitmap is S*(k+m) device bytes
 * (0 = lost) or NULL for all present.  Enqueues on `stream`: *d_status = 0 (a
 * memset, as xec_read_device); a check kernel that sets *d_status = 4 if any
 * marked block is lost while another block of its class is lost (not launched
 * with d_bitmap NULL); then the write kernel over (stripe, class, chunk of the
 * range) tiles, which does nothing if *d_status != 0 and otherwise reads each
 * class's mask and bitmap bytes and picks its mode.
 * Checks: 1, 2, S == 0 -> XEC_SUCCESS with nothing queued, then the checks of
 * xec_update_range_device, then d_status NULL or not 4-byte aligned ->
 * XEC_INVALID_ALIGNMENT. */
xec_status xec_write_device(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                            size_t k, size_t m, const uint8_t* d_bitmap, const uint8_t* d_mask,
                            size_t offset, size_t len, uint64_t* d_digests, int32_t* d_status,
                            hipStream_t stream);

/* Host-only scan xec_write runs over its items (no GPU and no xec_init needed):
 * XEC_INVALID_COUNTS if an item breaks xec_update's rules (i >= k, c >= S, not
 * strictly ascending; or k, m are invalid as in xec_check_args, or h_items is
 * NULL with n_items > 0) anywhere in the list, else XEC_DECODE_FAILURE if an
 * item is not servable, else XEC_SUCCESS with *n_rebuild = the lost items
 * (rebuild-write) and *n_data_only = the items whose class lost its parity
 * block -- items, not classes; either pointer may be NULL.  h_bitmap == NULL:
 * everything is present. */
xec_status xec_check_write_items(const uint8_t* h_bitmap, size_t S, size_t k, size_t m,
                                 const uint32_t* h_items, size_t n_items, size_t* n_rebuild,
                                 size_t* n_data_only);

/* Diagnostics: which tiling the calling thread's most recent xec_write or
 * xec_write_device launched -- 0 none (an error, or nothing to write),
 * XEC_TILING_ARG_LIST or XEC_TILING_LIST (xec_write), XEC_TILING_CLASS
 * (xec_write_device).  The other *_tiling_used values are not affected. */
int xec_write_tiling_used(void);

/* The digest terms of a range: the sum over the len/8 little-endian words w[n]
 * at `bytes` of splitmix_at(w[n], offset/8 + n)  (mod 2^64) -- `bytes` points
 * at the range's first byte, `offset` is where that byte sits in its block.
 * Host only, no xec_init needed; offset % 8 == 0 and len % 8 == 0 (tails are
 * ignored as in xec_digest_host).  xec_digest_host(b, bs) ==
 * xec_digest_range_host(b, 0, bs); the function is additive over any split of
 * a range; and the upkeep above is range(new) - range(old), so a caller that
 * patches host-side copies can keep its digests the same way. */
uint64_t xec_digest_range_host(const void* bytes, size_t offset, size_t len);

/* Host-only recoverability scan used by xec_decode (no GPU needed):
 * returns XEC_DECODE_FAILURE if some stripe is unrecoverable, else
 * XEC_SUCCESS and sets *needs_recovery to 1 iff some stripe needs recovery. */
xec_status xec_check_bitmap(const uint8_t* h_bitmap, size_t S, size_t k, size_t m,
                            int* needs_recovery);

/* Host-only argument check, identical to xorec_check_args
 * (xorec_utils.hpp:61-86); pointers are only tested for 64-B alignment. */
xec_status xec_check_args(const void* data, const void* parity, size_t bs, size_t k, size_t m);

/* Device-side erasure injection (the GPU analogue of
 * AbstractBenchmark::simulate_data_loss, abstract_bm.cpp:20-39, without the
 * per-block host memsets of xorec_gpu_cmp_bm.cpp:71-89): zero every block
 * whose d_bitmap byte is 0, data and parity alike. */
xec_status xec_erase(void* d_data, void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                     const uint8_t* d_bitmap, hipStream_t stream);

/* Host-only erasure draw for one stripe's (k+m)-byte bitmap: the reference's
 * select_lost_blocks (src/utils/utils.cpp:100-127) with an explicit seed in
 * place of its wall clock -- `lost` draws from PCG32(RANDOM_SEED + seed,
 * stream 1) over the blocks still eligible, each draw marking its block 0 and
 * removing its parity class, so the set is always recoverable.  lost == 0
 * leaves the bitmap as it is; lost > m is XEC_INVALID_COUNTS (where the
 * reference prints and exits). */
xec_status xec_select_lost_blocks(size_t k, size_t m, size_t lost, uint8_t* h_bitmap,
                                  uint64_t seed);

/* Synthetic input generator (tests and bench): stripe c's stripe_bytes are
 * little-endian u64 splitmix64 outputs from state seed_base + c.
 * stripe_bytes % 8 == 0 and d_buf 8-B aligned, else XEC_INVALID_SIZE /
 * XEC_INVALID_ALIGNMENT. */
xec_status xec_fill_splitmix64(void* d_buf, size_t S, size_t stripe_bytes, uint64_t seed_base,
                               hipStream_t stream);

/* Device-side validation payload: the reference's
 * write_validation_pattern / validate_block (src/utils/utils.cpp:35-97) run on
 * the GPU over nblocks consecutive blocks of bs bytes.  Block b gets PCG32
 * bytes from offset 8 (state RANDOM_SEED + seed + b, stream 1 -- an explicit
 * seed instead of the reference's wall clock), its length at 4 and the
 * rotate-add checksum at 0; blocks under 16 bytes are one repeated byte.
 * xec_validate_blocks writes the number of blocks failing the check to *d_bad
 * (device memory).  16-byte alignment is required when bs % 16 == 0. */
xec_status xec_write_validation_pattern(void* d_data, size_t nblocks, size_t bs, uint64_t seed,
                                        hipStream_t stream);
xec_status xec_validate_blocks(const void* d_data, size_t nblocks, size_t bs, uint32_t* d_bad,
                               hipStream_t stream);

/* Tuning overrides: xec_set_launch, xec_set_occupancy, xec_set_decode_tiling
 * and xec_set_validate_kernel are PER THREAD -- an override applies to the
 * calls the setting thread makes afterwards and to no other thread's, so a
 * sweep on one thread cannot change the kernels another thread launches
 * concurrently (a new thread starts at the defaults).  The defaults are the
 * measured best; a plugin need not call any of them.
 *
 * Launch-shape override for tuning sweeps.  Each argument 0 = the measured default:
 *   unroll        16-byte granules per lane per class member: 1 or 2;
 *   max_grid      workgroups per launch (grid-stride beyond), 0 = one per tile;
 *   cache_policy  1 = non-temporal loads/stores (nt), 2 = default policy;
 *   block_threads workgroup size, 64 (one wave) or 256. */
xec_status xec_set_launch(int unroll, int max_grid, int cache_policy, int block_threads);

/* Residency of the encode/decode kernels (per thread, like xec_set_launch):
 * at most `waves_per_simd` (1..8; 8 = no cap) waves resident per SIMD,
 * enforced by reserving LDS per workgroup (the kernels use none).
 * 0 = automatic (the default): the cap measured fastest for the member count
 * k/m at the default launch shape -- 1 at k/m = 32, 2 at 16, 4 at 4 and 8;
 * for other member counts none below 8, 4 below 20, 2 below 56, else 1;
 * none at 1 and 2.  The repair kernels take the same table;
 * xec_verify too, except 1 at k/m = 8 (its own sweep); the update kernels, the
 * write kernels and the digest kernel run uncapped at every k/m (their own sweeps); the read
 * kernel takes the table, except that an xec_read or xec_readv whose items are all present
 * runs uncapped.  The reserved LDS keeps other kernels' LDS
 * users off those CUs while a launch runs.  Returns XEC_INVALID_SIZE outside
 * 0..8. */
xec_status xec_set_occupancy(int waves_per_simd);

/* Tuning / diagnostics (no reference counterpart): how xec_decode tiles the
 * batch.  0 = automatic (default): work-list tiles -- one per (lost data
 * block, 1 KiB column chunk), from the list the host scan builds -- when at
 * most 3/4 of the stripes lost a data block and the list fits the scratch
 * (k <= 256, S <= 2^24), and for lists of up to 1,024 entries wherever
 * stripe tiles would run; otherwise class tiles -- one
 * per (stripe, class, chunk), one class reduction each, encode's tiling --
 * when the batch lost more than one data block per stripe on average and at
 * least half of its S*m classes lost one, else stripe tiles -- one per
 * (stripe, chunk), rebuilding the stripe's lost blocks one after another.
 * Batches of at most 1,024 stripes with k <= 32 that would upload the bitmap
 * or a list send one loss mask per stripe in the kernel arguments instead
 * (class or stripe tiles by the same rule, nothing copied).
 * xec_decode_device (no host scan) uses stripe tiles.  1 = always stripe
 * tiles, 2 = always class tiles, 3 = work-list tiles where the list fits (else
 * the automatic bitmap choice), 4 = kernel-argument mask tiles where they
 * apply (else automatic).  Results are identical; only the speed differs.
 * XEC_INVALID_SIZE outside 0..4. */
xec_status xec_set_decode_tiling(int tiling);

/* Tuning / diagnostics (no reference counterpart): kernel shape of
 * xec_write_validation_pattern / xec_validate_blocks.  Grouped: the checksum
 * chain of a block is split across G lanes (G = its 128-byte segments past
 * the first 128 bytes, rounded up to a power of two, at most 64; 64/G blocks
 * per wave); needs bs % 128 == 0 and bs >= 256.  Lane: one lane walks a whole
 * block.  0 = automatic (default): validation grouped wherever bs allows it;
 * the pattern grouped below 2^18 blocks, lane per block from there.
 * 1 = always lane per block, 2 = grouped wherever bs allows it.  Results are
 * identical.  XEC_INVALID_SIZE outside 0..2. */
xec_status xec_set_validate_kernel(int mode);

/* Tuning (per thread, like xec_set_launch): column rotation of the encode and
 * decode tiles.  Stripe c's 1 KiB column chunk q is processed as chunk
 * (q + c*tiles) mod (chunks per block): a permutation of each block's chunks,
 * so results are identical; it changes which columns of the stripes in flight
 * together are read at once.  0 = automatic (the measured default), -1 = none,
 * 1..2^20 = that many chunks per stripe.  XEC_INVALID_SIZE outside -1..2^20.
 * It does not apply to xec_read / xec_read_device, xec_readv / xec_readv_device,
 * xec_update / xec_update_device, xec_update_range / xec_update_range_device
 * and xec_write / xec_write_device, nor to xec_read_shards_device,
 * xec_readv_shards_device and xec_write_shards_device: their tiles walk the
 * chunks of each item's
 * byte range, not a column of every stripe.  (xec_update and xec_update_device
 * applied an explicit rotation while they had kernels of their own; the
 * automatic setting was none for them, so only a caller that set one sees the
 * order of a block's chunks change, never a byte of the result.) */
xec_status xec_set_rotation(int tiles);

/* The calling thread's overrides above as one value.  A caller that fans its
 * calls out to threads of its own (XorecBenchmarkHipMulti's shard workers)
 * reads them with xec_get_tuning and applies them in each worker with
 * xec_set_tuning, so every thread launches the shape the caller configured.
 * xec_set_tuning checks every field as the setters do and changes nothing
 * unless all are valid (XEC_INVALID_SIZE); a null pointer is
 * XEC_INVALID_ALIGNMENT. */
typedef struct {
  int unroll, max_grid, cache_policy, block_threads; /* xec_set_launch */
  int waves_per_simd;                                /* xec_set_occupancy */
  int decode_tiling;                                 /* xec_set_decode_tiling */
  int validate_kernel;                               /* xec_set_validate_kernel */
  int rotation;                                      /* xec_set_rotation */
} xec_tuning;
xec_status xec_get_tuning(xec_tuning* out);
xec_status xec_set_tuning(const xec_tuning* in);

/* Diagnostics: which tiling the calling thread's most recent xec_decode
 * launched -- 0 none (an error, or nothing to rebuild), then one of: */
enum {
  XEC_TILING_STRIPE = 1,   /* decode_kernel: (stripe, chunk) tiles over the bitmap */
  XEC_TILING_CLASS = 2,    /* decode_class_kernel: (stripe, class, chunk) tiles */
  XEC_TILING_LIST = 3,     /* decode_list_kernel: (lost block, chunk), list in d_bitmap */
  XEC_TILING_ARG_LIST = 4, /* decode_arglist_kernel: the same, list in the kernel arguments */
  XEC_TILING_ARG_MASK = 5, /* decode_argmask_kernel: class tiles, one loss mask per stripe
                              in the kernel arguments (S <= 1,024, k <= 32) */
  XEC_TILING_ARG_MASK_STRIPE = 6 /* the same masks over (stripe, chunk) tiles */
};
int xec_decode_tiling_used(void);
/* With XEC_TILING_ARG_LIST: how many entries the kernel-argument list of that
 * launch could hold -- 64, 256 or 1024, the smallest capacity that holds the
 * list, so a short list ships short kernel arguments; with XEC_TILING_ARG_MASK(_STRIPE)
 * the same for its S stripe masks; 0 for any other tiling. */
int xec_decode_arg_capacity_used(void);

/* Diagnostics / measurement: the calling thread's NEXT xec_encode, xec_decode,
 * xec_decode_per_stripe, xec_decode_device, xec_decode_device_list,
 * xec_repair, xec_repair_device, xec_verify, xec_update, xec_update_device,
 * xec_digest, xec_locate, xec_read, xec_read_device, xec_readv, xec_readv_device, xec_update_range,
 * xec_update_range_device, xec_encode_shards, xec_repair_shards_device,
 * xec_verify_shards, xec_digest_shards, xec_locate_shards,
 * xec_read_shards_device, xec_write_shards_device, xec_readv_shards_device,
 * xec_write or xec_write_device call
 * launches its encode / decode / repair / verify / update / digest / read / write kernel with hipExtLaunchKernel and these two
 * events (either may be NULL), which the runtime records from that kernel's
 * own dispatch: hipEventElapsedTime(start, stop) is the kernel's execution
 * time, with no event packet queued between kernels (a hipEventRecord between
 * two kernels is a queue packet of its own, ~6 us of gap in the kernel trace,
 * DESIGN.md §4).  Both must be events of the stream's device created with
 * timing enabled.  The call that follows consumes the setting whether or not
 * it launches a kernel (a decode with nothing to rebuild records nothing); a
 * per-stripe decode that launches in pieces times its first piece.  The
 * pipeline calls ignore and clear it. */
xec_status xec_set_kernel_events(hipEvent_t start, hipEvent_t stop);

/* ---- host-in / host-out pipeline --------------------
 * The MI355X analogue of the reference's GPU-memory / unified-memory variants
 * (src/algorithms/xorec_gpu_ptr_bm.cpp:17-65, xorec_unified_ptr_bm.cpp:15-86,
 * src/xorec/xorec.cpp:114-320), which keep the data on the host side of the
 * link.  A pipeline owns `nstreams` (1..16) device slots of `chunk_stripes`
 * stripes on the current device; a batch in host memory is streamed through
 * them chunk by chunk: H2D -> kernel -> D2H, chunks overlapping across
 * streams.  Host buffers may be pageable (file or socket buffers) or pinned
 * (hipHostMalloc / hipHostRegister); pinned ones run at the link's rate
 * (config 3: encode 55, decode 55 GB/s of data against 57 raw), pageable ones
 * at 55 / 52.  Results bound for pageable memory go through
 * pinned bounce buffers the pipeline owns, copied out by a helper thread of
 * its own; pageable inputs are staged through two pinned buffers
 * of chunk_stripes*(k+m)*bs bytes, filled one chunk ahead by a pool of host
 * threads (4; XEC_PIPELINE_COPY_THREADS at create, 0 = none: HIP stages
 * them).  The calls return when the results are in host memory.  A
 * pipeline serves one call at a time: threads that stream concurrently each
 * create their own (the library's other entry points may be called from any
 * thread).  Each call runs on the pipeline's device and leaves the caller's
 * current device as it found it.  Same argument checks and status codes as
 * xec_encode / xec_decode. */
typedef struct xec_pipeline xec_pipeline;

xec_status xec_pipeline_create(xec_pipeline** out, size_t chunk_stripes, size_t bs, size_t k,
                               size_t m, int nstreams);
xec_status xec_pipeline_destroy(xec_pipeline* p);

/* h_data: S*k*bs bytes in, h_parity: S*m*bs bytes out. */
xec_status xec_pipeline_encode(xec_pipeline* p, const void* h_data, void* h_parity, size_t S);

/* Rebuilds lost data blocks of h_data in place from h_parity (read-only);
 * only chunks that lost a data block cross the link, and only the rebuilt
 * blocks are copied back.  All-or-nothing like xec_decode. */
xec_status xec_pipeline_decode(xec_pipeline* p, void* h_data, const void* h_parity, size_t S,
                               const uint8_t* h_bitmap);

/* Human-readable status name ("Success", "InvalidSize", ...). */
const char* xec_status_string(xec_status s);

/* Build identification, e.g. "xec-hip gfx950 <date>". */
const char* xec_build_info(void);

/* ---- node topology (diagnostics; no reference counterpart) ----------------
 * The reference drives one GPU (xorec_gpu_cmp.cu:7-16).  Config 5 scatters
 * stripe ranges from a root GPU to its peers; how those bytes travel depends
 * on the pair, so the multi-GPU runs record it:
 *   can_access_peer  hipDeviceCanAccessPeer(device, peer): 1 when `device`
 *                    can map `peer`'s memory (direct peer DMA), else 0 --
 *                    a copy between them is staged by the runtime;
 *   link_type        hipExtGetLinkTypeAndHopCount: the HSA link type
 *                    (XEC_LINK_PCIE 2, XEC_LINK_XGMI 4, ...), -1 when the
 *                    runtime reports none (device == peer, or no link);
 *   hop_count        hops of that link, -1 likewise.
 * XEC_INVALID_COUNTS for a device id outside 0..count-1, XEC_DEVICE_ERROR
 * when the runtime fails; *out is written only on success. */
enum { XEC_LINK_PCIE = 2, XEC_LINK_XGMI = 4 };
typedef struct {
  int can_access_peer;
  int link_type;
  int hop_count;
} xec_peer_link_info;
xec_status xec_peer_link(int device, int peer, xec_peer_link_info* out);

#ifdef __cplusplus
}
#endif
#endif /* XEC_H */
