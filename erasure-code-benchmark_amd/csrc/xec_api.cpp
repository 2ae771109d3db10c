// xec_api.cpp -- the C ABI of libxec_hip.so (declared in include/xec.h).
//
// Host-side responsibilities, each following the reference behaviour:
//   - initialisation contract        xorec_gpu_cmp.cu:7-27, xorec.cpp:16-22
//   - argument checks                xorec_utils.hpp:61-86
//   - batch recoverability scan      xorec_gpu_cmp.cu:75-81 (require_recovery /
//                                    is_recoverable, xorec_utils.hpp:144-175)
//   - H2D bitmap / work-list upload  xorec_gpu_cmp.cu:83 (here off the caller's
//                                    stream, upload_begin below)
// then one kernel launch per call (xec_kernels.hip).
#include "xec.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "xec_internal.h"
#include "xec_kernels.h"

namespace {

std::atomic<bool> g_initialised{false};

// Tuning overrides (xec_set_launch, xec_set_occupancy, xec_set_decode_tiling);
// 0 = default.  Per thread: an override applies to the calls its own thread
// makes, so a tuning sweep on one thread never changes the kernels that
// another thread (a ShardPool worker, a pipeline user) launches meanwhile.
thread_local int g_unroll = 0;
thread_local int g_max_grid = 0;
thread_local int g_nt = 0;
thread_local int g_threads = 0;
thread_local int g_occupancy = 0;      // waves per SIMD, 0 = automatic
thread_local int g_decode_tiling = 0;  // 0 auto, 1 stripe, 2 class, 3 list, 4 mask
thread_local int g_arg_cap_used = 0;   // xec_decode_arg_capacity_used
thread_local int g_tiling_used = 0;    // xec_decode_tiling_used: this thread's last xec_decode
thread_local int g_rotation = 0;       // xec_set_rotation: 0 automatic, -1 none, > 0 tiles
thread_local int g_repair_tiling_used = 0;  // xec_repair_tiling_used: this thread's last repair
thread_local int g_update_tiling_used = 0;  // xec_update_tiling_used: this thread's last update

constexpr size_t kBlockMultiple = 256;  // XOREC_BLOCK_SIZE_MULTIPLE
constexpr size_t kMinBlock = 256;       // XOREC_MIN_BLOCK_SIZE
constexpr size_t kAlign = 64;           // XOREC_ALIGNMENT
constexpr int kMaxRotation = 1 << 20;   // xec_set_rotation's upper bound (tiles)

// LDS to reserve per workgroup so that at most `waves` waves of T-thread
// workgroups are resident per SIMD: a gfx950 CU has 160 KiB of LDS and 4
// SIMDs, so 4*waves/(T/64) workgroups fit.  Rounded down to the 512-B
// allocation granule (7 waves per SIMD comes out as 7.25); 0 = no cap.
uint32_t lds_for_occupancy(int waves, int threads) {
  if (waves <= 0 || waves >= 8) return 0;
  const uint32_t wgs = (uint32_t)(4 * waves) / (uint32_t)(threads / 64);
  uint32_t b = wgs ? (160u * 1024u) / wgs : 65536u;
  b &= ~511u;
  return b > 65536u ? 65536u : b;
}

// Resident waves per SIMD that measured fastest for the default shape (one
// wave per workgroup, one granule per lane), by class member count k/m
// (bf0ca45:tools/archive/sweep.py --occ; profiles/r01i, r01j: two devices, encode and decode,
// k=4..32).  A wave keeps up to k/m KiB of loads in flight (~11 KiB at k/m =
// 16, hipcc's rolling window; all 32 at k/m = 32); the best residency keeps
// roughly 16-32 KiB in flight per SIMD -- 8 waves per SIMD at k/m = 16 queue
// 4x the requests and ran 3 % (encode) to 6 % (decode) slower.  0 = no cap
// (8 per SIMD).  Member counts without a compiled unroll run the generic loop
// (8 loads in flight per group); swept at 3, 5, 6, 12, 24, 48 and 64
// (profiles/r02q): no cap below 8 members, 4 waves from 8 (12: +6 / +5 %
// encode / decode), 2 from 20 (24: +8 / +8 %, 48: +4 / +7 %), 1 from 56
// (64: +6 / +3 %).
int auto_occupancy(uint64_t nm) {
  switch (nm) {
    case 1: case 2: return 0;
    case 4: case 8: return 4;
    case 16: return 2;
    case 32: return 1;
    default: return nm < 8 ? 0 : nm < 20 ? 4 : nm < 56 ? 2 : 1;
  }
}

// Decode does one class reduction per lost data block of its stripe, one after
// the other, so its work per tile is k/m x (lost blocks per stripe) loads.  At
// one erasure per stripe that is the encode table above; with several
// (bf0ca45:tools/archive/sweep.py --lost, profiles/r01p: 16+2, 16+4, 16+8, 32+8, 8+2 at 2..8
// erasures per stripe) 2 waves per SIMD measured best from 8 loads per tile
// up (+3 to +15 % over the single-erasure choice), 4 from 4.  Only the member
// counts those shapes cover (2, 4, 8) take this branch.
// The policy reads the batch average, i.e. it assumes the losses are spread
// evenly over the stripes (as in every measured shape); a batch where a few
// stripes lose many blocks and most lose none is classed as single-erasure.
int decode_auto_occupancy(uint64_t nm, uint64_t lost_data, uint64_t S) {
  if (lost_data <= S || (nm != 2 && nm != 4 && nm != 8)) return auto_occupancy(nm);
  const uint64_t work = nm * ((lost_data + S - 1) / S);
  return work >= 8 ? 2 : work >= 4 ? 4 : 0;
}

// Decode tiling (xec_kernels.hip).  List tiles (the default where the list
// fits, below) give every lost data block its own tiles: one reduction each,
// none idle, whatever the spread of the losses.  Otherwise, stripe tiles run
// one class reduction per lost data block of their stripe, back to back;
// class tiles are encode's tiles, one reduction each, but a class without a
// loss leaves its tiles idle.  Measured in one process on both (bf0ca45:tools/archive/tiling_ab.py,
// profiles/r02a/tiling_ab.json; 16+2, 8+2 x 1 MiB, 16+4, 16+8, 32+8 x 64 KiB at
// 1, m/2 and m losses per stripe): class tiles win once more than one block
// per stripe AND at least half of the classes are lost (+3 to +9 % with every
// class lost, +16 % at 16+8 with 4 lost, tie at 32+8 with 4), and lose
// clearly below that (-6 % at 8+2 with one loss per stripe, 3x slower at
// 16+8 with one).  With m == 1 the tilings coincide.
bool use_class_tiles(uint64_t S, uint64_t m, uint64_t lost_data) {
  const int t = g_decode_tiling;
  if (m <= 1 || t == 1) return false;
  if (t == 2) return true;
  return lost_data > S && 2 * lost_data >= S * m;  // automatic (0, or 3 / 4 where n/a)
}

// ---- work-list staging -------------------------------------------------------
// The work list is written by the host scan into pinned host memory and copied
// into the caller's d_bitmap scratch on the stream.  A staging buffer is
// reused once the copy queued from it has run (its event); buffers are kept
// for the life of the process (a copy may still be queued when a call
// returns), at most kMaxStaging per process unless every one is in use.
struct Staging {
  void* host = nullptr;
  size_t cap = 0;
  int device = -1;
  hipEvent_t done = nullptr;     // on a library stream: the buffer's last reader has passed
  hipEvent_t handoff = nullptr;  // throw-away record on the caller's stream (record_after)
  bool busy = false;
};
constexpr size_t kMaxStaging = 64;
std::mutex g_stage_mu;
std::vector<Staging*> g_stage;

// The thread's pending HIP error and the library.  What
// the runtime does (tools/lab/last_error_probe.hip, profiles/r05b): a call
// that succeeds leaves a pending error alone; a call that fails replaces it;
// hipErrorNotReady from a stream or event query is not recorded on ROCm 7.2,
// but was read back as a launch failure under an earlier runtime
// (profiles/r04s).  So the library (1) asks no query at all while an error of
// the caller's is pending -- it takes the answer that needs none, which is
// always correct -- (2) clears a NotReady only if that is what the query left
// pending, and (3) reports any other query error as the call's failure,
// leaving it pending for the caller.
bool caller_error_pending() { return hipPeekAtLastError() != hipSuccess; }

void clear_own_not_ready() {
  if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
}

// hipEventQuery on a buffer's event (recorded on a stream the library owns,
// track_stream below): 1 once the work it marks has passed, 0 not yet, -1 the
// query failed -- a sticky device fault, which fails the call.  The query is
// asked even while an error of the caller's is pending: taking
// every buffer as in use then made each call allocate a new one up to the
// pool's cap and then wait on a recycled one.  On this runtime a successful
// query leaves the pending error alone and a NotReady is not recorded
// (profiles/r05b), so only the clearing step is skipped: the pending error is
// the caller's, never ours to clear.
int event_passed(hipEvent_t e) {
  const bool callers = caller_error_pending();
  const hipError_t q = hipEventQuery(e);
  if (q == hipSuccess) return 1;
  if (q == hipErrorNotReady) {
    if (!callers) clear_own_not_ready();
    return 0;
  }
  return -1;
}

// A buffer read by the caller's stream is free once that stream has passed
// the reading work -- but an event recorded on the CALLER's stream may outlive
// that stream (a pipeline destroys its streams), and querying it later made
// HIP report a stray error (hipErrorStreamCaptureUnsupported, read by the
// next launch's hipGetLastError: tools/fuzz_big.py --pipeline, profiles/r04s).
// So the caller's stream only hands over to a tracking stream of the
// library's (hipStreamWaitEvent on a throw-away record), and the buffer's
// event is recorded there.  A tracking stream waits for its callers in the
// order the hand-offs were queued, so one shared stream would keep a short
// decode's buffer busy behind every earlier caller's unrelated long work
// (ADVICE r04): each device has kTrackLanes of them, a caller stream always
// hands over to the same lane (its handle hashed), so independent callers on
// different streams rarely share one (g_track_mu guards the list).
constexpr size_t kTrackLanes = 4;
std::mutex g_track_mu;
struct TrackLanes {
  int dev;
  hipStream_t lane[kTrackLanes];
};
std::vector<TrackLanes> g_track_streams;
hipStream_t track_stream(int dev, hipStream_t caller) {
  const uintptr_t h = reinterpret_cast<uintptr_t>(caller);
  const size_t lane = static_cast<size_t>((h >> 4) ^ (h >> 12)) % kTrackLanes;
  std::lock_guard<std::mutex> lk(g_track_mu);
  for (auto& ts : g_track_streams)
    if (ts.dev == dev) return ts.lane[lane];
  TrackLanes t{dev, {}};
  for (auto& s : t.lane)
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      for (auto& made : t.lane)
        if (made != nullptr) (void)hipStreamDestroy(made);
      return nullptr;
    }
  g_track_streams.push_back(t);
  return t.lane[lane];
}

// Record `done` once `caller` has passed its current work, on a tracking
// stream of `dev` (`handoff` is the throw-away record on the caller's
// stream); false if that cannot be queued.
bool record_after(hipEvent_t done, hipEvent_t handoff, hipStream_t caller, int dev) {
  const hipStream_t ts = track_stream(dev, caller);
  return ts != nullptr && hipEventRecord(handoff, caller) == hipSuccess &&
         hipStreamWaitEvent(ts, handoff, 0) == hipSuccess && hipEventRecord(done, ts) == hipSuccess;
}

// The slot is picked and marked busy under the lock; waiting for a recycled
// buffer's last reader and re-allocating happen after the lock is dropped, so
// one thread waiting for another's copy never stalls other threads' calls.
// *fault: an event query failed (event_passed -1); nullptr is returned and
// the call must fail.
Staging* stage_acquire(size_t bytes, int dev, bool* fault) {
  Staging* pick = nullptr;
  bool recycled = false;
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    for (Staging* st : g_stage) {
      if (st->busy || st->device != dev || st->cap < bytes) continue;
      const int passed = event_passed(st->done);
      if (passed < 0) {
        *fault = true;
        return nullptr;
      }
      if (passed == 0) continue;  // a queued copy still reads it
      if (pick == nullptr || st->cap < pick->cap) pick = st;
    }
    if (pick == nullptr && g_stage.size() >= kMaxStaging) {
      for (Staging* st : g_stage)  // recycle an idle one of this device: wait for its copy
        if (!st->busy && st->device == dev) {
          pick = st;
          recycled = true;
          break;
        }
    }
    if (pick == nullptr) {
      pick = new Staging;
      pick->device = dev;
      if (hipEventCreateWithFlags(&pick->done, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&pick->handoff, hipEventDisableTiming) != hipSuccess) {
        if (pick->done) (void)hipEventDestroy(pick->done);
        delete pick;
        return nullptr;
      }
      g_stage.push_back(pick);
    }
    pick->busy = true;
  }
  auto give_back = [&]() {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    pick->busy = false;
    return nullptr;
  };
  if (recycled && hipEventSynchronize(pick->done) != hipSuccess) {
    *fault = true;  // a sticky fault: left pending for the caller
    return give_back();
  }
  if (pick->cap < bytes) {
    if (pick->host != nullptr) (void)hipHostFree(pick->host);
    pick->host = nullptr;
    pick->cap = 0;
    size_t cap = 64u << 10;
    while (cap < bytes) cap <<= 1;
    if (hipHostMalloc(&pick->host, cap, hipHostMallocDefault) != hipSuccess) {
      pick->host = nullptr;
      return give_back();
    }
    pick->cap = cap;
  }
  return pick;
}

// `stream` = where a copy from the buffer was queued (nullptr-able), or
// `queued` = false when nothing was; `own`: the stream is the library's (its
// copy stream), else the caller's (record_after).  If the event cannot be
// recorded, the copy is waited for instead, so the buffer is never reused early.
void stage_release(Staging* st, bool queued, hipStream_t stream, bool own) {
  if (queued && !(own ? hipEventRecord(st->done, stream) == hipSuccess
                      : record_after(st->done, st->handoff, stream, st->device)))
    (void)hipStreamSynchronize(stream);
  std::lock_guard<std::mutex> lk(g_stage_mu);
  st->busy = false;
}

// ---- uploads off the caller's stream ---------------------------------------
// What a decode kernel reads besides the batch -- the bitmap or the work list
// -- comes from host memory.  Copied on the caller's stream, the copy waits
// for the kernel before it and the decode kernel for the copy (the copy
// engine's start and completion hand-offs included): 17-73 us per decode in
// tools/lab/mix_ceiling.py (profiles/r03f: event time minus kernel time at
// 16+8, 32+8, 32+1 x 4 KiB), 2-8 % of those decodes.  So the bytes go to a
// device buffer the library owns, on a copy stream of its own (one per
// device, non-blocking), which starts at once -- while the caller's stream is
// still busy with earlier work -- and the decode kernel only waits for the
// copy's event.  A buffer is reused once the kernel that read it has passed
// (its event on the caller's stream); buffers are kept for the life of the
// process, at most kMaxSlots per device unless every one is in use.  The
// caller's d_bitmap scratch is used instead when no buffer can be had.
struct DevSlot {
  void* dev = nullptr;
  size_t cap = 0;
  int device = -1;
  hipEvent_t copied = nullptr;  // on the copy stream, after the upload
  hipEvent_t done = nullptr;    // on a library stream, after the reading kernel (record_after)
  hipEvent_t handoff = nullptr;  // throw-away record on the caller's stream
  bool busy = false;
};
constexpr size_t kMaxSlots = 16;
std::mutex g_slot_mu;
std::vector<DevSlot*> g_slots;
std::vector<std::pair<int, hipStream_t>> g_copy_streams;

hipStream_t copy_stream(int dev) {  // under g_slot_mu
  for (auto& cs : g_copy_streams)
    if (cs.first == dev) return cs.second;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  g_copy_streams.emplace_back(dev, s);
  return s;
}

struct Upload {
  DevSlot* slot = nullptr;  // null: the bytes went to the caller's scratch on `stream`
  hipStream_t cs = nullptr;  // the copy stream they went on
  uint8_t* dev = nullptr;   // where the kernel reads them
};

// XEC_SCRATCH_UPLOADS=1 in the environment sends every upload through the
// caller's scratch on the stream (the fallback path; tests use it).
bool side_uploads() {
  static const bool off = [] {
    const char* e = std::getenv("XEC_SCRATCH_UPLOADS");
    return e != nullptr && e[0] == '1';
  }();
  return !off;
}

// Uploads go off the caller's stream only while that stream is busy: then a
// copy queued on it would wait for the kernel before it (the bubble above).
// On an idle stream -- a synchronous caller such as the reference's
// BM_generic loop, which synchronises after every call -- the copy on the
// stream starts at once, and the side path's cross-stream event would only
// add latency: 8 MiB (40/32) with 8 lost ran at 2,284 instead of 3,669
// Gbit/s per call, 128 MiB with 2-8 lost 21-27 % slower (tools/ab/
// refrows_ab.sh, profiles/r03zk).  A NotReady answer is cleared so that no
// later hipGetLastError reads it as a launch failure; any other answer (a
// sticky fault of earlier work, an invalid stream) is an error the caller
// gets back as XEC_DEVICE_ERROR, and is left for its hipGetLastError.  While
// an error of the caller's is pending nothing is asked: the stream is taken as
// idle (the copy goes on it, correct either way) and the error stays theirs.
// Returns 0 idle, 1 busy, -1 error.
int stream_busy(hipStream_t stream) {
  if (caller_error_pending()) return 0;
  const hipError_t q = hipStreamQuery(stream);
  if (q == hipSuccess) return 0;
  if (q != hipErrorNotReady) {
    if (const char* e = std::getenv("XEC_DEBUG"); e != nullptr && e[0] == '1')
      std::fprintf(stderr, "xec: hipStreamQuery: %s\n", hipGetErrorName(q));
    return -1;
  }
  clear_own_not_ready();
  return 1;
}

// The device `stream` belongs to (the current device for the null stream).
// HIP accepts a stream of device B while device A is current, and the decode
// kernel then runs on B: the library buffers, copy stream and staging the
// call uses must be B's too.  So a decode makes the stream's device current
// for its duration and restores the caller's on return.
class StreamDevice {
 public:
  explicit StreamDevice(hipStream_t stream) {
    ok_ = hipGetDevice(&prev_) == hipSuccess;
    dev_ = prev_;
    if (ok_ && stream != nullptr) {
      ok_ = hipStreamGetDevice(stream, &dev_) == hipSuccess;
      if (ok_ && dev_ != prev_) ok_ = switched_ = hipSetDevice(dev_) == hipSuccess;
    }
  }
  ~StreamDevice() {
    if (switched_) (void)hipSetDevice(prev_);
  }
  StreamDevice(const StreamDevice&) = delete;
  StreamDevice& operator=(const StreamDevice&) = delete;
  bool ok() const { return ok_; }
  int device() const { return dev_; }

 private:
  int prev_ = 0, dev_ = 0;
  bool ok_ = false, switched_ = false;
};

bool capturing(hipStream_t stream) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
}

// Starts copying `bytes` of host memory to a library buffer on the device's
// copy stream; false (nothing queued) if no buffer or stream can be had, and
// then *fault if an event query or wait failed (the call must fail).
// `dev` is the current device (StreamDevice).  As in stage_acquire, a slot is
// picked and marked busy under the lock, and a recycled slot's wait and
// re-allocation happen outside it.
bool upload_begin(const void* host, size_t bytes, int dev, Upload& up, bool* fault) {
  DevSlot* pick = nullptr;
  hipStream_t cs = nullptr;
  bool recycled = false;
  {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    cs = copy_stream(dev);
    if (cs == nullptr) return false;
    for (DevSlot* sl : g_slots) {
      if (sl->busy || sl->device != dev || sl->cap < bytes) continue;
      const int passed = event_passed(sl->done);
      if (passed < 0) {
        *fault = true;
        return false;
      }
      if (passed == 0) continue;  // a kernel still reads it
      if (pick == nullptr || sl->cap < pick->cap) pick = sl;
    }
    size_t mine = 0;
    for (DevSlot* sl : g_slots) mine += sl->device == dev;
    if (pick == nullptr && mine >= kMaxSlots) {
      for (DevSlot* sl : g_slots)  // recycle an idle one: wait for its reader (below)
        if (!sl->busy && sl->device == dev) {
          pick = sl;
          recycled = true;
          break;
        }
      if (pick == nullptr) return false;
    }
    if (pick == nullptr) {
      pick = new DevSlot;
      pick->device = dev;
      if (hipEventCreateWithFlags(&pick->copied, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&pick->done, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&pick->handoff, hipEventDisableTiming) != hipSuccess) {
        if (pick->copied) (void)hipEventDestroy(pick->copied);
        if (pick->done) (void)hipEventDestroy(pick->done);
        delete pick;
        return false;
      }
      g_slots.push_back(pick);
    }
    pick->busy = true;
  }
  auto give_back = [&]() {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    pick->busy = false;
    return false;
  };
  if (recycled && hipEventSynchronize(pick->done) != hipSuccess) {
    *fault = true;  // a sticky fault: left pending for the caller
    return give_back();
  }
  if (pick->cap < bytes) {
    if (pick->dev != nullptr) (void)hipFree(pick->dev);
    pick->dev = nullptr;
    pick->cap = 0;
    size_t cap = 64u << 10;
    while (cap < bytes) cap <<= 1;
    if (hipMalloc(&pick->dev, cap) != hipSuccess) {
      pick->dev = nullptr;
      return give_back();
    }
    pick->cap = cap;
  }
  if (hipMemcpyAsync(pick->dev, host, bytes, hipMemcpyHostToDevice, cs) != hipSuccess ||
      hipEventRecord(pick->copied, cs) != hipSuccess) {
    (void)hipStreamSynchronize(cs);
    std::lock_guard<std::mutex> lk(g_slot_mu);
    pick->busy = false;
    return false;
  }
  up.slot = pick;
  up.cs = cs;
  up.dev = static_cast<uint8_t*>(pick->dev);
  return true;
}

// The caller's stream waits for the upload (before the kernel that reads it).
bool upload_join(const Upload& up, hipStream_t stream) {
  return up.slot == nullptr || hipStreamWaitEvent(stream, up.slot->copied, 0) == hipSuccess;
}

// After the launch (`launched`: a kernel on `stream` reads the buffer) or
// without one: the buffer is free once that kernel, or the copy, has passed.
void upload_end(Upload& up, hipStream_t stream, bool launched) {
  if (up.slot == nullptr) return;
  hipStream_t after = launched ? stream : up.cs;
  const bool ok = launched ? record_after(up.slot->done, up.slot->handoff, stream, up.slot->device)
                           : hipEventRecord(up.slot->done, up.cs) == hipSuccess;
  if (!ok) (void)hipStreamSynchronize(after);
  std::lock_guard<std::mutex> lk(g_slot_mu);
  up.slot->busy = false;
  up.slot = nullptr;
}

// Defaults measured on MI355X (bf0ca45:tools/archive/sweep.py, profiles/r01_sweep_*.json):
// non-temporal loads and parity stores, sc1 rebuilt-block stores (every byte
// is touched once; xec_kernels.hip kEncodeStoreAux / kDecodeStoreAux), one-wave
// workgroups with one 1 KiB tile each, one workgroup per tile, residency
// capped per member count (auto_occupancy).
// Column rotation of the tile kernels (Geometry::rot): the chunks a stripe's
// column walk is shifted by, per stripe (xec_set_rotation).  Automatic: none
// for encode and for decodes the host scan cannot see; decode_rotation below.
uint32_t rotation() {
  const int r = g_rotation;
  return r > 0 ? (uint32_t)r : 0u;
}

// Automatic decode rotation.  When every lost data block of the batch sits in
// one parity class -- one failed device: the same shard gone from every
// stripe -- with m >= 2, the stripes in flight read the same columns of k/m
// blocks m*bs apart, which this HBM serves slowly; an odd rotation puts them
// on different columns.  Measured in one process against no rotation
// (tools/lab/loss_pattern_probe.py --rotations, profiles/r04d): one failed
// device +15.7 % at 16+2 x 1 MiB, +15.4 % at 8+2, +11.5 % at 16+4, +5.8 % at
// 32+4, +5.4 % at 16+2 x 512 KiB, +3.8 % at 16+2 x 4 MiB, but -4.0 % at
// 16+2 x 256 KiB -- hence the 512 KiB floor.  Where the class alternates
// between stripes (the bench's pattern) or several classes lost blocks, a
// rotation lost up to 11 %, and encode lost 2-15 % (profiles/r04c), so neither
// rotates.
// The lost_class of a work list (xec_decode_per_stripe lists the rebuilt
// blocks only; its scan has no class summary of its own).
XecScan items_scan(const uint32_t* items, uint64_t n, size_t m) {
  XecScan v;
  v.lost_data = n;
  for (uint64_t q = 0; q < n; ++q) {
    const int64_t c = static_cast<int64_t>((items[q] & 0xFFu) % m);
    if (q == 0) v.lost_class = c;
    else if (v.lost_class != c) {
      v.lost_class = -1;
      break;
    }
  }
  return v;
}

constexpr uint32_t kSameClassRotation = 3;
constexpr size_t kRotateMinBlock = 512u << 10;
uint32_t decode_rotation(const XecScan& scan, size_t m, size_t bs) {
  const int r = g_rotation;
  if (r != 0) return r > 0 ? (uint32_t)r : 0u;
  return m >= 2 && scan.lost_class >= 0 && bs >= kRotateMinBlock ? kSameClassRotation : 0u;
}

xec::LaunchShape launch_shape(size_t bs, int auto_w) {
  xec::LaunchShape ls;
  ls.rot = rotation();
  const int t = g_threads;
  ls.threads = t == 256 ? 256 : 64;
  const int u = g_unroll;
  ls.unroll = (u == 1 || u == 2) ? u : 1;
  const int g = g_max_grid;
  ls.max_grid = g > 0 ? (uint32_t)g : 0u;
  // nt stores address the block with a 32-bit buffer offset (xec_kernels.hip)
  ls.nt = g_nt != 2 && bs <= 0x7fffffffu;
  int w = g_occupancy;
  if (w == 0) w = (ls.threads == 64 && ls.unroll == 1) ? auto_w : 0;
  ls.lds_bytes = lds_for_occupancy(w, ls.threads);
  return ls;
}

// Workgroups the chip holds at once for a launch of shape ls (CUs x the
// workgroups per CU its LDS reservation admits, at most 32 waves per CU):
// the fixed grid of decode_devlist_kernel, which walks a count the host never
// sees.  0 if the device cannot be queried.
constexpr uint64_t kDevListMaxGrid = 131072;  // xec_decode_device_list's largest default grid

uint32_t resident_workgroups(const xec::LaunchShape& ls) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus <= 0)
    return 0;
  const uint32_t waves = (uint32_t)ls.threads / 64u;
  uint32_t per_cu = 32u / (waves ? waves : 1u);
  if (ls.lds_bytes > 0 && (160u * 1024u) / ls.lds_bytes < per_cu)
    per_cu = (160u * 1024u) / ls.lds_bytes;
  return (uint32_t)cus * (per_cu ? per_cu : 1u);
}

// xec_set_kernel_events arms the next codec call of this thread; that call
// consumes the setting whether or not it launched a kernel (include/xec.h).
struct KernelEventsScope {
  ~KernelEventsScope() { xec::t_kernel_events = xec::KernelEvents{}; }
};

// The body of a codec entry point whose host-side bookkeeping allocates (upload
// buffers, pinned staging, their lists).  No exception crosses the C ABI: an
// allocation failure there is a device error for the caller, not a
// std::terminate.
template <class Body>
xec_status guarded(Body&& body) {
  const KernelEventsScope events_scope;
  try {
    return body();
  } catch (...) {
    return XEC_DEVICE_ERROR;
  }
}

// XEC_DEBUG=1: a call that fails with XEC_DEVICE_ERROR names its line, the
// HIP error of the failing call and the one pending on the thread (stderr;
// diagnostics only).
bool debug_on() {
  static const bool on = [] {
    const char* e = std::getenv("XEC_DEBUG");
    return e != nullptr && e[0] == '1';
  }();
  return on;
}
xec_status dev_error(int line, hipError_t e) {
  if (debug_on())
    std::fprintf(stderr, "xec: device error at xec_api.cpp:%d (%s; pending %s)\n", line,
                 hipGetErrorName(e), hipGetErrorName(hipPeekAtLastError()));
  return XEC_DEVICE_ERROR;
}
#define DEVERR(e) dev_error(__LINE__, (e))
// What a launch returned, as the ABI's status; `line` is the entry point's own.
xec_status launch_status(int line, hipError_t le) {
  return le == hipSuccess ? XEC_SUCCESS : dev_error(line, le);
}

// The device scratch a list too long for the kernel arguments goes through.
xec_status check_scratch(const void* d_scratch, size_t scratch_bytes, size_t need) {
  if (reinterpret_cast<uintptr_t>(d_scratch) % 4 != 0) return XEC_INVALID_ALIGNMENT;
  if (d_scratch == nullptr || scratch_bytes < need) return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

// Items c << 8 | i of data blocks: each in range, and strictly ascending =
// batch order, no duplicates.
bool items_ascending(const uint32_t* h_items, size_t n, size_t S, size_t k) {
  for (size_t t = 0; t < n; ++t) {
    const uint32_t it = h_items[t];
    if ((it & 0xFFu) >= k || (it >> 8) >= S || (t > 0 && it <= h_items[t - 1])) return false;
  }
  return true;
}

// A list too long for the kernel arguments: fill(words) writes its `bytes` into
// pinned staging, one copy on `stream` itself takes them to d_scratch, and
// launch() queues the kernel that reads them there.  `line`: see launch_status.
template <class Fill, class Launch>
xec_status upload_list_and_launch(size_t bytes, void* d_scratch, hipStream_t stream, int line,
                                  Fill&& fill, Launch&& launch) {
  const StreamDevice sd(stream);  // the stream's device, as in xec_decode
  if (!sd.ok()) return dev_error(line, hipSuccess);
  bool fault = false;
  Staging* sg = stage_acquire(bytes, sd.device(), &fault);
  if (sg == nullptr) return dev_error(line, hipSuccess);
  fill(static_cast<uint32_t*>(sg->host));
  hipError_t le = hipMemcpyAsync(d_scratch, sg->host, bytes, hipMemcpyHostToDevice, stream);
  const bool queued = le == hipSuccess;
  if (queued) le = launch();
  stage_release(sg, queued, stream, false);
  return launch_status(line, le);
}

}  // namespace

extern "C" {

xec_status xec_check_args(const void* data, const void* parity, size_t bs, size_t k, size_t m) {
  if (reinterpret_cast<uintptr_t>(data) % kAlign != 0 ||
      reinterpret_cast<uintptr_t>(parity) % kAlign != 0)
    return XEC_INVALID_ALIGNMENT;
  if (bs < kMinBlock || bs % kBlockMultiple != 0) return XEC_INVALID_SIZE;
  if (k < 1 || m < 1 || k % m != 0) return XEC_INVALID_COUNTS;
  return XEC_SUCCESS;
}

// What every entry point that takes a batch checks first, in this order.
static xec_status check_entry(const void* data, const void* parity, size_t bs, size_t k,
                              size_t m) {
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  return xec_check_args(data, parity, bs, k, m);
}

// xec_check_bitmap / xec_scan_bitmap live in xec_scan.cpp (host-only, AVX2 where available).

xec_status xec_init(int device_id) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return XEC_DEVICE_ERROR;
  if (device_id < 0 || device_id >= count) return XEC_DEVICE_ERROR;
  if (hipSetDevice(device_id) != hipSuccess) return XEC_DEVICE_ERROR;
  // code objects onto the device now rather than at the first codec call
  if (xec::preload_kernels() != hipSuccess || xec::preload_validate() != hipSuccess)
    return XEC_DEVICE_ERROR;
  g_initialised.store(true, std::memory_order_release);
  return XEC_SUCCESS;
}

xec_status xec_set_kernel_events(hipEvent_t start, hipEvent_t stop) {
  xec::t_kernel_events = xec::KernelEvents{start, stop};
  return XEC_SUCCESS;
}

xec_status xec_encode(const void* d_data, void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                      hipStream_t stream) {
  const KernelEventsScope events_scope;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  return xec::launch_encode(d_data, d_parity, g, ls, stream) == hipSuccess ? XEC_SUCCESS
                                                                           : XEC_DEVICE_ERROR;
}

// Bitmaps from this size on are copied to the device BEFORE the host scan, so
// the scan (~1.1 ns per stripe, 75 us for config 4's 65,536 stripes) runs
// while the transfer does and the synchronous caller waits for
// max(scan, copy) + kernel instead of their sum (bf0ca45:tools/archive/scan_cost.py,
// profiles/r02b, r02c).  Smaller bitmaps keep the scan first, so a batch that
// needs no recovery queues no device work at all.
constexpr size_t kCopyFirstBitmapBytes = 256u << 10;

// Work-list tiles are taken (automatic tiling) when at most this fraction of
// the stripes lost a data block: then stripe and class tiles would leave most
// of their tiles idle (sparse: 2.2x faster at 1 stripe in 9, skewed: 1.0-3.1x
// at 1 in 5; bf0ca45:tools/archive/tiling_ab.py --pattern, profiles/r02n).  When every stripe
// lost blocks, the bitmap tilings are as fast or faster (list tiles -1..-5 %
// against the better of them, profiles/r02n/tiling_uniform.json, r02o).
constexpr uint64_t kListStripesNum = 3, kListStripesDen = 4;

static xec_status decode_impl(void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                              size_t m, const uint8_t* h_bitmap, uint8_t* d_bitmap,
                              hipStream_t stream) {
  g_tiling_used = 0;
  g_arg_cap_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  const size_t bitmap_bytes = S * (k + m);
  // The host scan reads h_bitmap now: a graph captured from this call would
  // replay this call's losses whatever the bitmap holds then.  So a call with
  // work to queue is refused on a capturing stream, before anything is
  // queued; xec_decode_device is the capturable form.  A batch that needs no
  // recovery, or cannot be recovered, returns its verdict from the scan
  // alone, before any device call -- the reference's order
  // (xorec_gpu_cmp.cu:75-81) -- so it never pays the capture query.
  const bool cap = bitmap_bytes >= kCopyFirstBitmapBytes && capturing(stream);
  const bool copy_first = bitmap_bytes >= kCopyFirstBitmapBytes && !cap;
  // Small bitmaps are scanned first: a batch that needs no recovery (or
  // cannot be recovered) returns before any device query or copy.  That pass
  // also lists the lost data blocks, speculatively, so a decode whose list
  // travels in the kernel arguments -- the small messages, e.g. the
  // reference's 8 MiB rows -- scans its bitmap once, not twice (VERDICT r05
  // item 3: the second pass was ~0.6-0.8 us of an 8 MiB decode call).  The
  // scan stops listing once its projection says the list will not be used
  // (more than kArgItems losses, or a class-tile batch): listing 1,024 items
  // for nothing cost 1.3 us (profiles/r06i).
  XecScan scan;
  uint32_t items[xec::kArgItems];
  bool listed = false;  // items holds every lost data block
  if (!copy_first) {
    st = xec_scan_bitmap(h_bitmap, S, k, m, &scan, items, xec::kArgItems, /*speculative=*/true);
    listed = scan.listed == scan.lost_data;
    if (st != XEC_SUCCESS || !scan.needs_recovery || scan.lost_data == 0) return st;
    if (cap || capturing(stream)) return DEVERR(hipSuccess);
  }
  const StreamDevice sd(stream);
  if (!sd.ok()) return DEVERR(hipSuccess);
  const int dev = sd.device();
  // Whether uploads go off the stream, asked (hipStreamQuery) only when
  // something is about to be uploaded: a list that travels in the kernel
  // arguments never pays for the query.  A query that fails (not merely
  // "busy") fails the call.
  int side_state = -2;
  bool query_failed = false;
  auto side = [&]() {
    if (side_state == -2) {
      side_state = side_uploads() ? stream_busy(stream) : 0;
      query_failed = side_state < 0;
    }
    return side_state == 1;
  };
  // The bitmap goes to the device (a library buffer, or the caller's scratch
  // on `stream`); for large bitmaps before the scan, so the two overlap.
  Upload bmu;
  auto upload_bitmap = [&]() -> bool {
    if (side() && upload_begin(h_bitmap, bitmap_bytes, dev, bmu, &query_failed)) return true;
    if (query_failed) return false;
    bmu = Upload{};
    bmu.dev = d_bitmap;
    return hipMemcpyAsync(d_bitmap, h_bitmap, bitmap_bytes, hipMemcpyHostToDevice, stream) ==
           hipSuccess;
  };
  if (copy_first) {
    if (!upload_bitmap()) return DEVERR(hipSuccess);
    st = xec_scan_bitmap(h_bitmap, S, k, m, &scan, nullptr, 0);
    if (st != XEC_SUCCESS || !scan.needs_recovery || scan.lost_data == 0) {
      upload_end(bmu, stream, false);  // only the bitmap copy was queued
      return st;                       // failure, or nothing to rebuild
    }
  }
  // Which tiling: list tiles when the losses are sparse (or forced); for a
  // list short enough to travel in the kernel arguments also wherever stripe
  // tiles would run (no copy at all); class tiles keep dense multi-erasure
  // batches.  The list is built by a second, listing pass only
  // when it is used (the first pass costs ~1.1 ns per stripe).
  const int tiling = g_decode_tiling;
  const bool listable = (tiling == 0 || tiling == 3 || tiling == 4) && k <= kWorkItemMaxK &&
                        S <= kWorkItemMaxStripes;
  const bool small = scan.lost_data <= xec::kArgItems;
  const bool sparse = scan.stripes_lost * kListStripesDen <= (uint64_t)S * kListStripesNum;
  const bool cls = use_class_tiles(S, m, scan.lost_data);
  // A batch of at most kArgItems stripes (k <= 32) whose decode would upload
  // something -- a list longer than the kernel arguments hold, or the bitmap
  // for class / stripe tiles -- sends one loss mask per stripe in the kernel
  // arguments instead, over class tiles where the bitmap path would take them
  // and stripe tiles otherwise: nothing is copied, so a synchronous caller
  // does not wait for a copy ahead of the kernel (decode_argmask_kernel; the
  // reference's row 1126, 8 MiB (40/32) with 8 losses, profiles/r06w).  Forced
  // with xec_set_decode_tiling(4).
  const bool arglist = listable && small && (tiling == 3 || sparse || !cls);
  const bool maskable = !copy_first && S <= xec::kArgItems && k <= xec::kArgMaskMaxK;
  if (maskable && (tiling == 4 || (tiling == 0 && !arglist))) {
    uint32_t masks[xec::kArgItems];
    xec_loss_masks(h_bitmap, S, k, m, masks);
    // class tiles: one reduction per tile, encode's residency table; stripe
    // tiles: as the bitmap's stripe tiles
    xec::LaunchShape ls = launch_shape(
        bs, cls ? auto_occupancy(k / m) : decode_auto_occupancy(k / m, scan.lost_data, S));
    ls.rot = decode_rotation(scan, m, bs);
    const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
    g_tiling_used = cls ? XEC_TILING_ARG_MASK : XEC_TILING_ARG_MASK_STRIPE;
    g_arg_cap_used = (int)xec::arg_items_capacity(S);
    const hipError_t le = xec::launch_decode(
        d_data, d_parity, nullptr, g, ls,
        cls ? xec::kDecodeArgMaskTiles : xec::kDecodeArgMaskStripeTiles, stream, S, masks);
    return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
  }
  if (listable && (tiling == 3 || sparse || (!cls && small))) {
    // one reduction per tile, as encode: encode's residency table
    xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
    ls.rot = decode_rotation(scan, m, bs);
    const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
    if (small) {  // the launch copies the list into its kernel arguments
      upload_end(bmu, stream, false);
      if (!listed) {
        st = xec_scan_bitmap(h_bitmap, S, k, m, &scan, items, xec::kArgItems);
        if (st != XEC_SUCCESS) return st;
      }
      g_tiling_used = XEC_TILING_ARG_LIST;
      g_arg_cap_used = (int)xec::arg_items_capacity(scan.lost_data);
      const hipError_t le = xec::launch_decode(d_data, d_parity, nullptr, g, ls,
                                               xec::kDecodeArgListTiles, stream, scan.lost_data,
                                               items);
      return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
    }
    // u32 entries staged in pinned host memory by the listing pass, then
    // uploaded: to a library buffer off the stream, or into the 4-byte-aligned
    // part of the caller's S*(k+m)-byte scratch on it (if the list fits)
    const size_t pad = (4 - reinterpret_cast<uintptr_t>(d_bitmap) % 4) % 4;
    const uint64_t cap = bitmap_bytes > pad ? (bitmap_bytes - pad) / 4 : 0;
    const uint64_t n = scan.lost_data;
    Staging* sg = nullptr;
    const bool off_stream = side();
    if (query_failed) {
      upload_end(bmu, stream, false);
      return DEVERR(hipSuccess);
    }
    if (off_stream || n <= cap) sg = stage_acquire(n * 4, dev, &query_failed);
    if (query_failed) {
      upload_end(bmu, stream, false);
      return DEVERR(hipSuccess);
    }
    if (sg != nullptr) {
      st = xec_scan_bitmap(h_bitmap, S, k, m, &scan, static_cast<uint32_t*>(sg->host), n);
      if (st != XEC_SUCCESS) {
        stage_release(sg, false, stream, false);
        upload_end(bmu, stream, false);
        return st;
      }
      Upload lu;
      bool ok = true;
      if (side() && upload_begin(sg->host, n * 4, dev, lu, &query_failed)) {
        stage_release(sg, true, lu.cs, true);
        ok = upload_join(lu, stream);
      } else if (query_failed) {
        stage_release(sg, false, stream, false);
        upload_end(bmu, stream, false);
        return DEVERR(hipSuccess);
      } else if (n <= cap) {
        // stream-ordered after any bitmap copy into the same scratch
        lu.dev = d_bitmap + pad;
        ok = hipMemcpyAsync(lu.dev, sg->host, n * 4, hipMemcpyHostToDevice, stream) == hipSuccess;
        stage_release(sg, ok, stream, false);
      } else {
        stage_release(sg, false, stream, false);  // denser than the scratch holds: bitmap tiles
      }
      if (lu.dev != nullptr) {
        upload_end(bmu, stream, false);
        g_tiling_used = XEC_TILING_LIST;
        const hipError_t le =
            ok ? xec::launch_decode(d_data, d_parity, lu.dev, g, ls, xec::kDecodeListTiles,
                                    stream, n)
               : hipErrorUnknown;
        upload_end(lu, stream, true);
        return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
      }
    }
    // no staging memory, or a list denser than the scratch holds: bitmap tiles
  }
  if (!copy_first && !upload_bitmap()) return DEVERR(hipSuccess);
  if (!upload_join(bmu, stream)) {
    upload_end(bmu, stream, false);
    return DEVERR(hipSuccess);
  }
  // class tiles: one reduction per tile, so the encode's residency table
  xec::LaunchShape ls = launch_shape(
      bs, cls ? auto_occupancy(k / m) : decode_auto_occupancy(k / m, scan.lost_data, S));
  ls.rot = decode_rotation(scan, m, bs);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  g_tiling_used = cls && m > 1 ? XEC_TILING_CLASS : XEC_TILING_STRIPE;
  const hipError_t le = xec::launch_decode(d_data, d_parity, bmu.dev, g, ls,
                                           cls ? xec::kDecodeClassTiles : xec::kDecodeStripeTiles,
                                           stream);
  upload_end(bmu, stream, true);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

xec_status xec_decode(void* d_data, const void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                      const uint8_t* h_bitmap, uint8_t* d_bitmap, hipStream_t stream) {
  return guarded(
      [&] { return decode_impl(d_data, d_parity, S, bs, k, m, h_bitmap, d_bitmap, stream); });
}

int xec_decode_tiling_used(void) { return g_tiling_used; }
int xec_decode_arg_capacity_used(void) { return g_arg_cap_used; }

static xec_status decode_per_stripe_impl(void* d_data, const void* d_parity, size_t S, size_t bs,
                                         size_t k, size_t m, const uint8_t* h_bitmap,
                                         uint8_t* d_bitmap, uint8_t* h_codes, hipStream_t stream) {
  g_tiling_used = 0;
  g_arg_cap_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  if (k > kWorkItemMaxK || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  uint64_t n = 0, failures = 0;
  // one pass gives the verdicts and, for a short list, the list itself
  uint32_t short_items[xec::kArgItems];
  st = xec_scan_stripes(h_bitmap, S, k, m, h_codes, short_items, xec::kArgItems, &n, &failures);
  if (st != XEC_SUCCESS) return st;
  const xec_status verdict = failures ? XEC_DECODE_FAILURE : XEC_SUCCESS;
  if (n == 0) return verdict;
  if (capturing(stream)) return XEC_DEVICE_ERROR;  // work to queue: see xec_decode
  xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  // the rebuilt blocks' classes decide the column rotation, as in xec_decode
  auto rotate_for = [&](const uint32_t* items, uint64_t count) {
    ls.rot = decode_rotation(items_scan(items, count, m), m, bs);
    g = xec::make_geometry(S, bs, k, m, ls);
  };
  if (n <= xec::kArgItems) {
    rotate_for(short_items, n);
    g_tiling_used = XEC_TILING_ARG_LIST;
    g_arg_cap_used = (int)xec::arg_items_capacity(n);
    return xec::launch_decode(d_data, d_parity, nullptr, g, ls, xec::kDecodeArgListTiles, stream,
                              n, short_items) == hipSuccess
               ? verdict
               : XEC_DEVICE_ERROR;
  }
  // A longer list is uploaded whole off the stream (upload_begin), or else
  // goes through the scratch in pieces of what it holds: copy a piece, rebuild
  // it, copy the next (stream order keeps a copy behind the kernel still
  // reading the previous piece).
  const StreamDevice sd(stream);  // the stream's device, as in xec_decode
  if (!sd.ok()) return XEC_DEVICE_ERROR;
  const int dev = sd.device();
  const int busy = side_uploads() ? stream_busy(stream) : 0;
  if (busy < 0) return XEC_DEVICE_ERROR;
  bool fault = false;
  Staging* sg = stage_acquire(n * 4, dev, &fault);
  if (sg == nullptr) return XEC_DEVICE_ERROR;
  uint32_t* items = static_cast<uint32_t*>(sg->host);
  (void)xec_scan_stripes(h_bitmap, S, k, m, nullptr, items, n, &n, &failures);
  rotate_for(items, n);
  g_tiling_used = XEC_TILING_LIST;
  Upload lu;
  if (busy == 1 && upload_begin(items, n * 4, dev, lu, &fault)) {
    stage_release(sg, true, lu.cs, true);
    const bool ok = upload_join(lu, stream) &&
                    xec::launch_decode(d_data, d_parity, lu.dev, g, ls, xec::kDecodeListTiles,
                                       stream, n) == hipSuccess;
    upload_end(lu, stream, true);
    return ok ? verdict : XEC_DEVICE_ERROR;
  }
  if (fault) {  // an event query or wait failed in upload_begin
    stage_release(sg, false, stream, false);
    return XEC_DEVICE_ERROR;
  }
  const size_t pad = (4 - reinterpret_cast<uintptr_t>(d_bitmap) % 4) % 4;
  const uint64_t cap = (S * (k + m) - pad) / 4;  // >= 511 here: n > 1,024 <= S*k
  uint8_t* d_items = d_bitmap + pad;
  bool queued = false, ok = true;
  for (uint64_t q0 = 0; q0 < n && ok; q0 += cap) {
    const uint64_t piece = n - q0 < cap ? n - q0 : cap;
    ok = hipMemcpyAsync(d_items, items + q0, piece * 4, hipMemcpyHostToDevice, stream) ==
         hipSuccess;
    queued |= ok;
    ok = ok && xec::launch_decode(d_data, d_parity, d_items, g, ls, xec::kDecodeListTiles, stream,
                                  piece) == hipSuccess;
  }
  stage_release(sg, queued, stream, false);
  return ok ? verdict : XEC_DEVICE_ERROR;
}

xec_status xec_decode_per_stripe(void* d_data, const void* d_parity, size_t S, size_t bs,
                                 size_t k, size_t m, const uint8_t* h_bitmap, uint8_t* d_bitmap,
                                 uint8_t* h_codes, hipStream_t stream) {
  return guarded([&] {
    return decode_per_stripe_impl(d_data, d_parity, S, bs, k, m, h_bitmap, d_bitmap, h_codes,
                                  stream);
  });
}

xec_status xec_decode_device(void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                             size_t m, const uint8_t* d_bitmap, int32_t* d_status,
                             hipStream_t stream) {
  const KernelEventsScope events_scope;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (d_bitmap == nullptr && S != 0) return XEC_INVALID_SIZE;
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  // No host view of the bitmap: the loss count is unknown, so the tiling is
  // the stripe tiling with the single-erasure residency table unless
  // xec_set_decode_tiling(2) says every class lost a block.
  const bool cls = m > 1 && g_decode_tiling == 2;
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_check(d_bitmap, g, d_status, stream) != hipSuccess) return XEC_DEVICE_ERROR;
  g.gate = d_status;
  return xec::launch_decode(d_data, d_parity, d_bitmap, g, ls,
                            cls ? xec::kDecodeClassTiles : xec::kDecodeStripeTiles,
                            stream) == hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

size_t xec_decode_device_list_bytes(size_t S, size_t k, size_t m) {
  (void)k;
  return 4 * (xec::kDevListHeader + S * m);
}

xec_status xec_decode_device_list(void* d_data, const void* d_parity, size_t S, size_t bs,
                                  size_t k, size_t m, const uint8_t* d_bitmap, void* d_work,
                                  size_t work_bytes, int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0 ||
      d_work == nullptr || reinterpret_cast<uintptr_t>(d_work) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (S != 0 && (d_bitmap == nullptr || k > kWorkItemMaxK || S > kWorkItemMaxStripes ||
                 work_bytes < xec_decode_device_list_bytes(S, k, m)))
    return XEC_INVALID_SIZE;
  if (S == 0)
    return hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) == hipSuccess ? XEC_SUCCESS
                                                                              : XEC_DEVICE_ERROR;
  // One reduction per tile, as encode: encode's residency table.  The list's
  // length is known only on the device, so the decode walks it with a grid
  // fixed at launch (unless xec_set_launch gave max_grid): one workgroup per
  // 8 possible tiles (S*m entries x chunks), at least what the chip holds at
  // once (on the stream's device) and at most kDevListMaxGrid.  A grid past
  // the list's end costs ~0.17 ns per idle workgroup; a grid of only what the
  // chip holds walks a dense list 5-18 % slower than one workgroup per tile.
  // Against that resident-only grid this was 3-5 % faster on dense lists and
  // 1-8 % on sparse ones (configs 2-4, 16+8 x 64 KiB, every stripe or 1 in 9
  // losing a block; tools/lab/devlist_grid.py, profiles/r06n).
  const StreamDevice sd(stream);
  if (!sd.ok()) return XEC_DEVICE_ERROR;
  xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (ls.max_grid == 0) {
    const uint64_t resident = resident_workgroups(ls);
    if (resident == 0) return XEC_DEVICE_ERROR;
    const uint64_t eighth = (uint64_t)S * m * g.tiles_per_block / 8;
    const uint64_t want = eighth < kDevListMaxGrid ? eighth : kDevListMaxGrid;
    ls.max_grid = (uint32_t)(want > resident ? want : resident);
  }
  uint32_t* list = static_cast<uint32_t*>(d_work);
  if (xec::launch_scan_list(d_bitmap, g, d_status, list, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  return xec::launch_decode(d_data, d_parity, reinterpret_cast<const uint8_t*>(list), g, ls,
                            xec::kDecodeDevListTiles, stream, S * m) == hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

// ---- repair and scrub ---------------------------------------------------------
// xec_repair: the host scan lists every lost block, data and parity alike
// (xec_scan_repair), and the launch is always work-list tiles, one reduction
// per tile as encode: encode's residency table.  Up to kArgItems entries
// travel in the kernel arguments; a longer list is staged in pinned memory and
// goes through the caller's scratch on `stream` in pieces of what it holds
// (copy a piece, rebuild it, copy the next: stream order keeps a copy behind
// the kernel still reading the previous piece), as xec_decode_per_stripe's
// fallback does.
static xec_status repair_impl(void* d_data, void* d_parity, size_t S, size_t bs, size_t k,
                              size_t m, const uint8_t* h_bitmap, uint8_t* d_bitmap,
                              hipStream_t stream) {
  g_repair_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  if (k + m > kRepairItemMaxRow || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  uint64_t n = 0;
  uint32_t short_items[xec::kArgItems];
  st = xec_scan_repair(h_bitmap, S, k, m, short_items, xec::kArgItems, &n);
  if (st != XEC_SUCCESS || n == 0) return st;  // verdict from the scan alone: no device call
  if (capturing(stream)) return DEVERR(hipSuccess);  // work to queue: see xec_decode
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (n <= xec::kArgItems) {
    g_repair_tiling_used = XEC_TILING_ARG_LIST;
    const hipError_t le = xec::launch_repair(d_data, d_parity, nullptr, g, ls,
                                             xec::kRepairArgListTiles, stream, n, short_items);
    return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
  }
  if (d_bitmap == nullptr) return XEC_INVALID_SIZE;  // the list needs the scratch
  const StreamDevice sd(stream);  // the stream's device, as in xec_decode
  if (!sd.ok()) return DEVERR(hipSuccess);
  bool fault = false;
  Staging* sg = stage_acquire(n * 4, sd.device(), &fault);
  if (sg == nullptr) return DEVERR(hipSuccess);
  uint32_t* items = static_cast<uint32_t*>(sg->host);
  (void)xec_scan_repair(h_bitmap, S, k, m, items, n, &n);
  g_repair_tiling_used = XEC_TILING_LIST;
  const size_t pad = (4 - reinterpret_cast<uintptr_t>(d_bitmap) % 4) % 4;
  const uint64_t cap = (S * (k + m) - pad) / 4;  // >= 255 here: n > 1,024 <= S*(k+m)
  uint8_t* d_items = d_bitmap + pad;
  bool queued = false;
  hipError_t le = hipSuccess;
  for (uint64_t q0 = 0; q0 < n && le == hipSuccess; q0 += cap) {
    const uint64_t piece = n - q0 < cap ? n - q0 : cap;
    le = hipMemcpyAsync(d_items, items + q0, piece * 4, hipMemcpyHostToDevice, stream);
    queued |= le == hipSuccess;
    if (le == hipSuccess)
      le = xec::launch_repair(d_data, d_parity, d_items, g, ls, xec::kRepairListTiles, stream,
                              piece);
  }
  stage_release(sg, queued, stream, false);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

xec_status xec_repair(void* d_data, void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                      const uint8_t* h_bitmap, uint8_t* d_bitmap, hipStream_t stream) {
  return guarded(
      [&] { return repair_impl(d_data, d_parity, S, bs, k, m, h_bitmap, d_bitmap, stream); });
}

int xec_repair_tiling_used(void) { return g_repair_tiling_used; }

xec_status xec_repair_device(void* d_data, void* d_parity, size_t S, size_t bs, size_t k,
                             size_t m, const uint8_t* d_bitmap, int32_t* d_status,
                             hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_repair_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (d_bitmap == nullptr && S != 0) return XEC_INVALID_SIZE;
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  // No host view of the bitmap: class tiles, each doing the one reduction its
  // class needs or none -- encode's tiling and residency table.
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_check(d_bitmap, g, d_status, stream) != hipSuccess) return XEC_DEVICE_ERROR;
  g.gate = d_status;
  g_repair_tiling_used = XEC_TILING_CLASS;
  return xec::launch_repair(d_data, d_parity, d_bitmap, g, ls, xec::kRepairClassTiles, stream) ==
                 hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

// Residency of verify_kernel by class member count.  It has one more load per
// lane than encode and no store stream, so encode's table was the start and
// caps 1, 2, 4 and 8 were swept once at configs 2, 3 and 4 (k/m = 8, 16, 32;
// tools/repair_scrub_bench.py --sweep, profiles/repair_scrub/): at 8 members
// one wave per SIMD was 3.0 % faster than encode's 4 (83.9 against 86.5 us,
// every round); at 16 encode's 2 tied with no cap and beat 1 and 4 by 3 %; at
// 32 caps 1, 4 and 8 were within 0.5 %, inside the run-to-run spread, so
// encode's 1 stays.  Member counts that were not swept keep encode's value.
static int verify_auto_occupancy(uint64_t nm) { return nm == 8 ? 1 : auto_occupancy(nm); }

xec_status xec_verify(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, uint8_t* d_flags, uint32_t* d_count, hipStream_t stream) {
  const KernelEventsScope events_scope;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (reinterpret_cast<uintptr_t>(d_count) % 4 != 0) return XEC_INVALID_ALIGNMENT;
  if (d_flags == nullptr && S != 0) return XEC_INVALID_SIZE;
  if (d_count != nullptr &&
      hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  if (hipMemsetAsync(d_flags, 0, S * m, stream) != hipSuccess) return XEC_DEVICE_ERROR;
  const xec::LaunchShape ls = launch_shape(bs, verify_auto_occupancy(k / m));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_verify(d_data, d_parity, d_flags, g, ls, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  if (d_count != nullptr &&
      xec::launch_count_flags(d_flags, S * m, d_count, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  return XEC_SUCCESS;
}

// ---- shard-major layout ------------------------------------------------------
// xec_encode_shards / xec_repair_shards_device / xec_verify_shards: encode, the
// class-tile repair and the scrub over one buffer per shard (include/xec.h).
// The table is read on the host before the call returns and travels in the
// kernel arguments, so there is no host work a capture would miss.  Residency:
// auto_occupancy / verify_auto_occupancy, tables swept on the batch layout and
// NOT swept on this one (tools/shards_bench.py compares the two layouts at the
// tables' values only).
static thread_local int g_shards_cap_used = 0;  // xec_shards_arg_capacity_used

// [p, p + (S-1)*stride + bs) of one shard; the caller made sure it is representable.
struct ShardHull {
  uintptr_t lo, hi;
  size_t stride;
};

// Steps 3 to 7 of xec_check_shards, S > 0.
static xec_status check_shard_table(const void* const* h_shards, size_t data_stride,
                                    size_t parity_stride, size_t S, size_t bs, size_t k,
                                    size_t m) {
  if (k > xec::kShardPtrs || m > xec::kShardPtrs - k) return XEC_INVALID_SIZE;
  const size_t n = k + m;
  if (h_shards == nullptr) return XEC_INVALID_SIZE;
  for (size_t i = 0; i < n; ++i)
    if (h_shards[i] == nullptr) return XEC_INVALID_SIZE;
  for (size_t i = 0; i < n; ++i)
    if (reinterpret_cast<uintptr_t>(h_shards[i]) % kAlign != 0) return XEC_INVALID_ALIGNMENT;
  if (data_stride % kAlign != 0 || parity_stride % kAlign != 0) return XEC_INVALID_ALIGNMENT;
  if (data_stride < bs || parity_stride < bs) return XEC_INVALID_SIZE;
  const size_t big = data_stride > parity_stride ? data_stride : parity_stride;
  if (S - 1 > (SIZE_MAX - bs) / big) return XEC_INVALID_SIZE;  // (S-1)*stride + bs in 64 bits
  ShardHull hull[xec::kShardPtrs];
  for (size_t i = 0; i < n; ++i) {
    const size_t stride = i < k ? data_stride : parity_stride;
    const size_t len = (S - 1) * stride + bs;
    const uintptr_t p = reinterpret_cast<uintptr_t>(h_shards[i]);
    if (len > UINTPTR_MAX - p) return XEC_INVALID_SIZE;  // the hull itself must not wrap
    hull[i] = ShardHull{p, p + len, stride};
  }
  for (size_t x = 0; x < n; ++x)
    for (size_t y = x + 1; y < n; ++y) {
      const ShardHull &a = hull[x], &b = hull[y];
      if (a.hi <= b.lo || b.hi <= a.lo) continue;  // disjoint hulls
      if (a.stride != b.stride) return XEC_INVALID_SIZE;
      // interleaved: the blocks of y sit at a fixed offset d inside x's stride
      const size_t s = a.stride;
      const size_t d = b.lo >= a.lo ? (b.lo - a.lo) % s : (s - (a.lo - b.lo) % s) % s;
      if (d < bs || s - d < bs) return XEC_INVALID_SIZE;
    }
  return XEC_SUCCESS;
}

xec_status xec_check_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                            size_t S, size_t bs, size_t k, size_t m) {
  const xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  return check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
}

int xec_shards_arg_capacity_used(void) { return g_shards_cap_used; }

xec_status xec_encode_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  const xec_status st = xec_check_shards(h_shards, data_stride, parity_stride, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_encode_shards(h_shards, data_stride, parity_stride, g, ls, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

xec_status xec_repair_shards_device(const void* const* h_shards, size_t data_stride,
                                    size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                    const uint8_t* d_bitmap, int32_t* d_status,
                                    hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (d_bitmap == nullptr && S != 0) return XEC_INVALID_SIZE;
  if (S != 0) {
    st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
    if (st != XEC_SUCCESS) return st;
  }
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = launch_shape(bs, auto_occupancy(k / m));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_check(d_bitmap, g, d_status, stream) != hipSuccess) return XEC_DEVICE_ERROR;
  g.gate = d_status;
  if (xec::launch_repair_shards(h_shards, data_stride, parity_stride, d_bitmap, g, ls, stream) !=
      hipSuccess)
    return XEC_DEVICE_ERROR;
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

xec_status xec_verify_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, uint8_t* d_flags,
                             uint32_t* d_count, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (reinterpret_cast<uintptr_t>(d_count) % 4 != 0) return XEC_INVALID_ALIGNMENT;
  if (d_flags == nullptr && S != 0) return XEC_INVALID_SIZE;
  if (S != 0) {
    st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
    if (st != XEC_SUCCESS) return st;
  }
  if (d_count != nullptr &&
      hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  if (hipMemsetAsync(d_flags, 0, S * m, stream) != hipSuccess) return XEC_DEVICE_ERROR;
  const xec::LaunchShape ls = launch_shape(bs, verify_auto_occupancy(k / m));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_verify_shards(h_shards, data_stride, parity_stride, d_flags, g, ls, stream) !=
      hipSuccess)
    return XEC_DEVICE_ERROR;
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  if (d_count != nullptr &&
      xec::launch_count_flags(d_flags, S * m, d_count, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  return XEC_SUCCESS;
}

// xec_digest_shards / xec_locate_shards / xec_read_shards_device: the digest, the
// locate and the device-resident degraded read over the same table.  Launch
// shape and residency are the batch calls' (digest_launch_shape: uncapped;
// read_occupancy: the table of a reconstruct tile), both defined with those
// calls further down and, again, swept on the batch layout only.
static xec::LaunchShape digest_launch_shape(size_t bs);
static int read_occupancy(uint64_t nm, size_t n_lost);
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb);

// Step 3 of xec_digest_shards (locate = false) and xec_locate_shards: the call's
// own pointers and sizes, in digest_check's order.
static xec_status digest_shards_check(size_t S, size_t k, size_t m, const void* d_digests,
                                      const void* d_work, size_t work_bytes, bool locate,
                                      const void* d_bitmap, const void* d_count) {
  if (S != 0 && d_digests == nullptr) return XEC_INVALID_SIZE;
  if (locate && ((S != 0 && d_work == nullptr) || work_bytes < xec_locate_work_bytes(S, k, m)))
    return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_digests) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(d_work) % 8 != 0 || reinterpret_cast<uintptr_t>(d_count) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (locate && S != 0 && d_bitmap == nullptr) return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

xec_status xec_digest_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, const uint8_t* d_select,
                             uint64_t* d_digests, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  st = digest_shards_check(S, k, m, d_digests, nullptr, 0, false, nullptr, nullptr);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  const xec::LaunchShape ls = digest_launch_shape(bs);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  const hipError_t e = xec::launch_digest_shards(h_shards, data_stride, parity_stride, d_select,
                                                 d_select ? xec::kDigestSelect : xec::kDigestAll,
                                                 d_digests, g, ls, stream);
  if (e != hipSuccess) return DEVERR(e);
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

xec_status xec_locate_shards(const void* const* h_shards, size_t data_stride, size_t parity_stride,
                             size_t S, size_t bs, size_t k, size_t m, const uint64_t* d_digests,
                             const uint8_t* d_flags, uint8_t* d_bitmap, uint32_t* d_count,
                             void* d_work, size_t work_bytes, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  st = digest_shards_check(S, k, m, d_digests, d_work, work_bytes, true, d_bitmap, d_count);
  if (st != XEC_SUCCESS) return st;
  if (S != 0) {
    st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
    if (st != XEC_SUCCESS) return st;
  }
  if (d_count != nullptr &&
      hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = digest_launch_shape(bs);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  uint64_t* fresh = static_cast<uint64_t*>(d_work);
  hipError_t e = xec::launch_digest_shards(h_shards, data_stride, parity_stride, d_flags,
                                           d_flags ? xec::kDigestFlags : xec::kDigestAll, fresh, g,
                                           ls, stream);
  if (e != hipSuccess) return DEVERR(e);
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  e = xec::launch_locate_compare(fresh, d_digests, d_flags, d_bitmap, d_count, g, stream);
  return e == hipSuccess ? XEC_SUCCESS : DEVERR(e);
}

// Does [out, out + bytes) meet the hull of a shard of the (checked) table?
// Ranges that only touch do not.
static bool overlaps_a_shard_hull(const void* out, size_t bytes, const void* const* h_shards,
                                  size_t data_stride, size_t parity_stride, size_t S, size_t bs,
                                  size_t k, size_t m) {
  for (size_t i = 0; i < k + m; ++i)
    if (ranges_overlap(out, bytes, h_shards[i],
                       (S - 1) * (i < k ? data_stride : parity_stride) + bs))
      return true;
  return false;
}

xec_status xec_read_shards_device(const void* const* h_shards, size_t data_stride,
                                  size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                  const uint8_t* d_bitmap, const uint32_t* d_items,
                                  size_t n_items, size_t offset, size_t len, void* d_out,
                                  int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (n_items != 0 && S != 0) {
    // steps 4 to 7 of xec_read, then d_items' alignment
    if (k + m > kRepairItemMaxRow || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
    if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset > bs || len > bs - offset)
      return XEC_INVALID_SIZE;
    if (d_out == nullptr || d_items == nullptr) return XEC_INVALID_SIZE;
    if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return XEC_INVALID_ALIGNMENT;
    if (reinterpret_cast<uintptr_t>(d_items) % 4 != 0) return XEC_INVALID_ALIGNMENT;
    st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
    if (st != XEC_SUCCESS) return st;
    if (n_items > SIZE_MAX / len ||
        overlaps_a_shard_hull(d_out, n_items * len, h_shards, data_stride, parity_stride, S, bs, k,
                              m))
      return XEC_INVALID_SIZE;
  }
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  if (n_items == 0 || S == 0) return XEC_SUCCESS;
  // No host view of the bitmap: the table of a reconstruct tile (read_occupancy).
  const xec::LaunchShape ls = launch_shape(bs, read_occupancy(k / m, d_bitmap ? 1 : 0));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_read_check(d_bitmap, d_items, n_items, g, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  const hipError_t le =
      xec::launch_read_shards(h_shards, data_stride, parity_stride, d_out, g, ls, offset, len,
                              n_items, d_items, d_bitmap, stream);
  if (le != hipSuccess) return DEVERR(le);
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

// ---- in-place block update -----------------------------------------------------
// xec_update / xec_update_device: parity[c][i % m] ^= data[c][i] ^ new, then
// data[c][i] = new, for the named blocks only: the ranged update's kernels over
// [0, bs) without digests (xec_kernels.hip, update and ranged update).  The
// delta keeps a class's syndrome, so xec_verify still flags a class that was
// already corrupt; a re-encode would not.  Residency is uncapped (a lane has
// 3-5 loads in flight, the table's 1-2 members): caps 1, 2, 4 and 8 were swept
// once with one block per stripe at configs 2, 3 and 4 (tools/update_bench.py
// --sweep, profiles/update/; on the whole-block kernels these calls had then)
// -- caps 1 and 2 cost 1.4-2.6x everywhere, 4 is 7-16 % slower, 8 equals none.
// (With the parity store still sc1, cap 4 was 3 % faster at config 3 and 7 %
// and 5 % slower at configs 2 and 4.)  The order
// of the checks is: initialisation, xec_check_args, nothing to do, then the new
// buffer and the list -- all on the host before any device call.
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na != 0 && nb != 0 && x < y + nb && y < x + na;
}

static xec_status update_check_new(const void* d_data, const void* d_parity, const void* d_new,
                                   size_t new_bytes, size_t S, size_t bs, size_t k, size_t m) {
  if (reinterpret_cast<uintptr_t>(d_new) % kAlign != 0) return XEC_INVALID_ALIGNMENT;
  if (d_new == nullptr || ranges_overlap(d_new, new_bytes, d_data, S * k * bs) ||
      ranges_overlap(d_new, new_bytes, d_parity, S * m * bs))
    return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

// What xec_update and xec_update_range do once their own argument checks have
// passed: the scratch check of a list too long for the kernel arguments, the
// capture rule, then the ranged kernels over the list by value or uploaded.
// A whole-block update is the range [0, bs) without digests.
static xec_status update_list_launch(void* d_data, void* d_parity, const void* d_new, size_t S,
                                     size_t bs, size_t k, size_t m, const uint32_t* h_items,
                                     size_t n, size_t offset, size_t len, uint64_t* d_digests,
                                     void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
  const bool in_args = n <= xec::kArgItems;
  if (!in_args) {
    const xec_status st = check_scratch(d_scratch, scratch_bytes, xec_update_scratch_bytes(n));
    if (st != XEC_SUCCESS) return st;
  }
  if (capturing(stream)) return DEVERR(hipSuccess);  // work to queue: see xec_decode
  const xec::LaunchShape ls = launch_shape(bs, 0);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (in_args) {
    g_update_tiling_used = XEC_TILING_ARG_LIST;
    return launch_status(__LINE__, xec::launch_update_range(
                                       d_data, d_parity, d_new, nullptr, d_digests, g, ls,
                                       xec::kUpdateArgListTiles, offset, len, stream, n, h_items));
  }
  return upload_list_and_launch(
      n * 4, d_scratch, stream, __LINE__,
      [&](uint32_t* staged) {
        std::memcpy(staged, h_items, n * 4);
        g_update_tiling_used = XEC_TILING_LIST;
      },
      [&] {
        return xec::launch_update_range(d_data, d_parity, d_new, d_scratch, d_digests, g, ls,
                                        xec::kUpdateListTiles, offset, len, stream, n);
      });
}

static xec_status update_impl(void* d_data, void* d_parity, const void* d_new, size_t S,
                              size_t bs, size_t k, size_t m, const uint32_t* h_items,
                              size_t n, void* d_scratch, size_t scratch_bytes,
                              hipStream_t stream) {
  g_update_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (n == 0 || S == 0) return XEC_SUCCESS;
  if (k > kWorkItemMaxK || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  st = update_check_new(d_data, d_parity, d_new, n * bs, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (h_items == nullptr || !items_ascending(h_items, n, S, k)) return XEC_INVALID_COUNTS;
  return update_list_launch(d_data, d_parity, d_new, S, bs, k, m, h_items, n, 0, bs, nullptr,
                            d_scratch, scratch_bytes, stream);
}

xec_status xec_update(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                      size_t k, size_t m, const uint32_t* h_items, size_t n_items,
                      void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
  return guarded([&] {
    return update_impl(d_data, d_parity, d_new, S, bs, k, m, h_items, n_items, d_scratch,
                       scratch_bytes, stream);
  });
}

size_t xec_update_scratch_bytes(size_t n_items) { return 4 * n_items; }

int xec_update_tiling_used(void) { return g_update_tiling_used; }

xec_status xec_update_device(void* d_data, void* d_parity, const void* d_new, size_t S,
                             size_t bs, size_t k, size_t m, const uint8_t* d_mask,
                             hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_update_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  // every argument is checked before any work is queued on the stream
  if (d_mask == nullptr) return XEC_INVALID_SIZE;
  st = update_check_new(d_data, d_parity, d_new, S * k * bs, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // No host view of the mask: class tiles, each folding its class's marked
  // members or doing nothing.
  const xec::LaunchShape ls = launch_shape(bs, 0);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  g_update_tiling_used = XEC_TILING_CLASS;
  return xec::launch_update_range(d_data, d_parity, d_new, d_mask, nullptr, g, ls,
                                  xec::kUpdateClassTiles, 0, bs, stream) == hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

// ---- block digests and locate ----------------------------------------------------
// digest(block) = sum over its u64 words of splitmix_at(w[n], n) mod 2^64
// (xec_kernels.h); xec_digest_host is that sentence on the host.
uint64_t xec_digest_host(const void* block, size_t bs) {
  const unsigned char* p = static_cast<const unsigned char*>(block);
  uint64_t sum = 0;
  for (size_t n = 0; n < bs / 8; ++n) {
    uint64_t w = 0;
    for (int b = 7; b >= 0; --b) w = (w << 8) | p[8 * n + (size_t)b];  // little-endian
    sum += xec::splitmix_at(w, n);
  }
  return sum;
}

// Launch shape of digest_kernel, swept once at configs 2, 3 and 4
// (tools/digest_bench.py --sweep, profiles/digest/; kernel times in us at
// config 2 / 3 / 4).  A lane has 8 loads in flight whatever k/m is, so there
// is one choice, not a table.
//  * Residency: no cap.  None 96.6 / 669.7 / 1717; cap 1 115.0 / 826.3 / 4926,
//    cap 2 98.9 / 669.4 / 2706, cap 4 96.2 / 668.5 / 1789, cap 8 = none (the
//    kernel's registers admit 4 waves per SIMD): a cap only loses, most at
//    config 4, whose one-tile blocks need every wave to cover their loads.
//  * Loads: nt (the library's default policy).  Default loads were 8 % slower
//    at config 2 (104.7), 11 % at config 3 (741.0), 2 % at config 4 (1759).
//  * Grid: at most kDigestMaxGrid workgroups, walking the tiles in grid
//    strides.  One workgroup per tile is the same at configs 2 and 3 (9,216 and
//    69,632 tiles: 96.7 / 668.3 against 96.1 / 669.5) but config 4 has 2.16
//    million 4 KiB tiles, and 131,072 workgroups ran them in 1559 against 1775
//    (full digest) and 457 against 704 (locate over the flags of 1 damaged
//    stripe in 9); 32,768: 1585 / 463, 8,192: 1626 / 483 and 1-4 % slower at
//    config 3, 2,048: 2146 / 858.
// The segment (kDigestSegmentBytes, xec_kernels.h): 16 KiB was 1.117 x verify
// at config 3 where 64 KiB was 1.070 and 256 KiB 1.067 (config 2 is one
// segment from 64 KiB on, config 4 always), so 64 KiB, which keeps more
// workgroups per block for small batches.
constexpr uint32_t kDigestMaxGrid = 131072;

static xec::LaunchShape digest_launch_shape(size_t bs) {
  xec::LaunchShape ls = launch_shape(bs, 0);
  if (ls.max_grid == 0) ls.max_grid = kDigestMaxGrid;
  return ls;
}

// The checks xec_digest and xec_locate share, in the order include/xec.h
// gives; d_work, d_bitmap and d_count are xec_locate's (locate = false: xec_digest).
static xec_status digest_check(const void* d_data, const void* d_parity, size_t S, size_t bs,
                               size_t k, size_t m, const void* d_digests, const void* d_work,
                               size_t work_bytes, bool locate, const void* d_bitmap,
                               const void* d_count) {
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  const xec_status st = xec_check_args(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S != 0 && d_digests == nullptr) return XEC_INVALID_SIZE;
  if (locate && ((S != 0 && d_work == nullptr) || work_bytes < xec_locate_work_bytes(S, k, m)))
    return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_digests) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(d_work) % 8 != 0 || reinterpret_cast<uintptr_t>(d_count) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (locate && S != 0 && d_bitmap == nullptr) return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

xec_status xec_digest(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, const uint8_t* d_select, uint64_t* d_digests,
                      hipStream_t stream) {
  const KernelEventsScope events_scope;
  const xec_status st = digest_check(d_data, d_parity, S, bs, k, m, d_digests, nullptr, 0, false,
                                     nullptr, nullptr);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = digest_launch_shape(bs);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  const hipError_t e = xec::launch_digest(d_data, d_parity, d_select,
                                          d_select ? xec::kDigestSelect : xec::kDigestAll,
                                          d_digests, g, ls, stream);
  return e == hipSuccess ? XEC_SUCCESS : DEVERR(e);
}

size_t xec_locate_work_bytes(size_t S, size_t k, size_t m) { return 8 * S * (k + m); }

xec_status xec_locate(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                      size_t m, const uint64_t* d_digests, const uint8_t* d_flags,
                      uint8_t* d_bitmap, uint32_t* d_count, void* d_work, size_t work_bytes,
                      hipStream_t stream) {
  const KernelEventsScope events_scope;
  const xec_status st = digest_check(d_data, d_parity, S, bs, k, m, d_digests, d_work, work_bytes,
                                     true, d_bitmap, d_count);
  if (st != XEC_SUCCESS) return st;
  if (d_count != nullptr &&
      hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  if (S == 0) return XEC_SUCCESS;
  const xec::LaunchShape ls = digest_launch_shape(bs);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  uint64_t* fresh = static_cast<uint64_t*>(d_work);
  hipError_t e = xec::launch_digest(d_data, d_parity, d_flags,
                                    d_flags ? xec::kDigestFlags : xec::kDigestAll, fresh, g, ls,
                                    stream);
  if (e == hipSuccess)
    e = xec::launch_locate_compare(fresh, d_digests, d_flags, d_bitmap, d_count, g, stream);
  return e == hipSuccess ? XEC_SUCCESS : DEVERR(e);
}

// ---- degraded read ----------------------------------------------------------------
// xec_read / xec_read_device: bytes [offset, offset + len) of the blocks the
// items name, packed into d_out; a lost block's range is reconstructed from
// the same range of the other blocks of its class (xec_kernels.hip, degraded
// read).  Nothing but d_out is written.  Always list tiles, one per (item,
// chunk of the range).
//
// Residency (read_occupancy).  A reconstruct tile is one class reduction, as a
// tile of encode or of the list decode, so it starts from their table
// (auto_occupancy); a copy tile has one load in flight per lane, which a cap
// only starves, so a list the host scan found free of losses runs uncapped.
// The device form cannot know and takes the table.
// Swept once, capped against uncapped, at configs 2, 3 and 4 (k/m = 8, 16, 32)
// with one whole lost block per stripe and with the same blocks present
// (tools/read_bench.py --sweep, profiles/read/; kernel times in us, cap 0 = this
// function's choice):
//   reconstruct  cap 0    1      2      4      8 (none)
//     config 2   95.5   124.3  105.1   94.9   95.7      (the table's 4 = none)
//     config 3   683.1  767.8  685.0  739.1  716.3      (the table's 2: 4.6 % ahead of none)
//     config 4   1249   1248   1343   1309   1317       (the table's 1: 5.2 % ahead of none)
//   copy
//     config 2   21.9    78.1   46.9   30.2   21.9
//     config 3   84.8   304.3  184.8  112.7   84.8
//     config 4   163.8  372.4  224.3  163.9  163.7
// so the table stands for reconstructions, and a copy wants every wave it can
// get.  (Taken with d_out stored nt; the shipped sc1 store is 0.5-3 % faster
// in each row, xec_kernels.hip.)
static int read_occupancy(uint64_t nm, size_t n_lost) { return n_lost == 0 ? 0 : auto_occupancy(nm); }

static thread_local int g_read_tiling_used = 0;  // xec_read_tiling_used: this thread's last read

// The checks both forms share once the items' source is set aside, in
// include/xec.h's order (steps 4 to 8; `items` is h_items or d_items).
static xec_status read_check_range(const void* d_data, const void* d_parity, size_t S, size_t bs,
                                   size_t k, size_t m, const void* items, size_t n, size_t offset,
                                   size_t len, const void* d_out) {
  if (k + m > kRepairItemMaxRow || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset > bs || len > bs - offset)
    return XEC_INVALID_SIZE;
  if (d_out == nullptr || items == nullptr) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return XEC_INVALID_ALIGNMENT;
  if (n > SIZE_MAX / len || ranges_overlap(d_out, n * len, d_data, S * k * bs) ||
      ranges_overlap(d_out, n * len, d_parity, S * m * bs))
    return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

static xec_status read_impl(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                            size_t m, const uint8_t* h_bitmap, const uint32_t* h_items, size_t n,
                            size_t offset, size_t len, void* d_out, void* d_scratch,
                            size_t scratch_bytes, hipStream_t stream) {
  g_read_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (n == 0 || S == 0) return XEC_SUCCESS;
  st = read_check_range(d_data, d_parity, S, bs, k, m, h_items, n, offset, len, d_out);
  if (st != XEC_SUCCESS) return st;
  const bool in_args = n <= xec::kArgItems;
  uint32_t short_bits[xec::kArgItems / 32];
  size_t n_lost = 0;
  st = xec_scan_read_items(h_bitmap, S, k, m, h_items, n, in_args ? short_bits : nullptr, &n_lost);
  if (st != XEC_SUCCESS) return st;
  if (!in_args) {
    st = check_scratch(d_scratch, scratch_bytes, xec_read_scratch_bytes(n));
    if (st != XEC_SUCCESS) return st;
  }
  if (capturing(stream)) return DEVERR(hipSuccess);  // work to queue: see xec_decode
  const xec::LaunchShape ls = launch_shape(bs, read_occupancy(k / m, n_lost));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (in_args) {
    g_read_tiling_used = XEC_TILING_ARG_LIST;
    return launch_status(
        __LINE__, xec::launch_read(d_data, d_parity, d_out, g, ls, xec::kReadArgListTiles, offset,
                                   len, n, nullptr, nullptr, h_items, short_bits, stream));
  }
  // items, then their loss bits, in one copy
  return upload_list_and_launch(
      xec_read_scratch_bytes(n), d_scratch, stream, __LINE__,
      [&](uint32_t* staged) {
        std::memcpy(staged, h_items, n * 4);
        (void)xec_scan_read_items(h_bitmap, S, k, m, h_items, n, staged + n, nullptr);
        g_read_tiling_used = XEC_TILING_LIST;
      },
      [&] {
        return xec::launch_read(d_data, d_parity, d_out, g, ls, xec::kReadListTiles, offset, len,
                                n, static_cast<const uint32_t*>(d_scratch), nullptr, nullptr,
                                nullptr, stream);
      });
}

xec_status xec_read(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                    size_t m, const uint8_t* h_bitmap, const uint32_t* h_items, size_t n_items,
                    size_t offset, size_t len, void* d_out, void* d_scratch, size_t scratch_bytes,
                    hipStream_t stream) {
  return guarded([&] {
    return read_impl(d_data, d_parity, S, bs, k, m, h_bitmap, h_items, n_items, offset, len, d_out,
                     d_scratch, scratch_bytes, stream);
  });
}

size_t xec_read_scratch_bytes(size_t n_items) { return 4 * xec::read_list_words(n_items); }

int xec_read_tiling_used(void) { return g_read_tiling_used; }

xec_status xec_read_device(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                           size_t m, const uint8_t* d_bitmap, const uint32_t* d_items,
                           size_t n_items, size_t offset, size_t len, void* d_out,
                           int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_read_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (n_items != 0 && S != 0) {
    st = read_check_range(d_data, d_parity, S, bs, k, m, d_items, n_items, offset, len, d_out);
    if (st != XEC_SUCCESS) return st;
    if (reinterpret_cast<uintptr_t>(d_items) % 4 != 0) return XEC_INVALID_ALIGNMENT;
  }
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  if (n_items == 0 || S == 0) return XEC_SUCCESS;
  // No host view of the bitmap: the table of a reconstruct tile (read_occupancy).
  const xec::LaunchShape ls = launch_shape(bs, read_occupancy(k / m, d_bitmap ? 1 : 0));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_read_check(d_bitmap, d_items, n_items, g, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  g_read_tiling_used = XEC_TILING_LIST;
  const hipError_t le =
      xec::launch_read(d_data, d_parity, d_out, g, ls, xec::kReadDevTiles, offset, len, n_items,
                       d_items, d_bitmap, nullptr, nullptr, stream);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

// ---- vectored degraded read --------------------------------------------------------
// xec_readv / xec_readv_device: xec_read with a range per entry.  The tile
// schedule is a table (xec_internal.h, xec_plan_readv) instead of a division:
// entry t owns tiles [tile[t], tile[t + 1]) and bytes [out[t], out[t + 1]) of
// d_out, and a tile finds its entry by binary search (xec_kernels.hip, vectored
// read).  Residency as xec_read (read_occupancy).
static thread_local int g_readv_tiling_used = 0;  // xec_readv_tiling_used: this thread's last readv

static xec_status readv_check_batch(size_t S, size_t bs, size_t k, size_t m) {
  if (k + m > kRepairItemMaxRow || S > kWorkItemMaxStripes || (uint64_t)bs >= (1ull << 32))
    return XEC_INVALID_SIZE;
  return XEC_SUCCESS;
}

static xec_status readv_impl(const void* d_data, const void* d_parity, size_t S, size_t bs,
                             size_t k, size_t m, const uint8_t* h_bitmap, const xec_iov* h_iov,
                             size_t n, void* d_out, size_t out_bytes, void* d_scratch,
                             size_t scratch_bytes, hipStream_t stream) {
  g_readv_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (n == 0 || S == 0) return XEC_SUCCESS;
  st = readv_check_batch(S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (d_out == nullptr || h_iov == nullptr) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return XEC_INVALID_ALIGNMENT;
  // The tile size is the launch shape's; the residency, which needs the plan's
  // loss count, is set once the plan is known.
  xec::LaunchShape ls = launch_shape(bs, 0);
  const size_t tile_bytes = 16 * (size_t)ls.threads * (size_t)ls.unroll;
  // Six words per entry: 256 entries are 6 KiB of kernel arguments, 1,024 would
  // ship 24 KiB with every launch.
  const bool in_args = n <= xec::kReadvArgEntries;
  const size_t cap = in_args ? xec::readv_capacity(n) : n;
  uint32_t short_table[xec_readv_table_words(xec::kReadvArgEntries)];
  XecReadvPlan plan;
  (void)xec_plan_readv(h_bitmap, S, bs, k, m, h_iov, n, tile_bytes, cap,
                       in_args ? short_table : nullptr, &plan);
  if (plan.range_status != XEC_SUCCESS) return plan.range_status;
  if (plan.total_bytes > out_bytes || plan.total_tiles > 0xFFFFFFFFull ||
      ranges_overlap(d_out, plan.total_bytes, d_data, S * k * bs) ||
      ranges_overlap(d_out, plan.total_bytes, d_parity, S * m * bs))
    return XEC_INVALID_SIZE;
  if (plan.items_status != XEC_SUCCESS) return plan.items_status;
  if (!in_args) {
    st = check_scratch(d_scratch, scratch_bytes, xec_readv_scratch_bytes(n));
    if (st != XEC_SUCCESS) return st;
  }
  if (capturing(stream)) return DEVERR(hipSuccess);  // work to queue: see xec_decode
  ls = launch_shape(bs, read_occupancy(k / m, plan.n_lost));
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (in_args) {
    g_readv_tiling_used = XEC_TILING_ARG_LIST;
    return launch_status(__LINE__,
                         xec::launch_readv(d_data, d_parity, d_out, g, ls, xec::kReadArgListTiles, n,
                                           plan.total_tiles, nullptr, short_table, stream));
  }
  return upload_list_and_launch(
      xec_readv_scratch_bytes(n), d_scratch, stream, __LINE__,
      [&](uint32_t* staged) {
        (void)xec_plan_readv(h_bitmap, S, bs, k, m, h_iov, n, tile_bytes, n, staged, nullptr);
        g_readv_tiling_used = XEC_TILING_LIST;
      },
      [&] {
        return xec::launch_readv(d_data, d_parity, d_out, g, ls, xec::kReadListTiles, n,
                                 plan.total_tiles, static_cast<const uint32_t*>(d_scratch), nullptr,
                                 stream);
      });
}

xec_status xec_readv(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                     size_t m, const uint8_t* h_bitmap, const xec_iov* h_iov, size_t n_items,
                     void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes,
                     hipStream_t stream) {
  return guarded([&] {
    return readv_impl(d_data, d_parity, S, bs, k, m, h_bitmap, h_iov, n_items, d_out, out_bytes,
                      d_scratch, scratch_bytes, stream);
  });
}

size_t xec_readv_scratch_bytes(size_t n_items) { return 4 * xec_readv_table_words(n_items); }

size_t xec_readv_device_work_bytes(size_t n_items) {
  return n_items ? (4 * xec::readv_work_words(n_items) + 7) / 8 * 8 : 0;
}

int xec_readv_tiling_used(void) { return g_readv_tiling_used; }

xec_status xec_readv_device(const void* d_data, const void* d_parity, size_t S, size_t bs, size_t k,
                            size_t m, const uint8_t* d_bitmap, const xec_iov* d_iov,
                            size_t n_items, void* d_out, size_t out_bytes, void* d_work,
                            size_t work_bytes, int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_readv_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (n_items == 0 || S == 0)
    return hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) == hipSuccess ? XEC_SUCCESS
                                                                              : XEC_DEVICE_ERROR;
  st = readv_check_batch(S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (d_out == nullptr || d_iov == nullptr || d_work == nullptr) return XEC_INVALID_SIZE;
  if (work_bytes < xec_readv_device_work_bytes(n_items)) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || reinterpret_cast<uintptr_t>(d_iov) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(d_work) % 8 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (ranges_overlap(d_out, out_bytes, d_data, S * k * bs) ||
      ranges_overlap(d_out, out_bytes, d_parity, S * m * bs))
    return XEC_INVALID_SIZE;
  // the most tiles an entry can have is at the smallest tile, 1 KiB
  if ((uint64_t)n_items > 0xFFFFFFFFull / (((uint64_t)bs + 1023) / 1024)) return XEC_INVALID_SIZE;
  const StreamDevice sd(stream);
  if (!sd.ok()) return XEC_DEVICE_ERROR;
  // No host view of the bitmap: the table of a reconstruct tile (read_occupancy).
  xec::LaunchShape ls = launch_shape(bs, read_occupancy(k / m, d_bitmap ? 1 : 0));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  // The totals are known only on the device, so the read kernel walks them with
  // a grid fixed at launch from the most tiles out_bytes and n_items admit (an
  // entry's last tile may be a partial one), clamped as xec_decode_device_list
  // clamps its grid.
  const uint64_t tile_bytes = 16ull * (uint64_t)ls.threads * (uint64_t)ls.unroll;
  const uint64_t bound = (uint64_t)out_bytes / tile_bytes + n_items;
  if (ls.max_grid == 0) {
    const uint64_t resident = resident_workgroups(ls);
    if (resident == 0) return XEC_DEVICE_ERROR;
    const uint64_t want = bound / 8 < kDevListMaxGrid ? bound / 8 : kDevListMaxGrid;
    ls.max_grid = (uint32_t)(want > resident ? want : resident);
  }
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  uint32_t* work = static_cast<uint32_t*>(d_work);
  const uint32_t* iov = reinterpret_cast<const uint32_t*>(d_iov);
  if (xec::launch_readv_check(d_bitmap, iov, n_items, g, tile_bytes, work, d_status, stream) !=
          hipSuccess ||
      xec::launch_readv_scan(work, n_items, out_bytes, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  g_readv_tiling_used = XEC_TILING_LIST;
  const hipError_t le = xec::launch_readv(d_data, d_parity, d_out, g, ls, xec::kReadDevTiles, n_items,
                                          bound, iov, nullptr, stream, d_bitmap, work);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

// ---- ranged update with digest upkeep ------------------------------------------------
// xec_update_range / xec_update_range_device: xec_update over bytes
// [offset, offset + len) of each named block, and with d_digests the stored
// digests of the touched data and parity blocks follow in the same pass
// (xec_kernels.hip, update and ranged update).  Residency is uncapped, as for
// xec_update, which runs the same kernels.  xec_digest_range_host is the host's
// side of the upkeep identity.
uint64_t xec_digest_range_host(const void* bytes, size_t offset, size_t len) {
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  const uint64_t n0 = offset / 8;
  uint64_t sum = 0;
  for (size_t n = 0; n < len / 8; ++n) {
    uint64_t w = 0;
    for (int b = 7; b >= 0; --b) w = (w << 8) | p[8 * n + (size_t)b];  // little-endian
    sum += xec::splitmix_at(w, n0 + n);
  }
  return sum;
}

// Steps 5 to 8 of include/xec.h's list, shared by both forms; `new_bytes` is
// the extent of d_new (n_items*len packed, or the shadow's S*k*bs).
static xec_status update_range_check(const void* d_data, const void* d_parity, const void* d_new,
                                     size_t new_bytes, const void* sel, size_t S, size_t bs,
                                     size_t k, size_t m, size_t offset, size_t len,
                                     const uint64_t* d_digests) {
  if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset > bs || len > bs - offset)
    return XEC_INVALID_SIZE;
  if (d_new == nullptr || sel == nullptr) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_new) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(d_digests) % 8 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (ranges_overlap(d_new, new_bytes, d_data, S * k * bs) ||
      ranges_overlap(d_new, new_bytes, d_parity, S * m * bs))
    return XEC_INVALID_SIZE;
  if (d_digests != nullptr) {
    const size_t dig_bytes = 8 * S * (k + m);
    if (ranges_overlap(d_digests, dig_bytes, d_data, S * k * bs) ||
        ranges_overlap(d_digests, dig_bytes, d_parity, S * m * bs) ||
        ranges_overlap(d_digests, dig_bytes, d_new, new_bytes))
      return XEC_INVALID_SIZE;
  }
  return XEC_SUCCESS;
}

static xec_status update_range_impl(void* d_data, void* d_parity, const void* d_new, size_t S,
                                    size_t bs, size_t k, size_t m, const uint32_t* h_items,
                                    size_t n, size_t offset, size_t len, uint64_t* d_digests,
                                    void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
  g_update_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (n == 0 || S == 0) return XEC_SUCCESS;
  if (k > kWorkItemMaxK || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  if (len != 0 && n > SIZE_MAX / len) return XEC_INVALID_SIZE;
  st = update_range_check(d_data, d_parity, d_new, n * len, h_items, S, bs, k, m, offset, len,
                          d_digests);
  if (st != XEC_SUCCESS) return st;
  if (!items_ascending(h_items, n, S, k)) return XEC_INVALID_COUNTS;
  return update_list_launch(d_data, d_parity, d_new, S, bs, k, m, h_items, n, offset, len,
                            d_digests, d_scratch, scratch_bytes, stream);
}

xec_status xec_update_range(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                            size_t k, size_t m, const uint32_t* h_items, size_t n_items,
                            size_t offset, size_t len, uint64_t* d_digests, void* d_scratch,
                            size_t scratch_bytes, hipStream_t stream) {
  return guarded([&] {
    return update_range_impl(d_data, d_parity, d_new, S, bs, k, m, h_items, n_items, offset, len,
                             d_digests, d_scratch, scratch_bytes, stream);
  });
}

xec_status xec_update_range_device(void* d_data, void* d_parity, const void* d_new, size_t S,
                                   size_t bs, size_t k, size_t m, const uint8_t* d_mask,
                                   size_t offset, size_t len, uint64_t* d_digests,
                                   hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_update_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  // every argument is checked before any work is queued on the stream
  st = update_range_check(d_data, d_parity, d_new, S * k * bs, d_mask, S, bs, k, m, offset, len,
                          d_digests);
  if (st != XEC_SUCCESS) return st;
  const xec::LaunchShape ls = launch_shape(bs, 0);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  g_update_tiling_used = XEC_TILING_CLASS;
  const hipError_t le =
      xec::launch_update_range(d_data, d_parity, d_new, d_mask, d_digests, g, ls,
                               xec::kUpdateClassTiles, offset, len, stream);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

// ---- degraded write --------------------------------------------------------------------
// xec_write / xec_write_device: xec_update_range under a loss bitmap
// (xec_kernels.hip, degraded write).  The host scan hands every item two bits
// (its block lost, its class's parity lost); they travel with the list as
// xec_read's loss bits do.  Residency is uncapped in every mode: the sweep of
// the rebuild mode is recorded in DESIGN.md §3 *Degraded write*.
static thread_local int g_write_tiling_used = 0;  // xec_write_tiling_used: this thread's last write

static xec_status write_impl(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                             size_t k, size_t m, const uint8_t* h_bitmap, const uint32_t* h_items,
                             size_t n, size_t offset, size_t len, uint64_t* d_digests,
                             void* d_scratch, size_t scratch_bytes, hipStream_t stream) {
  g_write_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (n == 0 || S == 0) return XEC_SUCCESS;
  if (k > kWorkItemMaxK || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  if (len != 0 && n > SIZE_MAX / len) return XEC_INVALID_SIZE;
  st = update_range_check(d_data, d_parity, d_new, n * len, h_items, S, bs, k, m, offset, len,
                          d_digests);
  if (st != XEC_SUCCESS) return st;
  const bool in_args = n <= xec::kArgItems;
  uint32_t short_bits[xec::kArgItems / 16];
  st = xec_scan_write_items(h_bitmap, S, k, m, h_items, n, in_args ? short_bits : nullptr, nullptr,
                            nullptr);
  if (st != XEC_SUCCESS) return st;
  if (!in_args) {
    st = check_scratch(d_scratch, scratch_bytes, xec_write_scratch_bytes(n));
    if (st != XEC_SUCCESS) return st;
  }
  if (capturing(stream)) return DEVERR(hipSuccess);  // work to queue: see xec_decode
  const xec::LaunchShape ls = launch_shape(bs, 0);
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (in_args) {
    g_write_tiling_used = XEC_TILING_ARG_LIST;
    return launch_status(
        __LINE__, xec::launch_write(d_data, d_parity, d_new, nullptr, nullptr, d_digests, g, ls,
                                    xec::kUpdateArgListTiles, offset, len, stream, n, h_items,
                                    short_bits));
  }
  // items, then their loss bits, in one copy
  return upload_list_and_launch(
      xec_write_scratch_bytes(n), d_scratch, stream, __LINE__,
      [&](uint32_t* staged) {
        std::memcpy(staged, h_items, n * 4);
        (void)xec_scan_write_items(h_bitmap, S, k, m, h_items, n, staged + n, nullptr, nullptr);
        g_write_tiling_used = XEC_TILING_LIST;
      },
      [&] {
        return xec::launch_write(d_data, d_parity, d_new, d_scratch, nullptr, d_digests, g, ls,
                                 xec::kUpdateListTiles, offset, len, stream, n);
      });
}

xec_status xec_write(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs, size_t k,
                     size_t m, const uint8_t* h_bitmap, const uint32_t* h_items, size_t n_items,
                     size_t offset, size_t len, uint64_t* d_digests, void* d_scratch,
                     size_t scratch_bytes, hipStream_t stream) {
  return guarded([&] {
    return write_impl(d_data, d_parity, d_new, S, bs, k, m, h_bitmap, h_items, n_items, offset,
                      len, d_digests, d_scratch, scratch_bytes, stream);
  });
}

size_t xec_write_scratch_bytes(size_t n_items) { return 4 * xec::write_list_words(n_items); }

int xec_write_tiling_used(void) { return g_write_tiling_used; }

xec_status xec_write_device(void* d_data, void* d_parity, const void* d_new, size_t S, size_t bs,
                            size_t k, size_t m, const uint8_t* d_bitmap, const uint8_t* d_mask,
                            size_t offset, size_t len, uint64_t* d_digests, int32_t* d_status,
                            hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_write_tiling_used = 0;
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  // every argument is checked before any work is queued on the stream
  st = update_range_check(d_data, d_parity, d_new, S * k * bs, d_mask, S, bs, k, m, offset, len,
                          d_digests);
  if (st != XEC_SUCCESS) return st;
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  const xec::LaunchShape ls = launch_shape(bs, 0);
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_write_check(d_bitmap, d_mask, g, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  g_write_tiling_used = XEC_TILING_CLASS;
  const hipError_t le =
      xec::launch_write(d_data, d_parity, d_new, d_mask, d_bitmap, d_digests, g, ls,
                        xec::kUpdateClassTiles, offset, len, stream);
  return le == hipSuccess ? XEC_SUCCESS : DEVERR(le);
}

// ---- shard-major degraded write and vectored read ---------------------------------------
// xec_write_shards_device / xec_readv_shards_device: the list-tiled degraded
// write with its list checked on the device, and xec_readv_device, both over a
// shard table (xec_kernels.hip).  Launch shape and residency are the batch
// calls' (uncapped for the write; read_occupancy for the read), swept on the
// batch layout only.  Neither touches xec_write_tiling_used or
// xec_readv_tiling_used, as xec_read_shards_device leaves xec_read_tiling_used.
xec_status xec_write_shards_device(const void* const* h_shards, size_t data_stride,
                                   size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                   const uint8_t* d_bitmap, const uint32_t* d_items,
                                   size_t n_items, size_t offset, size_t len, const void* d_new,
                                   uint64_t* d_digests, int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (n_items == 0 || S == 0)
    return hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) == hipSuccess ? XEC_SUCCESS
                                                                              : XEC_DEVICE_ERROR;
  if (k + m > kRepairItemMaxRow || S > kWorkItemMaxStripes) return XEC_INVALID_SIZE;
  if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset > bs || len > bs - offset)
    return XEC_INVALID_SIZE;
  if (d_new == nullptr || d_items == nullptr) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_new) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(d_items) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(d_digests) % 8 != 0)
    return XEC_INVALID_ALIGNMENT;
  // the tile count is at most n_items * len / 16, so it fits once n_items * len does
  if (n_items > SIZE_MAX / len) return XEC_INVALID_SIZE;
  st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  const size_t new_bytes = n_items * len, dig_bytes = d_digests ? 8 * S * (k + m) : 0;
  if (overlaps_a_shard_hull(d_new, new_bytes, h_shards, data_stride, parity_stride, S, bs, k, m) ||
      overlaps_a_shard_hull(d_digests, dig_bytes, h_shards, data_stride, parity_stride, S, bs, k,
                            m) ||
      ranges_overlap(d_new, new_bytes, d_digests, dig_bytes))
    return XEC_INVALID_SIZE;
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  const xec::LaunchShape ls = launch_shape(bs, 0);
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  if (xec::launch_write_items_check(d_bitmap, d_items, n_items, g, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  const hipError_t le =
      xec::launch_write_shards(h_shards, data_stride, parity_stride, d_new, d_items, d_bitmap,
                               d_digests, g, ls, offset, len, n_items, stream);
  if (le != hipSuccess) return DEVERR(le);
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

xec_status xec_readv_shards_device(const void* const* h_shards, size_t data_stride,
                                   size_t parity_stride, size_t S, size_t bs, size_t k, size_t m,
                                   const uint8_t* d_bitmap, const xec_iov* d_iov, size_t n_items,
                                   void* d_out, size_t out_bytes, void* d_work, size_t work_bytes,
                                   int32_t* d_status, hipStream_t stream) {
  const KernelEventsScope events_scope;
  g_shards_cap_used = 0;
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  xec_status st = xec_check_args(nullptr, nullptr, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  // every argument is checked before any work is queued on the stream
  if (d_status == nullptr || reinterpret_cast<uintptr_t>(d_status) % 4 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (n_items == 0 || S == 0)
    return hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) == hipSuccess ? XEC_SUCCESS
                                                                              : XEC_DEVICE_ERROR;
  st = readv_check_batch(S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (d_out == nullptr || d_iov == nullptr || d_work == nullptr) return XEC_INVALID_SIZE;
  if (work_bytes < xec_readv_device_work_bytes(n_items)) return XEC_INVALID_SIZE;
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || reinterpret_cast<uintptr_t>(d_iov) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(d_work) % 8 != 0)
    return XEC_INVALID_ALIGNMENT;
  st = check_shard_table(h_shards, data_stride, parity_stride, S, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (overlaps_a_shard_hull(d_out, out_bytes, h_shards, data_stride, parity_stride, S, bs, k, m))
    return XEC_INVALID_SIZE;
  // the most tiles an entry can have is at the smallest tile, 1 KiB
  if ((uint64_t)n_items > 0xFFFFFFFFull / (((uint64_t)bs + 1023) / 1024)) return XEC_INVALID_SIZE;
  const StreamDevice sd(stream);
  if (!sd.ok()) return XEC_DEVICE_ERROR;
  xec::LaunchShape ls = launch_shape(bs, read_occupancy(k / m, d_bitmap ? 1 : 0));
  xec::Geometry g = xec::make_geometry(S, bs, k, m, ls);
  // the grid bound of xec_readv_device
  const uint64_t tile_bytes = 16ull * (uint64_t)ls.threads * (uint64_t)ls.unroll;
  const uint64_t bound = (uint64_t)out_bytes / tile_bytes + n_items;
  if (ls.max_grid == 0) {
    const uint64_t resident = resident_workgroups(ls);
    if (resident == 0) return XEC_DEVICE_ERROR;
    const uint64_t want = bound / 8 < kDevListMaxGrid ? bound / 8 : kDevListMaxGrid;
    ls.max_grid = (uint32_t)(want > resident ? want : resident);
  }
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t), stream) != hipSuccess) return XEC_DEVICE_ERROR;
  uint32_t* work = static_cast<uint32_t*>(d_work);
  const uint32_t* iov = reinterpret_cast<const uint32_t*>(d_iov);
  if (xec::launch_readv_check(d_bitmap, iov, n_items, g, tile_bytes, work, d_status, stream) !=
          hipSuccess ||
      xec::launch_readv_scan(work, n_items, out_bytes, d_status, stream) != hipSuccess)
    return XEC_DEVICE_ERROR;
  g.gate = d_status;
  const hipError_t le =
      xec::launch_readv_shards(h_shards, data_stride, parity_stride, d_out, g, ls, n_items, bound,
                               iov, d_bitmap, work, stream);
  if (le != hipSuccess) return DEVERR(le);
  g_shards_cap_used = (int)xec::shard_tab_capacity(k + m);
  return XEC_SUCCESS;
}

xec_status xec_erase(void* d_data, void* d_parity, size_t S, size_t bs, size_t k, size_t m,
                     const uint8_t* d_bitmap, hipStream_t stream) {
  xec_status st = check_entry(d_data, d_parity, bs, k, m);
  if (st != XEC_SUCCESS) return st;
  if (S == 0) return XEC_SUCCESS;
  const xec::Geometry g = xec::make_geometry(S, bs, k, m, xec::LaunchShape{256, 1, 0, false, 0});
  return xec::launch_erase(d_data, d_parity, d_bitmap, g, stream) == hipSuccess ? XEC_SUCCESS
                                                                               : XEC_DEVICE_ERROR;
}

xec_status xec_fill_splitmix64(void* d_buf, size_t S, size_t stripe_bytes, uint64_t seed_base,
                               hipStream_t stream) {
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  if (reinterpret_cast<uintptr_t>(d_buf) % 8 != 0) return XEC_INVALID_ALIGNMENT;
  if (stripe_bytes % 8 != 0) return XEC_INVALID_SIZE;
  return xec::launch_fill(d_buf, S, stripe_bytes / 8, seed_base, stream) == hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

xec_status xec_write_validation_pattern(void* d_data, size_t nblocks, size_t bs, uint64_t seed,
                                        hipStream_t stream) {
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  if (bs < 2) return XEC_INVALID_SIZE;
  if (bs >= 16 && bs % 16 == 0 && reinterpret_cast<uintptr_t>(d_data) % 16 != 0)
    return XEC_INVALID_ALIGNMENT;
  return xec::launch_pattern(d_data, nblocks, bs, seed, stream) == hipSuccess ? XEC_SUCCESS
                                                                              : XEC_DEVICE_ERROR;
}

xec_status xec_validate_blocks(const void* d_data, size_t nblocks, size_t bs, uint32_t* d_bad,
                               hipStream_t stream) {
  if (!g_initialised.load(std::memory_order_acquire)) return XEC_NOT_INITIALIZED;
  if (bs >= 16 && bs % 16 == 0 && reinterpret_cast<uintptr_t>(d_data) % 16 != 0)
    return XEC_INVALID_ALIGNMENT;
  if (reinterpret_cast<uintptr_t>(d_bad) % 4 != 0) return XEC_INVALID_ALIGNMENT;
  return xec::launch_validate(d_data, nblocks, bs, d_bad, stream) == hipSuccess
             ? XEC_SUCCESS
             : XEC_DEVICE_ERROR;
}

xec_status xec_set_launch(int unroll, int max_grid, int cache_policy, int block_threads) {
  if (unroll != 0 && unroll != 1 && unroll != 2) return XEC_INVALID_SIZE;
  if (max_grid < 0 || cache_policy < 0 || cache_policy > 2) return XEC_INVALID_SIZE;
  if (block_threads != 0 && block_threads != 64 && block_threads != 256) return XEC_INVALID_SIZE;
  g_threads = block_threads;
  g_unroll = unroll;
  g_max_grid = max_grid;
  g_nt = cache_policy;
  return XEC_SUCCESS;
}

xec_status xec_set_occupancy(int waves_per_simd) {
  if (waves_per_simd < 0 || waves_per_simd > 8) return XEC_INVALID_SIZE;
  g_occupancy = waves_per_simd;
  return XEC_SUCCESS;
}

xec_status xec_set_decode_tiling(int tiling) {
  if (tiling < 0 || tiling > 4) return XEC_INVALID_SIZE;
  g_decode_tiling = tiling;
  return XEC_SUCCESS;
}

xec_status xec_set_validate_kernel(int mode) {
  if (mode < 0 || mode > 2) return XEC_INVALID_SIZE;
  xec::g_validate_mode = mode;
  return XEC_SUCCESS;
}

xec_status xec_set_rotation(int tiles) {
  if (tiles < -1 || tiles > kMaxRotation) return XEC_INVALID_SIZE;
  g_rotation = tiles;
  return XEC_SUCCESS;
}

xec_status xec_get_tuning(xec_tuning* out) {
  if (out == nullptr) return XEC_INVALID_ALIGNMENT;
  out->rotation = g_rotation;
  out->unroll = g_unroll;
  out->max_grid = g_max_grid;
  out->cache_policy = g_nt;
  out->block_threads = g_threads;
  out->waves_per_simd = g_occupancy;
  out->decode_tiling = g_decode_tiling;
  out->validate_kernel = xec::g_validate_mode;
  return XEC_SUCCESS;
}

xec_status xec_set_tuning(const xec_tuning* in) {
  if (in == nullptr) return XEC_INVALID_ALIGNMENT;
  // all or nothing: each setter checks its own fields; if any rejects, the
  // thread's previous values are put back
  const xec_tuning keep = [] {
    xec_tuning t{};
    (void)xec_get_tuning(&t);
    return t;
  }();
  if (xec_set_launch(in->unroll, in->max_grid, in->cache_policy, in->block_threads) !=
          XEC_SUCCESS ||
      xec_set_occupancy(in->waves_per_simd) != XEC_SUCCESS ||
      xec_set_decode_tiling(in->decode_tiling) != XEC_SUCCESS ||
      xec_set_validate_kernel(in->validate_kernel) != XEC_SUCCESS ||
      xec_set_rotation(in->rotation) != XEC_SUCCESS) {
    g_unroll = keep.unroll;
    g_max_grid = keep.max_grid;
    g_nt = keep.cache_policy;
    g_threads = keep.block_threads;
    g_occupancy = keep.waves_per_simd;
    g_decode_tiling = keep.decode_tiling;
    xec::g_validate_mode = keep.validate_kernel;
    g_rotation = keep.rotation;
    return XEC_INVALID_SIZE;
  }
  return XEC_SUCCESS;
}

const char* xec_status_string(xec_status s) {
  switch (s) {
    case XEC_SUCCESS: return "Success";
    case XEC_INVALID_SIZE: return "InvalidSize";
    case XEC_INVALID_ALIGNMENT: return "InvalidAlignment";
    case XEC_INVALID_COUNTS: return "InvalidCounts";
    case XEC_DECODE_FAILURE: return "DecodeFailure";
    case XEC_NOT_INITIALIZED: return "NotInitialized";
    case XEC_DEVICE_ERROR: return "DeviceError";
  }
  return "Unknown";
}

#ifndef XEC_SRC_ID
#define XEC_SRC_ID "unknown"
#endif
// "src:<id>": the hash of the library's sources (erasure-code-benchmark_amd/Makefile)
xec_status xec_peer_link(int device, int peer, xec_peer_link_info* out) {
  int n = 0;
  if (out == nullptr) return XEC_INVALID_COUNTS;
  if (hipGetDeviceCount(&n) != hipSuccess) return XEC_DEVICE_ERROR;
  if (device < 0 || peer < 0 || device >= n || peer >= n) return XEC_INVALID_COUNTS;
  xec_peer_link_info r{1, -1, -1};
  if (device != peer) {
    if (hipDeviceCanAccessPeer(&r.can_access_peer, device, peer) != hipSuccess)
      return XEC_DEVICE_ERROR;
    uint32_t type = 0, hops = 0;
    // A pair the runtime knows no link for reports an error: that is "none",
    // not a failure of this call.  The error is ours to clear -- unless one
    // of the caller's was pending, which stays where it was (DESIGN.md §7,
    // the thread's error state).
    const bool clean = hipPeekAtLastError() == hipSuccess;
    if (hipExtGetLinkTypeAndHopCount(device, peer, &type, &hops) == hipSuccess) {
      r.link_type = (int)type;
      r.hop_count = (int)hops;
    } else if (clean) {
      (void)hipGetLastError();
    }
  }
  *out = r;
  return XEC_SUCCESS;
}

const char* xec_build_info(void) { return "xec-hip gfx950 src:" XEC_SRC_ID " " __DATE__ " " __TIME__; }

}  // extern "C"
