// xec_kernels.hip -- CDNA4 (gfx950) kernels of the XOR-EC hot path.
//
// Written for MI355X from the reference's *behaviour*
// (src/xorec/xorec.cpp:24-111: parity class i % m, single-erasure rebuild),
// not from its CUDA kernels: there are no atomics, no memset pass and no
// 8-byte grid-stride loop here (cf. xorec_gpu_cmp.cu:119-208).
//
// Work unit ("tile"): one parity class j of one stripe c over a contiguous
// column range of T*U 16-byte granules (T = threads per workgroup, 64 or 256).
// A lane owns U granules of the column range and keeps every member of the
// class in flight at once:
//   encode: NM = k/m loads  (data blocks j, j+m, ...)      -> 1 parity store
//   decode: NM loads        (class members, lost one       -> 1 store into the
//                            replaced by the class parity)     lost data block
// so each wave-instruction is a fully coalesced 1 KiB global_load_dwordx4
// from one block and each lane has NM*U independent 16-byte loads in flight.
// The XOR reduction happens in registers; no LDS is needed because no byte is
// read twice and no cross-lane exchange is needed ("Why no LDS").
//
// Addresses are formed per load as (uniform block base) + r*stride + (lane
// offset) in 64-bit VGPR arithmetic.  Keeping an array of NM uniform member
// pointers instead costs ~2*NM SGPRs; above 80 SGPRs gfx950 admits one wave
// per SIMD fewer (MI355X_MICROARCH.md, Residency), which measured -5 % here.
//
// All byte offsets are 64-bit: the batch may exceed 4 GiB (cf. the 32-bit
// indices of xorec_gpu_cmp.cu:127-131).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "xec_internal.h"
#include "xec_kernels.h"

namespace xec {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// pointer into the constant address space: uniform loads through it become
// scalar (s_load) loads served by the scalar cache
typedef const uint32_t __attribute__((address_space(4)))* const_u32_as4;
typedef const int32_t __attribute__((address_space(4)))* const_i32_as4;

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const uint8_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

template <bool NT>
__device__ __forceinline__ void st16(uint8_t* p, u32x4 v) {
  u32x4* q = reinterpret_cast<u32x4*>(p);
  if constexpr (NT) __builtin_nontemporal_store(v, q);
  else *q = v;
}

// Cache policy of the result stores of the NT kernels (gfx950 buffer aux bits:
// sc0 = 1, nt = 2, sc1 = 16).  Encode stores parity `nt`.  Decode stores the
// rebuilt block `sc1`, which does not keep the line in the XCD's L2
// (MI355X_MICROARCH.md, stores of each flavour): the rebuilt line shares its
// L2 set with the same column of the blocks the tile is reading, and an
// in-place nt line left dirty there measured 3-6 % slower (config 3, config
// 2, 16+4, 32+1 x 64 KiB on two devices; bf0ca45:tools/archive/ab/patches/store_policy.py,
// profiles/r01r, r01s); for encode sc1 was -2..+3 %, so it stays nt.
constexpr int kEncodeStoreAux = 2;   // nt
constexpr int kDecodeStoreAux = 16;  // sc1

// Store 16 bytes at block + off.  With NT the store is a buffer store whose
// cache policy is an explicit operand (AUX): hipcc (ROCm 7.2) silently drops
// the !nontemporal of __builtin_nontemporal_store in the unrolled reduction
// below (the emitted global_store has no `nt`), which measured 5 % slower.
// tests/test_isa.py checks every NT kernel's stores carry their policy.
template <bool NT, int AUX>
__device__ __forceinline__ void st16_block(uint8_t* block, uint64_t off, u32x4 v) {
  if constexpr (NT) {
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(block, 0, 0x7fffffff, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (uint32_t)off, 0, AUX);
  } else {
    st16<false>(block + off, v);
  }
}

// Decompose a tile index into (stripe c, class j, column chunk); chunks of
// one block are adjacent tile indices.
//
// kReverse note: both kernels hand workgroup b the tile total-1-b, i.e. walk
// the batch from its end.  In bench.py's encode/decode rotation that measured
// +1.1 % (encode +1.4 %, decode +0.8 %, three interleaved runs each,
// profiles/r01ae) and +2.1 / +1.2 % at config 3 in tools/ab (other shapes
// within +-0.8 %, profiles/r01ad); why is not known.
struct TileCoord {
  uint64_t c, j, chunk;
};

__device__ __forceinline__ TileCoord tile_coord(uint64_t t, const Geometry& g) {
  TileCoord tc;
  tc.chunk = t % g.tiles_per_block;
  const uint64_t cj = t / g.tiles_per_block;
  tc.j = cj % g.m;
  tc.c = cj / g.m;
  return tc;
}

// Column rotation (Geometry::rot, xec_set_rotation): stripe c's chunk q covers
// column chunk (q + c*rot) mod tiles_per_block.  A bijection on each block's
// chunks, so every byte is still read and written exactly once; it only moves
// which columns of concurrently read stripes are in flight together.  With
// one failed device -- the same shard lost in every stripe -- the stripes in
// flight read the same columns of blocks a power of two apart, which this HBM
// serves 10-20 % slower than a mix of offsets (tools/lab/read_probe.hip,
// profiles/r04b; DESIGN.md §3 *Which block is lost*).
__device__ __forceinline__ uint64_t rotated(uint64_t chunk, uint64_t c, const Geometry& g) {
  if (g.rot == 0) return chunk;
  const uint64_t q = chunk + (c * g.rot) % g.tiles_per_block;
  return q < g.tiles_per_block ? q : q - g.tiles_per_block;
}

// XOR-reduce the NM members of one class over this lane's U granules and
// store the result at dst.  Member r lives at base + r*stride, except member
// `subst`, whose bytes come from `sub` instead (decode: the class parity).
// `off` = this lane's byte offset of granule 0 in the block; granule u is
// off + u*T*16 and takes part only while inside the block (ragged tiles).
// SAUX = cache policy of the NT result store (kEncodeStoreAux / kDecodeStoreAux).
template <int NM, int U, bool NT, int T, int SAUX>
__device__ __forceinline__ void xor_members(const uint8_t* base, uint64_t stride,
                                            const uint8_t* sub, int subst, uint8_t* dst,
                                            uint64_t off, uint64_t bs, uint32_t nm_rt) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  if constexpr (NM > 0) {
    if (off + (U - 1) * kStep < bs) {  // whole tile inside the block: no predication
      u32x4 v[NM][U];
      // A running lane pointer (one 64-bit VGPR add per member) instead of NM
      // uniform member addresses, which the compiler would park in SGPRs.
      const uint8_t* p = base + off;
      const uint8_t* ps = sub + off;
#pragma unroll
      for (int r = 0; r < NM; ++r, p += stride) {
        const uint8_t* src = r == subst ? ps : p;
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(src + u * kStep);
      }
      // At 32+ members the compiler otherwise keeps a rolling window of ~11
      // loads in flight; with residency capped at one wave per SIMD
      // (xec_api.cpp auto_occupancy) all 32 in flight measured +4-6 %
      // (decode at config 4, encode at 32+1 x 64 KiB; tools/ab,
      // profiles/r01m).  At 16 members the window is faster (-2 %).
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r < NM; ++r) acc ^= v[r][u];
        st16_block<NT, SAUX>(dst, off + u * kStep, acc);
      }
      return;
    }
  }
  // Ragged tail of a block, or a member count without a compiled unroll
  // (groups of 8 loads in flight per granule).
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= bs) continue;
    u32x4 acc = {0u, 0u, 0u, 0u};
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rr = (int)(r + q);
        v[q] = ld16<NT>((rr == subst ? sub : base + (uint64_t)rr * stride) + o);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r) acc ^= ld16<NT>(((int)r == subst ? sub : base + (uint64_t)r * stride) + o);
    st16_block<NT, SAUX>(dst, o, acc);
  }
}

// ---------------------------------------------------------------------------
// encode: parity[c][j] = XOR_{r < k/m} data[c][j + r*m]      (xorec.cpp:37-57)
// ---------------------------------------------------------------------------
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void encode_kernel(const uint8_t* __restrict__ data,
                                                   uint8_t* __restrict__ parity, Geometry g) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    // tiles are walked from the end of the batch (kReverse note above)
    const uint64_t t = g.total_tiles - 1 - t0;
    const TileCoord tc = tile_coord(t, g);
    const uint8_t* base = data + (tc.c * g.k + tc.j) * g.bs;
    uint8_t* dst = parity + (tc.c * g.m + tc.j) * g.bs;
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    xor_members<NM, U, NT, T, kEncodeStoreAux>(base, g.m * g.bs, nullptr, -1, dst, off, g.bs,
                                               (uint32_t)g.nm);
  }
}

// ---------------------------------------------------------------------------
// decode: every lost data block L (at most one per class, checked on the
// host) of class j = L % m is rebuilt as
//   data[c][L] = parity[c][j] ^ XOR_{r != L/m} data[c][j + r*m]  (xorec.cpp:79-108)
// A tile is (stripe c, column chunk) -- not per class -- so a workgroup only
// exists where there may be work: it scans the stripe's k data bitmap bytes
// with scalar loads (s_load_dword through the scalar cache; 4 bytes per load,
// exact zero-byte test in SALU) and rebuilds each lost block it finds.  With
// one erasure per stripe and m > 1 this launches m times fewer workgroups than
// a per-class tiling, of which m-1 in m would only have found nothing to do.
// Absolute addresses are used for the dword loads: the caller's scratch
// pointer need not be aligned, and an aligned dword never crosses a page.
// ---------------------------------------------------------------------------
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void decode_kernel(uint8_t* data, const uint8_t* __restrict__ parity,
                                                   const uint8_t* __restrict__ bitmap, Geometry g) {
  // xec_decode_device: the check kernel ran first on this stream; a failed
  // batch is left untouched (all-or-nothing, xorec_gpu_cmp.cu:75-81).
  if (g.gate != nullptr && *(const_i32_as4)g.gate != 0) return;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m;
  const uint64_t stride = g.m * g.bs;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const uint64_t c = t / g.tiles_per_block;
    const uint64_t chunk = rotated(t % g.tiles_per_block, c, g);
    const uint64_t rowaddr = reinterpret_cast<uint64_t>(bitmap + c * (g.k + g.m));
    const uint64_t end = rowaddr + g.k;
    uint8_t* sdata = data + c * g.k * g.bs;
    const uint8_t* spar = parity + c * g.m * g.bs;
    const uint64_t off = (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
    for (uint64_t a = rowaddr & ~3ull; a < end; a += 4) {
      const uint32_t w = *(const_u32_as4)a;
      uint32_t z = ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;  // zero bytes
      if (a < rowaddr) z &= 0xFFFFFFFFu << (8 * (uint32_t)(rowaddr - a));
      if (a + 4 > end) z &= 0xFFFFFFFFu >> (8 * (uint32_t)(a + 4 - end));
      while (z) {
        const uint32_t i = (uint32_t)(a - rowaddr) + ((uint32_t)__builtin_ctz(z) >> 3);
        z &= z - 1;
        const uint32_t j = i % m, r = i / m;  // class and member of lost block i
        uint8_t* base = sdata + (uint64_t)j * g.bs;
        xor_members<NM, U, NT, T, kDecodeStoreAux>(base, stride, spar + (uint64_t)j * g.bs,
                                                   (int)r, base + (uint64_t)r * stride, off,
                                                   g.bs, nm);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// decode, class tiles: the tile is encode's (stripe c, class j, column chunk).
// The workgroup reads its class's k/m data bitmap bytes (scalar dword loads,
// bytes j, j+m, ... of the stripe's row) and, if one of them is lost -- the
// host scan guarantees at most one -- rebuilds it with one class reduction,
// the encode's exact memory shape.  Chosen by the host when (nearly) every
// class of the batch lost a block (xec_api.cpp decode_tiling): then no tile is
// idle, and no tile runs several reductions back to back as the stripe tiles
// above do, whose rebuilt-block store sits in the same vmcnt queue as the
// next reduction's loads.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sbyte(uint64_t addr) {
  const uint32_t w = *(const_u32_as4)(addr & ~3ull);
  return (w >> (8 * (uint32_t)(addr & 3))) & 0xFFu;
}

template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void decode_class_kernel(uint8_t* data,
                                                         const uint8_t* __restrict__ parity,
                                                         const uint8_t* __restrict__ bitmap,
                                                         Geometry g) {
  if (g.gate != nullptr && *(const_i32_as4)g.gate != 0) return;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint64_t stride = g.m * g.bs;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const TileCoord tc = tile_coord(t, g);
    const uint64_t row = reinterpret_cast<uint64_t>(bitmap + tc.c * (g.k + g.m)) + tc.j;
    uint32_t lost = nm;
    for (uint32_t r = 0; r < nm; ++r)
      if (sbyte(row + (uint64_t)r * g.m) == 0) { lost = r; break; }
    if (lost == nm) continue;
    uint8_t* base = data + (tc.c * g.k + tc.j) * g.bs;
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    xor_members<NM, U, NT, T, kDecodeStoreAux>(base, stride, parity + (tc.c * g.m + tc.j) * g.bs,
                                               (int)lost, base + (uint64_t)lost * stride, off,
                                               g.bs, nm);
  }
}

// ---------------------------------------------------------------------------
// decode, work-list tiles: the host scan that xec_decode runs anyway lists the
// lost data blocks (c << 8 | i, xec_internal.h xec_work_item) and copies the
// list instead of the bitmap; a tile is (list entry, 1 KiB chunk) -- one class
// reduction, encode's memory shape -- so no tile is idle and none rebuilds
// several blocks back to back, whatever the losses' spread over the stripes.
// Tile t reads its entry with one scalar load.
// ---------------------------------------------------------------------------
template <int NM, int U, bool NT, int T>
__device__ __forceinline__ void rebuild_item(uint8_t* data, const uint8_t* __restrict__ parity,
                                             uint32_t item, uint64_t chunk, const Geometry& g) {
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m;
  const uint64_t stride = g.m * g.bs;
  const uint64_t c = item >> 8;
  const uint32_t i = item & 0xFFu;
  const uint32_t j = i % m, r = i / m;  // class and member of the lost block
  uint8_t* base = data + (c * g.k + j) * g.bs;
  const uint64_t off = (rotated(chunk, c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
  xor_members<NM, U, NT, T, kDecodeStoreAux>(base, stride, parity + (c * g.m + j) * g.bs, (int)r,
                                             base + (uint64_t)r * stride, off, g.bs, nm);
}

template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void decode_list_kernel(uint8_t* data,
                                                        const uint8_t* __restrict__ parity,
                                                        const uint32_t* __restrict__ items,
                                                        Geometry g) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const uint32_t item = *(const_u32_as4)(items + t / g.tiles_per_block);
    rebuild_item<NM, U, NT, T>(data, parity, item, t % g.tiles_per_block, g);
  }
}

// The same with the list in the kernel arguments (at most CAP entries, CAP
// one of 64 / 256 / 1024, xec_kernels.h arg_items_capacity; the item is a
// scalar load from the kernarg segment): small decodes then copy nothing to
// the device (a <= 8 KiB H2D copy runs as a blit kernel of its own,
// 3.7-4.4 us, profiles/r02o, r02l).
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void decode_arglist_kernel(uint8_t* data,
                                                           const uint8_t* __restrict__ parity,
                                                           Geometry g, ArgItems<CAP> items) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    rebuild_item<NM, U, NT, T>(data, parity, items.v[t / g.tiles_per_block],
                               t % g.tiles_per_block, g);
  }
}

// Argument-mask tiles (small batches: S <= 1,024 stripes, k <= 32): the losses
// travel in the kernel arguments as one mask per stripe (bit i = data block i
// lost), so a small decode copies nothing to the device whatever its number
// of losses -- in a synchronous call the bitmap copy is a blit kernel of its
// own ahead of the decode (3.7-4.4 us, profiles/r02o), as long as the
// reference's 8 MiB kernels themselves.  Two tilings, as over the bitmap:
//  * by_class: encode's (stripe, class, chunk) tiles, as decode_class_kernel.
//    A class holds at most one lost data block (the host scan's
//    recoverability check), so the tile's block is the lowest set bit of the
//    stripe's mask within the class's positions j, j+m, j+2m, ...;
//  * otherwise (stripe, chunk) tiles, as decode_kernel: the tile rebuilds
//    every block its stripe's mask names, one class reduction after another
//    (few losses per stripe: class tiles would mostly idle).
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void decode_argmask_kernel(uint8_t* data,
                                                           const uint8_t* __restrict__ parity,
                                                           Geometry g, uint32_t by_class,
                                                           ArgItems<CAP> masks) {
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m;
  uint32_t class0 = 0;  // class 0's data positions: bits 0, m, 2m, ... (k <= 32)
  for (uint32_t r = 0; r < nm; ++r) class0 |= 1u << (r * m);
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    if (by_class) {
      const TileCoord tc = tile_coord(t, g);
      const uint32_t lost = masks.v[tc.c] & (class0 << tc.j);
      if (lost == 0) continue;
      rebuild_item<NM, U, NT, T>(data, parity,
                                 ((uint32_t)tc.c << 8) | (uint32_t)__builtin_ctz(lost), tc.chunk,
                                 g);
    } else {
      const uint64_t c = t / g.tiles_per_block, chunk = t % g.tiles_per_block;
      for (uint32_t lost = masks.v[c]; lost != 0; lost &= lost - 1)
        rebuild_item<NM, U, NT, T>(data, parity,
                                   ((uint32_t)c << 8) | (uint32_t)__builtin_ctz(lost), chunk, g);
    }
  }
}

// The same with a list the device built (xec_decode_device_list): list[0] is
// the entry count scan_list_kernel left, entries from list[1].  The host
// never sees the count, so the launch is a fixed grid (xec_api.cpp: one
// workgroup per 8 possible tiles, between what the chip holds at once and
// 131,072), walking the count's tiles in grid strides; workgroups past the
// list's end return at once.  On sparse batches that is 2-4x faster than
// decode_kernel over every stripe, and on dense ones within 1-4 % of one
// workgroup per tile (profiles/r06n); handing the tiles out in order from
// per-XCD work-queue heads instead was no better (0-31 % behind, commit
// 6f8fb1e, profiles/r02af, r02ag, r02ah), so the walk stays simple.  The gate
// is the check's verdict, as in decode_kernel.
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void decode_devlist_kernel(uint8_t* data,
                                                           const uint8_t* __restrict__ parity,
                                                           const uint32_t* __restrict__ list,
                                                           Geometry g) {
  if (*(const_i32_as4)g.gate != 0) return;
  const uint64_t total = (uint64_t)*(const_u32_as4)list * g.tiles_per_block;
  const uint32_t* entries = list + kDevListHeader;
  for (uint64_t t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
    const uint64_t t = total - 1 - t0;  // from the end of the list, as the other kernels
    const uint32_t item = *(const_u32_as4)(entries + t / g.tiles_per_block);
    rebuild_item<NM, U, NT, T>(data, parity, item, t % g.tiles_per_block, g);
  }
}

// ---------------------------------------------------------------------------
// repair (xec_repair, xec_repair_device): the recoverability rule is symmetric
// -- a class has at most one lost block among its k/m data blocks and its
// parity block -- so the lost block of a class, data or parity, is the XOR of
// the class's other k/m blocks.  A lost data block is decode's reduction
// (rebuild_item, stored sc1); a lost parity block is encode's reduction of
// that class (stored nt).  Blocks that are present are never written.
//
// Work-list tiles: an item is c << 8 | i with i in [0, k+m) (k + m <= 256);
// i >= k names parity block i - k.  The item is a scalar load, so the branch
// between the two reductions is uniform.
// ---------------------------------------------------------------------------
template <int NM, int U, bool NT, int T>
__device__ __forceinline__ void encode_class(const uint8_t* data, uint8_t* parity, uint64_t c,
                                             uint64_t j, uint64_t chunk, const Geometry& g) {
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint8_t* base = data + (c * g.k + j) * g.bs;
  uint8_t* dst = parity + (c * g.m + j) * g.bs;
  const uint64_t off = (rotated(chunk, c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
  xor_members<NM, U, NT, T, kEncodeStoreAux>(base, g.m * g.bs, nullptr, -1, dst, off, g.bs, nm);
}

template <int NM, int U, bool NT, int T>
__device__ __forceinline__ void repair_item(uint8_t* data, uint8_t* parity, uint32_t item,
                                            uint64_t chunk, const Geometry& g) {
  const uint32_t i = item & 0xFFu;
  if (i < (uint32_t)g.k)
    rebuild_item<NM, U, NT, T>(data, parity, item, chunk, g);
  else
    encode_class<NM, U, NT, T>(data, parity, item >> 8, i - (uint32_t)g.k, chunk, g);
}

template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void repair_list_kernel(uint8_t* data, uint8_t* parity,
                                                        const uint32_t* __restrict__ items,
                                                        Geometry g) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the list, as decode_list_kernel
    const uint32_t item = *(const_u32_as4)(items + t / g.tiles_per_block);
    repair_item<NM, U, NT, T>(data, parity, item, t % g.tiles_per_block, g);
  }
}

template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void repair_arglist_kernel(uint8_t* data, uint8_t* parity,
                                                           Geometry g, ArgItems<CAP> items) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    repair_item<NM, U, NT, T>(data, parity, items.v[t / g.tiles_per_block],
                              t % g.tiles_per_block, g);
  }
}

// Class tiles over a device bitmap (xec_repair_device; gated on the check's
// verdict): the workgroup reads its class's k/m data bitmap bytes and its
// parity byte (scalar dword loads, as decode_class_kernel) and does the one
// reduction the class needs, or none.  The check guarantees at most one loss
// per class, so the first zero byte found is the only one.
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void repair_class_kernel(uint8_t* data, uint8_t* parity,
                                                         const uint8_t* __restrict__ bitmap,
                                                         Geometry g) {
  if (g.gate != nullptr && *(const_i32_as4)g.gate != 0) return;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint64_t stride = g.m * g.bs;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const TileCoord tc = tile_coord(t, g);
    const uint64_t row = reinterpret_cast<uint64_t>(bitmap + tc.c * (g.k + g.m));
    if (sbyte(row + g.k + tc.j) == 0) {
      encode_class<NM, U, NT, T>(data, parity, tc.c, tc.j, tc.chunk, g);
      continue;
    }
    uint32_t lost = nm;
    for (uint32_t r = 0; r < nm; ++r)
      if (sbyte(row + tc.j + (uint64_t)r * g.m) == 0) { lost = r; break; }
    if (lost == nm) continue;
    uint8_t* base = data + (tc.c * g.k + tc.j) * g.bs;
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    xor_members<NM, U, NT, T, kDecodeStoreAux>(base, stride, parity + (tc.c * g.m + tc.j) * g.bs,
                                               (int)lost, base + (uint64_t)lost * stride, off,
                                               g.bs, nm);
  }
}

// ---------------------------------------------------------------------------
// verify (xec_verify, the scrub): encode's tile, but the class's k/m data
// blocks AND its parity block are XORed -- NM + 1 loads in flight per lane and
// granule -- and nothing is stored but the verdict: a class whose bytes agree
// reduces to zero everywhere.  reduce_members is xor_members without the store
// (member NM of the class is the parity block at `extra`); it returns the OR
// over this lane's U granules of the per-granule XOR, zero for granules past
// the block's end.  One ballot per wave, one byte store by one lane where any
// lane saw a nonzero byte; several tiles of a class may store the same 1.
// ---------------------------------------------------------------------------
template <int NM, int U, bool NT, int T>
__device__ __forceinline__ u32x4 reduce_members(const uint8_t* base, uint64_t stride,
                                                const uint8_t* extra, uint64_t off, uint64_t bs,
                                                uint32_t nm_rt) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  u32x4 any = {0u, 0u, 0u, 0u};
  if constexpr (NM > 0) {
    if (off + (U - 1) * kStep < bs) {  // whole tile inside the block: no predication
      u32x4 v[NM + 1][U];
      const uint8_t* p = base + off;
#pragma unroll
      for (int r = 0; r < NM; ++r, p += stride) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(p + u * kStep);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) v[NM][u] = ld16<NT>(extra + off + u * kStep);
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);  // as xor_members
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r <= NM; ++r) acc ^= v[r][u];
        any |= acc;
      }
      return any;
    }
  }
  // Ragged tail of a block, or a member count without a compiled unroll.
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= bs) continue;
    u32x4 acc = ld16<NT>(extra + o);
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = ld16<NT>(base + (uint64_t)(r + q) * stride + o);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r) acc ^= ld16<NT>(base + (uint64_t)r * stride + o);
    any |= acc;
  }
  return any;
}

template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void verify_kernel(const uint8_t* __restrict__ data,
                                                   const uint8_t* __restrict__ parity,
                                                   uint8_t* __restrict__ flags, Geometry g) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const TileCoord tc = tile_coord(t, g);
    const uint64_t cls = tc.c * g.m + tc.j;
    const uint8_t* base = data + (tc.c * g.k + tc.j) * g.bs;
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    const u32x4 v = reduce_members<NM, U, NT, T>(base, g.m * g.bs, parity + cls * g.bs, off, g.bs,
                                                 (uint32_t)g.nm);
    // every lane of the workgroup gets here: the tile loop is uniform
    const uint64_t bad = __ballot((v.x | v.y | v.z | v.w) != 0u);
    if (bad != 0 && (threadIdx.x & 63u) == 0) flags[cls] = 1;
  }
}

// *count += nonzero bytes of flags[0, n) (xec_verify zeroes *count first,
// stream-ordered): one atomicAdd per wave that found any.  A template (T =
// threads per workgroup) so that it is emitted with the kernels above, after
// the older ones.
template <int T>
__global__ __launch_bounds__(T) void count_flags_kernel(const uint8_t* __restrict__ flags,
                                                        uint64_t n, uint32_t* count) {
  uint32_t mine = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * T)
    mine += flags[t] != 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63u) == 0 && mine != 0) atomicAdd(count, mine);
}

// ---------------------------------------------------------------------------
// check + list (xec_decode_device_list): one thread per (stripe, class), as
// check_kernel, and a class that lost exactly one block, a data block, appends
// its work item (c << 8 | i, xec_internal.h) after the list header.  A wave
// reserves its entries with one atomicAdd on the count (ballot + popcount), so entries
// come out grouped by wave, roughly in stripe order; their order does not
// matter -- each entry is rebuilt on its own.  A recoverable batch has at most
// one entry per class, so S*m entries always fit; an unrecoverable one gates
// the decode off whatever the list holds.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_list_kernel(const uint8_t* __restrict__ bitmap,
                                                       Geometry g, int32_t* status,
                                                       uint32_t* list) {
  const uint64_t items = g.S * g.m, row = g.k + g.m;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * 256; b < items; b += (uint64_t)gridDim.x * 256) {
    const uint64_t t = b + threadIdx.x;  // the loop is uniform per workgroup: ballot sees every lane
    bool has = false;
    uint32_t entry = 0;
    if (t < items) {
      const uint64_t c = t / g.m, j = t % g.m;
      const uint8_t* r = bitmap + c * row;
      uint32_t lost = r[g.k + j] == 0, li = 0;
      for (uint64_t i = j; i < g.k; i += g.m)
        if (r[i] == 0) {
          ++lost;
          li = (uint32_t)i;
        }
      if (lost > 1) atomicOr(status, 4 /* XEC_DECODE_FAILURE */);
      has = lost == 1 && r[g.k + j] != 0;
      entry = (uint32_t)(c << 8) | li;
    }
    const uint64_t mask = __ballot(has);
    if (mask == 0) continue;
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)mask) - 1;
    uint32_t pos = 0;
    if (lane == leader) pos = atomicAdd(list, (uint32_t)__popcll(mask));
    pos = __shfl(pos, (int)leader);
    if (has) list[kDevListHeader + pos + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = entry;
  }
}

// *status = 0 and the list's count = 0 in one launch, stream-ordered before
// the scan.
__global__ void reset_status_list_kernel(int32_t* status, uint32_t* list) {
  *status = 0;
  *list = 0u;
}

// ---------------------------------------------------------------------------
// check: one thread per (stripe, class); counts the class's lost blocks among
// its k/m data bytes and its parity byte (is_recoverable, xorec_utils.hpp:160-175).
// Failure is rare, so the atomic is off the common path.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void check_kernel(const uint8_t* __restrict__ bitmap, Geometry g,
                                                    int32_t* status) {
  const uint64_t items = g.S * g.m, row = g.k + g.m;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < items;
       t += (uint64_t)gridDim.x * 256) {
    const uint64_t c = t / g.m, j = t % g.m;
    const uint8_t* r = bitmap + c * row;
    uint32_t lost = r[g.k + j] == 0;
    for (uint64_t i = j; i < g.k; i += g.m) lost += r[i] == 0;
    if (lost > 1) atomicOr(status, 4 /* XEC_DECODE_FAILURE */);
  }
}

// ---------------------------------------------------------------------------
// erase: zero every block whose bitmap byte is 0 (abstract_bm.cpp:20-39)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void erase_kernel(uint8_t* data, uint8_t* parity,
                                                    const uint8_t* __restrict__ bitmap, Geometry g) {
  const uint64_t tot = g.k + g.m;
  const uint64_t nblocks = g.S * tot;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    if (bitmap[b] != 0) continue;
    const uint64_t c = b / tot, i = b % tot;
    uint8_t* blk = i < g.k ? data + (c * g.k + i) * g.bs : parity + (c * g.m + (i - g.k)) * g.bs;
    for (uint64_t x = threadIdx.x * 16ull; x < g.bs; x += 256 * 16) st16<false>(blk + x, zero);
  }
}

// ---------------------------------------------------------------------------
// gather: the host pipeline's rebuilt small blocks into one contiguous run
// (csrc/xec_pipeline.cpp: one D2H copy instead of one per block)
// ---------------------------------------------------------------------------
template <uint32_t CAP>
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t* __restrict__ data,
                                                     uint8_t* __restrict__ out, uint64_t k,
                                                     uint64_t bs, uint32_t n, ArgItems<CAP> items) {
  for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
    const uint32_t item = items.v[g];
    const uint8_t* src = data + ((uint64_t)(item >> 8) * k + (item & 0xFFu)) * bs;
    uint8_t* dst = out + (uint64_t)g * bs;
    for (uint64_t x = threadIdx.x * 16ull; x < bs; x += 256 * 16) st16<false>(dst + x, ld16<true>(src + x));
  }
}

// ---------------------------------------------------------------------------
// fill: splitmix64 stream per stripe, state seed_base + c
// ---------------------------------------------------------------------------
// splitmix_at(seed, n): xec_kernels.h (the block digest shares it, on the
// device and on the host).
__global__ __launch_bounds__(256) void fill_kernel(uint64_t* buf, uint64_t S, uint64_t words,
                                                   uint64_t seed_base) {
  for (uint64_t c = blockIdx.y; c < S; c += gridDim.y) {
    uint64_t* row = buf + c * words;
    const uint64_t seed = seed_base + c;
    for (uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x; n < words;
         n += (uint64_t)gridDim.x * 256)
      row[n] = splitmix_at(seed, n);
  }
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
namespace {

// The first n of h_items in an ArgItems<CAP>, the rest zero (the kernel never
// reads past n; zeroed so a launch's arguments depend on the list alone).
template <uint32_t CAP>
ArgItems<CAP> arg_items(const uint32_t* h_items, uint64_t n) {
  ArgItems<CAP> a;
  std::memcpy(a.v, h_items, n * sizeof(uint32_t));
  std::memset(a.v + n, 0, (CAP - n) * sizeof(uint32_t));
  return a;
}

// g_class over bytes [offset, offset + len) of each block (read, ranged
// update, degraded write): the tiles are chunks of the RANGE, `units` items or
// classes of them, and there is no column rotation.
Geometry range_geometry(const Geometry& g_class, const LaunchShape& ls, uint64_t len,
                        uint64_t units) {
  Geometry g = g_class;
  const uint64_t tile_bytes = 16ull * (uint64_t)ls.threads * (uint64_t)ls.unroll;
  g.tiles_per_block = (len + tile_bytes - 1) / tile_bytes;
  g.total_tiles = units * g.tiles_per_block;
  g.rot = 0;
  return g;
}

}  // namespace

// Every launch_X below: its preconditions, then one with_shape (xec_dispatch.h)
// whose lambda picks the kernel by tiling and, where a list travels in the
// kernel arguments, its capacity by with_capacity.

hipError_t launch_encode(const void* d_data, void* d_parity, const Geometry& g,
                         const LaunchShape& ls, hipStream_t s) {
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    return launch_codec(encode_kernel<NM, U, NT, T>, grid, T, ls.lds_bytes, s,
                        static_cast<const uint8_t*>(d_data), static_cast<uint8_t*>(d_parity), g);
  });
}

hipError_t launch_decode(void* d_data, const void* d_parity, const uint8_t* d_bitmap,
                         const Geometry& g_class, const LaunchShape& ls, int tiling,
                         hipStream_t s, uint64_t n_items, const uint32_t* h_items) {
  // stripe tiles (stripe, chunk): decode_kernel; class tiles (stripe, class,
  // chunk) = encode's tiling: decode_class_kernel (with m == 1 the two
  // coincide and the stripe kernel runs); list tiles (entry, chunk):
  // decode_list_kernel over the n_items entries d_bitmap holds, or
  // decode_arglist_kernel over h_items (<= kArgItems) passed by value;
  // device-built list: decode_devlist_kernel over the count d_bitmap[0]
  // holds (n_items = its upper bound, which only sizes the grid); argument
  // masks: decode_argmask_kernel over class (or stripe) tiles, h_items = S
  // stripe masks.
  Geometry g = g_class;
  if (tiling == kDecodeClassTiles && g.m <= 1) tiling = kDecodeStripeTiles;
  if (tiling == kDecodeStripeTiles || tiling == kDecodeArgMaskStripeTiles)
    g.total_tiles = g.S * g.tiles_per_block;
  if (tiling == kDecodeListTiles || tiling == kDecodeArgListTiles ||
      tiling == kDecodeDevListTiles)
    g.total_tiles = n_items * g.tiles_per_block;
  if (g.total_tiles == 0) return hipSuccess;
  if (tiling == kDecodeArgListTiles && (n_items > kArgItems || h_items == nullptr))
    return hipErrorInvalidValue;
  if ((tiling == kDecodeArgMaskTiles || tiling == kDecodeArgMaskStripeTiles) &&
      (n_items != g.S || n_items > kArgItems || g.k > kArgMaskMaxK || h_items == nullptr))
    return hipErrorInvalidValue;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  uint8_t* dd = static_cast<uint8_t*>(d_data);
  const uint8_t* pp = static_cast<const uint8_t*>(d_parity);
  const uint32_t* list = reinterpret_cast<const uint32_t*>(d_bitmap);
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    switch (tiling) {
      case kDecodeDevListTiles:
        return launch_codec(decode_devlist_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp, list, g);
      case kDecodeArgListTiles:
        return with_capacity(n_items, [&](auto cap) {
          constexpr uint32_t CAP = decltype(cap)::value;
          return launch_codec(decode_arglist_kernel<NM, U, NT, T, CAP>, grid, T, lds, s, dd, pp, g,
                              arg_items<CAP>(h_items, n_items));
        });
      case kDecodeArgMaskTiles:
      case kDecodeArgMaskStripeTiles:
        return with_capacity(n_items, [&](auto cap) {
          constexpr uint32_t CAP = decltype(cap)::value;
          const uint32_t by_class = tiling == kDecodeArgMaskTiles;
          return launch_codec(decode_argmask_kernel<NM, U, NT, T, CAP>, grid, T, lds, s, dd, pp, g,
                              by_class, arg_items<CAP>(h_items, n_items));
        });
      case kDecodeListTiles:
        return launch_codec(decode_list_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp, list, g);
      case kDecodeClassTiles:
        return launch_codec(decode_class_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp, d_bitmap,
                            g);
      default:
        return launch_codec(decode_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp, d_bitmap, g);
    }
  });
}

hipError_t launch_check(const uint8_t* d_bitmap, const Geometry& g, int32_t* d_status,
                        hipStream_t s) {
  const uint32_t grid = grid_for((g.S * g.m + 255) / 256, 8192, 256);
  return launch(check_kernel, grid, 256, 0, s, d_bitmap, g, d_status);
}

hipError_t launch_scan_list(const uint8_t* d_bitmap, const Geometry& g, int32_t* d_status,
                            uint32_t* d_list, hipStream_t s) {
  const hipError_t e = launch(reset_status_list_kernel, 1, 1, 0, s, d_status, d_list);
  if (e != hipSuccess) return e;
  const uint32_t grid = grid_for((g.S * g.m + 255) / 256, 8192, 256);
  return launch(scan_list_kernel, grid, 256, 0, s, d_bitmap, g, d_status, d_list);
}

hipError_t launch_erase(void* d_data, void* d_parity, const uint8_t* d_bitmap, const Geometry& g,
                        hipStream_t s) {
  const uint64_t nblocks = g.S * (g.k + g.m);
  const uint32_t grid = grid_for(nblocks, 65536, 256);
  return launch(erase_kernel, grid, 256, 0, s, static_cast<uint8_t*>(d_data),
                static_cast<uint8_t*>(d_parity), d_bitmap, g);
}

hipError_t launch_gather(const void* d_data, void* d_out, uint64_t k, uint64_t bs,
                         const uint32_t* h_items, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > kArgItems || k == 0 || k > 256 || bs % 16 != 0 || h_items == nullptr)
    return hipErrorInvalidValue;
  const uint8_t* src = static_cast<const uint8_t*>(d_data);
  uint8_t* dst = static_cast<uint8_t*>(d_out);
  const uint32_t grid = grid_for(n, 0, 256);
  return with_capacity(n, [&](auto cap) {
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch(gather_kernel<CAP>, grid, 256, 0, s, src, dst, k, bs, (uint32_t)n,
                  arg_items<CAP>(h_items, n));
  });
}

hipError_t launch_fill(void* d_buf, uint64_t S, uint64_t words, uint64_t seed_base,
                       hipStream_t s) {
  uint64_t gx = (words + 255) / 256;
  if (gx > 1024) gx = 1024;
  const uint64_t gy = S < 65535 ? S : 65535;
  if (gx == 0 || gy == 0) return hipSuccess;
  return launch(fill_kernel, dim3((uint32_t)gx, (uint32_t)gy), 256, 0, s,
                static_cast<uint64_t*>(d_buf), S, words, seed_base);
}

// ---- repair and verify launchers ----------------------------------------
hipError_t launch_repair(void* d_data, void* d_parity, const uint8_t* d_bitmap,
                         const Geometry& g_class, const LaunchShape& ls, int tiling,
                         hipStream_t s, uint64_t n_items, const uint32_t* h_items) {
  // class tiles (stripe, class, chunk) over the bitmap: repair_class_kernel;
  // list tiles (entry, chunk): repair_list_kernel over the n_items entries
  // d_bitmap holds, or repair_arglist_kernel over h_items passed by value
  Geometry g = g_class;
  if (tiling == kRepairListTiles || tiling == kRepairArgListTiles)
    g.total_tiles = n_items * g.tiles_per_block;
  if (g.total_tiles == 0) return hipSuccess;
  if (g.k + g.m > 256 && tiling != kRepairClassTiles) return hipErrorInvalidValue;
  if (tiling == kRepairArgListTiles && (n_items > kArgItems || h_items == nullptr))
    return hipErrorInvalidValue;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  uint8_t* dd = static_cast<uint8_t*>(d_data);
  uint8_t* pp = static_cast<uint8_t*>(d_parity);
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    switch (tiling) {
      case kRepairArgListTiles:
        return with_capacity(n_items, [&](auto cap) {
          constexpr uint32_t CAP = decltype(cap)::value;
          return launch_codec(repair_arglist_kernel<NM, U, NT, T, CAP>, grid, T, lds, s, dd, pp, g,
                              arg_items<CAP>(h_items, n_items));
        });
      case kRepairListTiles:
        return launch_codec(repair_list_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp,
                            reinterpret_cast<const uint32_t*>(d_bitmap), g);
      default:
        return launch_codec(repair_class_kernel<NM, U, NT, T>, grid, T, lds, s, dd, pp, d_bitmap,
                            g);
    }
  });
}

hipError_t launch_verify(const void* d_data, const void* d_parity, uint8_t* d_flags,
                         const Geometry& g, const LaunchShape& ls, hipStream_t s) {
  if (g.total_tiles == 0) return hipSuccess;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    return launch_codec(verify_kernel<NM, U, NT, T>, grid, T, ls.lds_bytes, s,
                        static_cast<const uint8_t*>(d_data),
                        static_cast<const uint8_t*>(d_parity), d_flags, g);
  });
}

hipError_t launch_count_flags(const uint8_t* d_flags, uint64_t n, uint32_t* d_count,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = grid_for((n + 255) / 256, 1024, 256);
  return launch(count_flags_kernel<256>, grid, 256, 0, s, d_flags, n, d_count);
}

// ---------------------------------------------------------------------------
// digest and locate (xec_digest, xec_locate).  Kernels and launchers together.
//
//   digest(block) = sum over its u64 words w[n] of splitmix_at(w[n], n)  (mod 2^64)
//
// The sum is associative and commutative, so any split of a block over lanes,
// waves, workgroups and atomic adds gives the same bits.  A tile is one
// SEGMENT of one block -- kDigestSegmentBytes (xec_kernels.h), not a 1 KiB
// chunk: the workgroup walks it with 16-byte loads, each lane keeps its sum in
// registers, the workgroup reduces with shuffles and ONE lane does ONE 64-bit
// atomicAdd into the block's slot, so a 1 MiB block collects 16 adds where 1 KiB
// tiles would send 1,024 to one address (atomics run at the memory side and
// slow down ~14x when every adder hits one row, MI355X_MICROARCH.md).  The
// caller zeroes the slots first, stream-ordered.
//
// A lane keeps (n + 1) * golden as a running sum: its word index advances by
// 2 * T per step, so that is one 64-bit add, and the two 64-bit multiplies per
// word are splitmix_mix's own.
//
// Which blocks: slot b = c*(k+m) + i, the bitmap's layout.  kDigestAll: every
// block.  kDigestSelect: gate[b] != 0.  kDigestFlags: gate = xec_verify's
// flags, block i of stripe c iff gate[c*m + class of i] != 0.  The test is one
// scalar byte read per tile; a tile that fails it reads nothing else.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool digest_wanted(const uint8_t* gate, int mode, uint64_t c,
                                              uint64_t i, const Geometry& g) {
  if (mode == kDigestAll) return true;
  const uint64_t at = mode == kDigestSelect ? c * (g.k + g.m) + i
                                            : c * g.m + (i < g.k ? i % g.m : i - g.k);
  return sbyte(reinterpret_cast<uint64_t>(gate) + at) != 0;
}

// The two words of one granule; z = (n + 1) * golden of its first word.
__device__ __forceinline__ uint64_t digest_granule(u32x4 v, uint64_t z) {
  const uint64_t w0 = (uint64_t)v.x | ((uint64_t)v.y << 32);
  const uint64_t w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
  return splitmix_mix(w0 + z) + splitmix_mix(w1 + z + kSplitmixGolden);
}

// g.tiles_per_block = segments per block, g.total_tiles = S * (k+m) * that.
template <bool NT, int T>
__global__ __launch_bounds__(T) void digest_kernel(const uint8_t* __restrict__ data,
                                                   const uint8_t* __restrict__ parity,
                                                   const uint8_t* __restrict__ gate, int mode,
                                                   uint64_t* out, Geometry g) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  constexpr uint64_t kStepZ = (uint64_t)(2 * T) * kSplitmixGolden;  // 2*T words per step
  constexpr int kInFlight = 8;  // loads in flight per lane, as the generic reductions above
  __shared__ uint64_t wave_sum[T / 64];
  const uint64_t tot = g.k + g.m;
  for (uint64_t t = blockIdx.x; t < g.total_tiles; t += gridDim.x) {
    const uint64_t seg = t % g.tiles_per_block, b = t / g.tiles_per_block;
    const uint64_t c = b / tot, i = b % tot;
    if (!digest_wanted(gate, mode, c, i, g)) continue;  // uniform: scalar loads only
    const uint8_t* blk = i < g.k ? data + (c * g.k + i) * g.bs
                                 : parity + (c * g.m + (i - g.k)) * g.bs;
    const uint64_t begin = seg * kDigestSegmentBytes;
    const uint64_t end = g.bs - begin < kDigestSegmentBytes ? g.bs : begin + kDigestSegmentBytes;
    uint64_t off = begin + threadIdx.x * 16ull;
    uint64_t z = (off / 8 + 1) * kSplitmixGolden;  // (n + 1) * golden of this lane's first word
    uint64_t acc = 0;
    for (; off + (kInFlight - 1) * kStep < end; off += kInFlight * kStep, z += kInFlight * kStepZ) {
      u32x4 v[kInFlight];
#pragma unroll
      for (int q = 0; q < kInFlight; ++q) v[q] = ld16<NT>(blk + off + q * kStep);
#pragma unroll
      for (int q = 0; q < kInFlight; ++q) acc += digest_granule(v[q], z + q * kStepZ);
    }
    // Fewer than kInFlight granules left (a 4 KiB block is nothing else): every
    // load is issued before the first multiply here too.  With one load, then
    // its multiplies, then the next, config 4 ran 10-13 % slower (1862-1953
    // against 1696 us, profiles/digest/).
    if (off < end) {
      u32x4 v[kInFlight - 1];
#pragma unroll
      for (int q = 0; q < kInFlight - 1; ++q)
        if (off + q * kStep < end) v[q] = ld16<NT>(blk + off + q * kStep);
#pragma unroll
      for (int q = 0; q < kInFlight - 1; ++q)
        if (off + q * kStep < end) acc += digest_granule(v[q], z + q * kStepZ);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    if constexpr (T > 64) {  // the tile loop is uniform per workgroup: every wave gets here
      if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        acc = 0;
#pragma unroll
        for (int w = 0; w < T / 64; ++w) acc += wave_sum[w];
      }
      __syncthreads();  // wave_sum is free for the next tile
    }
    if (threadIdx.x == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(out + b), (unsigned long long)acc);
  }
}

// out[b] = 0 for every slot digest_kernel is going to add to (modes Select and
// Flags; with every block wanted the caller uses a memset).  One thread per slot.
__global__ __launch_bounds__(256) void digest_zero_kernel(const uint8_t* __restrict__ gate, int mode,
                                                         uint64_t* out, Geometry g) {
  const uint64_t tot = g.k + g.m, n = g.S * tot;
  for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (uint64_t)gridDim.x * 256) {
    const uint64_t c = b / tot, i = b % tot;
    const uint64_t at = mode == kDigestSelect ? b : c * g.m + (i < g.k ? i % g.m : i - g.k);
    if (gate[at] != 0) out[b] = 0;
  }
}

// xec_locate's verdict: bitmap[b] = 0 where block b was checked (every block,
// or gate = the flags of its class nonzero) and fresh[b] != stored[b], else 1;
// *count += the zeros written (the caller zeroes it first), one atomicAdd per
// wave that found any, as count_flags_kernel.  The grid-stride loop is uniform
// per wave only up to n, so lanes past it carry 0 into the shuffle.
__global__ __launch_bounds__(256) void locate_compare_kernel(const uint64_t* __restrict__ fresh,
                                                            const uint64_t* __restrict__ stored,
                                                            const uint8_t* __restrict__ gate,
                                                            uint8_t* __restrict__ bitmap,
                                                            uint32_t* count, Geometry g) {
  const uint64_t tot = g.k + g.m, n = g.S * tot;
  uint32_t mine = 0;
  for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (uint64_t)gridDim.x * 256) {
    const uint64_t c = b / tot, i = b % tot;
    const bool checked = gate == nullptr || gate[c * g.m + (i < g.k ? i % g.m : i - g.k)] != 0;
    const bool bad = checked && fresh[b] != stored[b];
    bitmap[b] = bad ? 0 : 1;
    mine += bad;
  }
  if (count == nullptr) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63u) == 0 && mine != 0) atomicAdd(count, mine);
}

hipError_t launch_digest(const void* d_data, const void* d_parity, const uint8_t* d_gate, int mode,
                         uint64_t* d_out, const Geometry& g_class, const LaunchShape& ls,
                         hipStream_t s) {
  Geometry g = g_class;
  g.tiles_per_block = (g.bs + kDigestSegmentBytes - 1) / kDigestSegmentBytes;
  g.total_tiles = g.S * (g.k + g.m) * g.tiles_per_block;
  if (g.total_tiles == 0) return hipSuccess;
  if (d_out == nullptr || (mode != kDigestAll && d_gate == nullptr) || mode < kDigestAll ||
      mode > kDigestFlags)
    return hipErrorInvalidValue;
  const uint8_t* dd = static_cast<const uint8_t*>(d_data);
  const uint8_t* pp = static_cast<const uint8_t*>(d_parity);
  const uint64_t slots = g.S * (g.k + g.m);
  hipError_t e = mode == kDigestAll
                     ? hipMemsetAsync(d_out, 0, slots * sizeof(uint64_t), s)
                     : launch(digest_zero_kernel, grid_for((slots + 255) / 256, 8192, 256), 256, 0,
                              s, d_gate, mode, d_out, g);
  if (e != hipSuccess) return e;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  if (ls.threads == 256)
    return ls.nt ? launch_codec(digest_kernel<true, 256>, grid, 256, lds, s, dd, pp, d_gate, mode,
                                d_out, g)
                 : launch_codec(digest_kernel<false, 256>, grid, 256, lds, s, dd, pp, d_gate, mode,
                                d_out, g);
  return ls.nt ? launch_codec(digest_kernel<true, 64>, grid, 64, lds, s, dd, pp, d_gate, mode,
                              d_out, g)
               : launch_codec(digest_kernel<false, 64>, grid, 64, lds, s, dd, pp, d_gate, mode,
                              d_out, g);
}

hipError_t launch_locate_compare(const uint64_t* d_fresh, const uint64_t* d_stored,
                                 const uint8_t* d_flags, uint8_t* d_bitmap, uint32_t* d_count,
                                 const Geometry& g, hipStream_t s) {
  const uint64_t slots = g.S * (g.k + g.m);
  if (slots == 0) return hipSuccess;
  return launch(locate_compare_kernel, grid_for((slots + 255) / 256, 1024, 256), 256, 0, s,
                d_fresh, d_stored, d_flags, d_bitmap, d_count, g);
}

// ---------------------------------------------------------------------------
// degraded read (xec_read, xec_read_device).  Kernels and launchers together.
//
// Item e = c << 8 | i (repair's packing) asks for bytes [offset, offset + len)
// of block i of stripe c, delivered at out + e*len.  A tile is (item, chunk of
// the RANGE): chunk q covers block offsets offset + q*16*T*U onwards, and
// g.tiles_per_block counts the chunks of the range, not of the block.  The
// item and its verdict -- copy, or reconstruct -- are scalar loads (kernel
// arguments, the uploaded list, or the device bitmap), so the branch is
// uniform per workgroup:
//   present: one 16-byte load and one store per granule;
//   lost:    the reduction of its class over the same range of the other k/m
//            blocks (decode's for a data block, encode's for a parity block;
//            xor_members_to, every member's loads in flight), whose result
//            goes straight to out.  The lost block itself is never read.
// data, parity and the bitmap are only read.
//
// Bounds.  The range starts and ends inside the block, so neither end is the
// block's.  Lower: a lane's first granule is offset + (q*T*U + lane)*16, never
// below offset, and the store address is formed from the item's own output
// base, out + e*len, plus the granule's distance from `offset` -- no pointer
// below out is ever formed.  Upper: xor_members_to takes offset + len as the
// end of what the tile may touch (its ragged-tail predicate), the copy path
// tests the same bound, and the NT store's buffer resource is `len` bytes long,
// so the hardware drops anything past the item's slot as well.
//
// Store policy of out (kReadStoreAux; buffer aux bits as above): sc1.  Decode's
// sc1 was chosen because the rebuilt line shares an L2 set with the blocks read
// in place; out is a separate buffer, so that argument does not carry over and
// the three policies were measured: libraries built from one tree with
// -DXEC_READ_STORE_AUX=2 / 16 / 0, tools/read_bench.py on each in turn, twice
// over (kernel times in us, both passes; profiles/read/store_aux*.json):
//   whole lost blocks, one per stripe   nt            sc1           default
//     config 2                          89.7 / 91.3   89.2 / 88.7   91.5 / 91.4
//     config 3                          681.1 / 670.5 661.6 / 650.8 683.6 / 666.7
//     config 4                          1301 / 1302   1267 / 1269   1340 / 1344
//   gather of the same blocks, present
//     config 2                          22.8 / 22.4   20.8 / 21.1   23.6 / 23.8
//     config 3                          85.4 / 85.4   76.7 / 76.6   80.5 / 79.3
//     config 4                          164.0 / 164.8 158.8 / 159.3 158.8 / 158.4
//   1,024 x 4 KiB of lost 1 MiB blocks  14.2 / 14.1   13.6 / 13.5   14.3 / 14.4
// sc1 is the fastest or tied in every row of both passes (2.7-3 % ahead of nt
// on reconstructions at configs 3 and 4, 6-10 % on the gather at 2 and 3): a
// line of out is written once and not read by this kernel, and sc1 does not
// keep it in the XCD's L2 beside the blocks still being read.
// ---------------------------------------------------------------------------
#ifndef XEC_READ_STORE_AUX
#define XEC_READ_STORE_AUX 16  // sc1
#endif
constexpr int kReadStoreAux = XEC_READ_STORE_AUX;

// xor_members (top of this file) with the store left to the caller:
// store(o, v) takes the result of the granule at block offset o, and `end` is
// the end of what the tile may touch -- here the range's end inside the block,
// which plays the part the block's size plays there (the ragged-tail
// predicate).  A copy and not a wrapper under xor_members: with xor_members
// forwarding to this, 82 to 374 of the existing encode / decode / repair
// kernels came out with other register assignments, and those kernels stay
// instruction for instruction what they were.
template <int NM, int U, bool NT, int T, typename Store>
__device__ __forceinline__ void xor_members_to(const uint8_t* base, uint64_t stride,
                                               const uint8_t* sub, int subst, uint64_t off,
                                               uint64_t end, uint32_t nm_rt, Store store) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  if constexpr (NM > 0) {
    if (off + (U - 1) * kStep < end) {  // whole tile inside the range: no predication
      u32x4 v[NM][U];
      const uint8_t* p = base + off;
      const uint8_t* ps = sub + off;
#pragma unroll
      for (int r = 0; r < NM; ++r, p += stride) {
        const uint8_t* src = r == subst ? ps : p;
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(src + u * kStep);
      }
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);  // as xor_members
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r < NM; ++r) acc ^= v[r][u];
        store(off + u * kStep, acc);
      }
      return;
    }
  }
  // Ragged tail of the range, or a member count without a compiled unroll
  // (groups of 8 loads in flight per granule).
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= end) continue;
    u32x4 acc = {0u, 0u, 0u, 0u};
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rr = (int)(r + q);
        v[q] = ld16<NT>((rr == subst ? sub : base + (uint64_t)rr * stride) + o);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r) acc ^= ld16<NT>(((int)r == subst ? sub : base + (uint64_t)r * stride) + o);
    store(o, acc);
  }
}

struct ReadRange {
  uint64_t offset, len;  // bytes, multiples of 16; offset + len <= bs
};

// 16 bytes at `rel` of the len-byte slot at `slot`.
template <bool NT>
__device__ __forceinline__ void st16_slot(uint8_t* slot, uint32_t len, uint64_t rel, u32x4 v) {
  if constexpr (NT) {
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(slot, 0, (int)len, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (uint32_t)rel, 0, kReadStoreAux);
  } else {
    st16<false>(slot + rel, v);
  }
}

template <int NM, int U, bool NT, int T>
__device__ __forceinline__ void read_tile(const uint8_t* __restrict__ data,
                                          const uint8_t* __restrict__ parity, uint8_t* out,
                                          uint64_t e, uint32_t item, bool lost, uint64_t chunk,
                                          const ReadRange& rr, const Geometry& g) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m, k = (uint32_t)g.k;
  const uint64_t c = item >> 8;
  const uint32_t i = item & 0xFFu;
  const uint64_t end = rr.offset + rr.len;
  const uint64_t off = rr.offset + (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
  uint8_t* slot = out + e * rr.len;
  const uint32_t len = (uint32_t)rr.len;
  auto store = [&](uint64_t o, u32x4 v) { st16_slot<NT>(slot, len, o - rr.offset, v); };
  if (!lost) {
    const uint8_t* blk = i < k ? data + (c * g.k + i) * g.bs : parity + (c * g.m + (i - k)) * g.bs;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (off + u * kStep < end) v[u] = ld16<NT>(blk + off + u * kStep);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (off + u * kStep < end) store(off + u * kStep, v[u]);
    return;
  }
  const uint32_t j = i < k ? i % m : i - k;  // the item's class
  const uint8_t* base = data + (c * g.k + j) * g.bs;
  if (i < k)  // a data block: the other members and the class parity, as decode
    xor_members_to<NM, U, NT, T>(base, g.m * g.bs, parity + (c * g.m + j) * g.bs, (int)(i / m), off,
                                 end, nm, store);
  else  // a parity block: every data member, as encode
    xor_members_to<NM, U, NT, T>(base, g.m * g.bs, nullptr, -1, off, end, nm, store);
}

// Bit e of the loss bits that travel with a host-checked list.
template <typename Word>
__device__ __forceinline__ bool read_lost_bit(Word word_at, uint64_t e) {
  return ((word_at(e >> 5) >> (uint32_t)(e & 31u)) & 1u) != 0;
}

// The list in device memory: n items, then the loss bits (xec_kernels.h).
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void read_list_kernel(const uint8_t* __restrict__ data,
                                                      const uint8_t* __restrict__ parity,
                                                      uint8_t* out,
                                                      const uint32_t* __restrict__ items,
                                                      ReadRange rr, Geometry g) {
  const uint32_t* bits = items + g.total_tiles / g.tiles_per_block;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the list, as decode_list_kernel
    const uint64_t e = t / g.tiles_per_block;
    const bool lost = read_lost_bit([&](uint64_t w) { return *(const_u32_as4)(bits + w); }, e);
    read_tile<NM, U, NT, T>(data, parity, out, e, *(const_u32_as4)(items + e), lost,
                            t % g.tiles_per_block, rr, g);
  }
}

// The same with items and bits in the kernel arguments (at most CAP items).
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void read_arglist_kernel(const uint8_t* __restrict__ data,
                                                         const uint8_t* __restrict__ parity,
                                                         uint8_t* out, ReadRange rr, Geometry g,
                                                         ArgItems<CAP> items,
                                                         ArgItems<CAP / 32> bits) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    const uint64_t e = t / g.tiles_per_block;
    const bool lost = read_lost_bit([&](uint64_t w) { return bits.v[w]; }, e);
    read_tile<NM, U, NT, T>(data, parity, out, e, items.v[e], lost, t % g.tiles_per_block, rr, g);
  }
}

// Items and bitmap on the device (xec_read_device; gated on read_check_kernel's
// verdict, so every item it sees is in range and servable): the verdict is the
// item's own bitmap byte, one scalar dword load.
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void read_dev_kernel(const uint8_t* __restrict__ data,
                                                     const uint8_t* __restrict__ parity,
                                                     uint8_t* out,
                                                     const uint32_t* __restrict__ items,
                                                     const uint8_t* __restrict__ bitmap,
                                                     ReadRange rr, Geometry g) {
  if (*(const_i32_as4)g.gate != 0) return;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    const uint64_t e = t / g.tiles_per_block;
    const uint32_t item = *(const_u32_as4)(items + e);
    const bool lost =
        bitmap != nullptr && sbyte(reinterpret_cast<uint64_t>(bitmap) +
                                   (uint64_t)(item >> 8) * (g.k + g.m) + (item & 0xFFu)) == 0;
    read_tile<NM, U, NT, T>(data, parity, out, e, item, lost, t % g.tiles_per_block, rr, g);
  }
}

// One thread per item: *status = max(*status, verdict), verdict 0 servable,
// 3 out of range (nothing of it is dereferenced), 4 lost with another block of
// its class lost too.  Only blocks of the item's own class are looked at.
__global__ __launch_bounds__(256) void read_check_kernel(const uint8_t* __restrict__ bitmap,
                                                        const uint32_t* __restrict__ items,
                                                        uint64_t n, Geometry g, int32_t* status) {
  const uint64_t row = g.k + g.m;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n;
       t += (uint64_t)gridDim.x * 256) {
    const uint32_t item = items[t];
    const uint64_t c = item >> 8, i = item & 0xFFu;
    if (c >= g.S || i >= row) {
      atomicMax(status, 3 /* XEC_INVALID_COUNTS */);
      continue;
    }
    if (bitmap == nullptr) continue;
    const uint8_t* r = bitmap + c * row;
    if (r[i] != 0) continue;
    const uint64_t j = i < g.k ? i % g.m : i - g.k;
    uint32_t others = i < g.k ? r[g.k + j] == 0 : 0;
    for (uint64_t l = j; l < g.k; l += g.m) others += l != i && r[l] == 0;
    if (others != 0) atomicMax(status, 4 /* XEC_DECODE_FAILURE */);
  }
}

hipError_t launch_read(const void* d_data, const void* d_parity, void* d_out,
                       const Geometry& g_class, const LaunchShape& ls, int tiling, uint64_t offset,
                       uint64_t len, uint64_t n_items, const uint32_t* d_items,
                       const uint8_t* d_bitmap, const uint32_t* h_items, const uint32_t* h_lost,
                       hipStream_t s) {
  if (n_items == 0) return hipSuccess;
  if (d_out == nullptr || len == 0 || offset % 16 != 0 || len % 16 != 0 ||
      offset + len > g_class.bs || g_class.k + g_class.m > 256 || tiling < kReadListTiles ||
      tiling > kReadDevTiles)
    return hipErrorInvalidValue;
  if (tiling == kReadArgListTiles ? (n_items > kArgItems || h_items == nullptr || h_lost == nullptr)
                                  : d_items == nullptr)
    return hipErrorInvalidValue;
  if (tiling == kReadDevTiles && g_class.gate == nullptr) return hipErrorInvalidValue;
  const Geometry g = range_geometry(g_class, ls, len, n_items);
  const ReadRange rr{offset, len};
  const uint8_t* d = static_cast<const uint8_t*>(d_data);
  const uint8_t* p = static_cast<const uint8_t*>(d_parity);
  uint8_t* out = static_cast<uint8_t*>(d_out);
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    switch (tiling) {
      case kReadArgListTiles:
        return with_capacity(n_items, [&](auto cap) {
          constexpr uint32_t CAP = decltype(cap)::value;  // and one `lost` bit per item
          return launch_codec(read_arglist_kernel<NM, U, NT, T, CAP>, grid, T, lds, s, d, p, out,
                              rr, g, arg_items<CAP>(h_items, n_items),
                              arg_items<CAP / 32>(h_lost, (n_items + 31) / 32));
        });
      case kReadListTiles:
        return launch_codec(read_list_kernel<NM, U, NT, T>, grid, T, lds, s, d, p, out, d_items,
                            rr, g);
      default:
        return launch_codec(read_dev_kernel<NM, U, NT, T>, grid, T, lds, s, d, p, out, d_items,
                            d_bitmap, rr, g);
    }
  });
}

hipError_t launch_read_check(const uint8_t* d_bitmap, const uint32_t* d_items, uint64_t n,
                             const Geometry& g, int32_t* d_status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return launch(read_check_kernel, grid_for((n + 255) / 256, 8192, 256), 256, 0, s, d_bitmap,
                d_items, n, g, d_status);
}

// ---------------------------------------------------------------------------
// vectored read (xec_readv, xec_readv_device).  Kernels and launchers together.
//
// The degraded read above with a range per entry.  Entries differ in their
// number of chunks, so a tile is no longer (t / tiles_per_block, t %
// tiles_per_block): entry e owns tiles [tile[e], tile[e + 1]), an exclusive
// prefix the host plan (xec_internal.h) or the scan kernel below wrote, and
// tile t finds e by binary search over it -- ceil(log2 n) dependent scalar
// loads from the kernel arguments, the uploaded table or d_work.  The entry,
// its range, its output start and its verdict are scalar too, so they are
// uniform per workgroup and the copy / reconstruct branch stays wave-uniform.
// The tile itself is read_tile_to: the bounds argument above read_tile holds
// per entry -- the slot is out + the entry's output start and no pointer below
// it is formed, the ragged-tail predicate uses the entry's offset + len, and
// the NT store's buffer resource is the entry's len bytes long.  st16_slot
// takes (int)len: the NT kernels run only for bs < 2^31 (launch_shape in
// xec_api.cpp), and len <= bs, so the cast never changes the value; for larger
// blocks the plain-store kernels run and len is not used at all.
// Tiles are walked from the end of the list, grid-stride, as read_list_kernel.
// ---------------------------------------------------------------------------

// read_tile with the slot as an argument.  A copy and not read_tile's body, as
// xor_members_to above: with read_tile forwarding to this, 180 of the 280 read
// kernels came out with another instruction schedule, and those kernels stay
// instruction for instruction what they were.
template <int NM, int U, bool NT, int T>
__device__ __forceinline__ void read_tile_to(const uint8_t* __restrict__ data,
                                             const uint8_t* __restrict__ parity, uint8_t* slot,
                                             uint32_t item, bool lost, uint64_t chunk,
                                             const ReadRange& rr, const Geometry& g) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m, k = (uint32_t)g.k;
  const uint64_t c = item >> 8;
  const uint32_t i = item & 0xFFu;
  const uint64_t end = rr.offset + rr.len;
  const uint64_t off = rr.offset + (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
  const uint32_t len = (uint32_t)rr.len;
  auto store = [&](uint64_t o, u32x4 v) { st16_slot<NT>(slot, len, o - rr.offset, v); };
  if (!lost) {
    const uint8_t* blk = i < k ? data + (c * g.k + i) * g.bs : parity + (c * g.m + (i - k)) * g.bs;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (off + u * kStep < end) v[u] = ld16<NT>(blk + off + u * kStep);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (off + u * kStep < end) store(off + u * kStep, v[u]);
    return;
  }
  const uint32_t j = i < k ? i % m : i - k;  // the entry's class
  const uint8_t* base = data + (c * g.k + j) * g.bs;
  if (i < k)  // a data block: the other members and the class parity, as decode
    xor_members_to<NM, U, NT, T>(base, g.m * g.bs, parity + (c * g.m + j) * g.bs, (int)(i / m), off,
                                 end, nm, store);
  else  // a parity block: every data member, as encode
    xor_members_to<NM, U, NT, T>(base, g.m * g.bs, nullptr, -1, off, end, nm, store);
}

// The entry whose tiles [tile(e), tile(e + 1)) hold t; t < tile(n), and every
// entry has at least one tile, so the prefix is strictly increasing.
template <typename TileAt>
__device__ __forceinline__ uint32_t readv_find(TileAt tile, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;  // tile(lo) <= t < tile(hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile(mid) <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// The table of xec_internal.h (xec_plan_readv) in columns of `cap` entries;
// w(x) is word x of it, a scalar load.
template <int NM, int U, bool NT, int T, typename W>
__device__ __forceinline__ void readv_table_tiles(const uint8_t* __restrict__ data,
                                                  const uint8_t* __restrict__ parity, uint8_t* out,
                                                  W w, uint32_t n, uint64_t cap,
                                                  const Geometry& g) {
  const uint32_t total = w(n);
  for (uint64_t t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
    const uint32_t t = total - 1 - (uint32_t)t0;
    const uint32_t e = readv_find(w, n, t);
    const uint64_t col = cap + 1 + e;  // the entry's word of the first column past the tiles
    const ReadRange rr{w(col + cap), w(col + 2 * cap)};
    const uint64_t start = (uint64_t)w(col + 4 * cap) << 32 | w(col + 3 * cap);
    const bool lost = ((w(6 * cap + 1 + (e >> 5)) >> (e & 31u)) & 1u) != 0;
    read_tile_to<NM, U, NT, T>(data, parity, out + start, w(col), lost, t - w(e), rr, g);
  }
}

// The table in device memory (cap = n).
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void readv_list_kernel(const uint8_t* __restrict__ data,
                                                       const uint8_t* __restrict__ parity,
                                                       uint8_t* out,
                                                       const uint32_t* __restrict__ table,
                                                       uint32_t n, Geometry g) {
  readv_table_tiles<NM, U, NT, T>(
      data, parity, out, [&](uint64_t x) { return *(const_u32_as4)(table + x); }, n, n, g);
}

// The same with the table in the kernel arguments (at most CAP entries).
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void readv_arglist_kernel(const uint8_t* __restrict__ data,
                                                          const uint8_t* __restrict__ parity,
                                                          uint8_t* out, uint32_t n, Geometry g,
                                                          ArgItems<xec_readv_table_words(CAP)> table) {
  readv_table_tiles<NM, U, NT, T>(
      data, parity, out, [&](uint64_t x) { return table.v[x]; }, n, CAP, g);
}

// Entries and bitmap on the device (xec_readv_device; gated on the verdict of
// readv_check_kernel and readv_scan_kernel, so every entry it sees is valid,
// in range and servable, and the output fits).  work = d_work (xec_kernels.h
// readv_work_words): the 64-bit output starts, then the tile starts; item,
// range and the block's bitmap byte are scalar loads.
template <int NM, int U, bool NT, int T>
__global__ __launch_bounds__(T) void readv_dev_kernel(const uint8_t* __restrict__ data,
                                                      const uint8_t* __restrict__ parity,
                                                      uint8_t* out,
                                                      const uint32_t* __restrict__ iov,
                                                      const uint8_t* __restrict__ bitmap,
                                                      const uint32_t* __restrict__ work,
                                                      uint32_t n, Geometry g) {
  if (*(const_i32_as4)g.gate != 0) return;
  const uint32_t* tiles = work + 2 * ((uint64_t)n + 1);
  auto tile = [&](uint32_t x) { return *(const_u32_as4)(tiles + x); };
  const uint32_t total = tile(n);
  for (uint64_t t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
    const uint32_t t = total - 1 - (uint32_t)t0;
    const uint32_t e = readv_find(tile, n, t);
    const uint32_t* ent = iov + 3 * (uint64_t)e;
    const uint32_t item = *(const_u32_as4)ent;
    const ReadRange rr{*(const_u32_as4)(ent + 1), *(const_u32_as4)(ent + 2)};
    const uint64_t start = (uint64_t) * (const_u32_as4)(work + 2 * (uint64_t)e + 1) << 32 |
                           *(const_u32_as4)(work + 2 * (uint64_t)e);
    const bool lost =
        bitmap != nullptr && sbyte(reinterpret_cast<uint64_t>(bitmap) +
                                   (uint64_t)(item >> 8) * (g.k + g.m) + (item & 0xFFu)) == 0;
    read_tile_to<NM, U, NT, T>(data, parity, out + start, item, lost, t - tile(e), rr, g);
  }
}

// One thread per entry: *status = max(*status, verdict), verdict 0 servable,
// 1 a range that breaks the rules (len == 0, offset or len % 16, offset + len
// > bs), 3 c >= S or i >= k + m, 4 lost with another block of its class lost
// too; an entry with a nonzero verdict is not dereferenced beyond its own 12
// bytes.  Writes the entry's length into bytes[e] and its tile count into
// tiles[e] (0 and 0 for a broken range) for readv_scan_kernel.
__global__ __launch_bounds__(256) void readv_check_kernel(const uint8_t* __restrict__ bitmap,
                                                         const uint32_t* __restrict__ iov,
                                                         uint64_t n, Geometry g,
                                                         uint64_t tile_bytes, uint64_t* bytes,
                                                         uint32_t* tiles, int32_t* status) {
  const uint64_t row = g.k + g.m;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n;
       t += (uint64_t)gridDim.x * 256) {
    const uint32_t item = iov[3 * t];
    const uint64_t offset = iov[3 * t + 1], len = iov[3 * t + 2];
    const bool range_ok = len != 0 && offset % 16 == 0 && len % 16 == 0 && offset + len <= g.bs;
    bytes[t] = range_ok ? len : 0;
    tiles[t] = range_ok ? (uint32_t)((len + tile_bytes - 1) / tile_bytes) : 0;
    const uint64_t c = item >> 8, i = item & 0xFFu;
    int32_t verdict = range_ok ? 0 : 1;
    if (c >= g.S || i >= row) {
      verdict = 3;
    } else if (range_ok && bitmap != nullptr && bitmap[c * row + i] == 0) {
      const uint8_t* r = bitmap + c * row;
      const uint64_t j = i < g.k ? i % g.m : i - g.k;
      uint32_t others = i < g.k ? r[g.k + j] == 0 : 0;
      for (uint64_t l = j; l < g.k; l += g.m) others += l != i && r[l] == 0;
      if (others != 0) verdict = 4;
    }
    if (verdict != 0) atomicMax(status, verdict);
  }
}

// bytes[0, n) and tiles[0, n) into their exclusive prefixes in list order, in
// place, the totals at [n]; *status raised to 1 if the byte total exceeds
// out_bytes.  One workgroup walks the list in passes of 256 entries: a wave
// scan by lane shifts, the four wave totals through LDS, and the running sums
// carried from pass to pass -- integer sums, so exact and the same whatever
// the launch.  The tile counts cannot overflow 32 bits (xec_readv_device's
// host check over n * ceil(bs / 1024)).  n / 256 dependent passes of one load,
// one scan and one store: at n = 2^20 (4,096 passes) the check and this scan
// together took at most 3.2 ms of a 4.0 ms xec_readv_device call whose read
// kernel ran 0.75 ms (16-byte entries, tools/readv_bench.py --scan), under
// 0.8 us a pass; at the 1,024 entries of a request queue it is four passes.
__global__ __launch_bounds__(256) void readv_scan_kernel(uint64_t* bytes, uint32_t* tiles,
                                                        uint64_t n, uint64_t out_bytes,
                                                        int32_t* status) {
  __shared__ unsigned long long wave_bytes[4];
  __shared__ uint32_t wave_tiles[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry_bytes = 0;
  uint32_t carry_tiles = 0;
  for (uint64_t base = 0; base < n; base += 256) {
    const uint64_t e = base + threadIdx.x;
    const unsigned long long b = e < n ? bytes[e] : 0;
    const uint32_t q = e < n ? tiles[e] : 0;
    unsigned long long sb = b;  // inclusive over the wave
    uint32_t sq = q;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long ub = __shfl_up(sb, d, 64);
      const uint32_t uq = __shfl_up(sq, d, 64);
      if (lane >= d) {
        sb += ub;
        sq += uq;
      }
    }
    if (lane == 63) {
      wave_bytes[wave] = sb;
      wave_tiles[wave] = sq;
    }
    __syncthreads();
    unsigned long long before_bytes = carry_bytes;
    uint32_t before_tiles = carry_tiles;
    for (uint32_t v = 0; v < 4; ++v) {
      if (v < wave) {
        before_bytes += wave_bytes[v];
        before_tiles += wave_tiles[v];
      }
      carry_bytes += wave_bytes[v];
      carry_tiles += wave_tiles[v];
    }
    if (e < n) {
      bytes[e] = before_bytes + sb - b;
      tiles[e] = before_tiles + sq - q;
    }
    __syncthreads();  // the wave totals are free for the next pass
  }
  if (threadIdx.x == 0) {
    bytes[n] = carry_bytes;
    tiles[n] = carry_tiles;
    if (carry_bytes > out_bytes) atomicMax(status, 1 /* XEC_INVALID_SIZE */);
  }
}

hipError_t launch_readv(const void* d_data, const void* d_parity, void* d_out, const Geometry& g,
                        const LaunchShape& ls, int tiling, uint64_t n, uint64_t tiles,
                        const uint32_t* d_table, const uint32_t* h_table, hipStream_t s,
                        const uint8_t* d_bitmap, const uint32_t* d_work) {
  if (n == 0) return hipSuccess;
  if (d_out == nullptr || n > 0xFFFFFFFFull || tiles > 0xFFFFFFFFull || g.k + g.m > 256 ||
      tiling < kReadListTiles || tiling > kReadDevTiles)
    return hipErrorInvalidValue;
  if (tiling == kReadArgListTiles ? (n > kReadvArgEntries || h_table == nullptr)
                                  : d_table == nullptr)
    return hipErrorInvalidValue;
  if (tiling == kReadDevTiles && (g.gate == nullptr || d_work == nullptr))
    return hipErrorInvalidValue;
  const uint8_t* d = static_cast<const uint8_t*>(d_data);
  const uint8_t* p = static_cast<const uint8_t*>(d_parity);
  uint8_t* out = static_cast<uint8_t*>(d_out);
  const uint32_t grid = grid_for(tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  const uint32_t n32 = (uint32_t)n;
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    switch (tiling) {
      case kReadArgListTiles:
        return with_readv_capacity(n, [&](auto cap) {
          constexpr uint32_t CAP = decltype(cap)::value;  // h_table is laid out for cap = CAP
          return launch_codec(readv_arglist_kernel<NM, U, NT, T, CAP>, grid, T, lds, s, d, p, out,
                              n32, g,
                              arg_items<xec_readv_table_words(CAP)>(h_table, xec_readv_table_words(CAP)));
        });
      case kReadListTiles:
        return launch_codec(readv_list_kernel<NM, U, NT, T>, grid, T, lds, s, d, p, out, d_table,
                            n32, g);
      default:
        return launch_codec(readv_dev_kernel<NM, U, NT, T>, grid, T, lds, s, d, p, out, d_table,
                            d_bitmap, d_work, n32, g);
    }
  });
}

hipError_t launch_readv_check(const uint8_t* d_bitmap, const uint32_t* d_iov, uint64_t n,
                              const Geometry& g, uint64_t tile_bytes, uint32_t* d_work,
                              int32_t* d_status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return launch(readv_check_kernel, grid_for((n + 255) / 256, 8192, 256), 256, 0, s, d_bitmap,
                d_iov, n, g, tile_bytes, reinterpret_cast<uint64_t*>(d_work),
                d_work + 2 * (n + 1), d_status);
}

hipError_t launch_readv_scan(uint32_t* d_work, uint64_t n, uint64_t out_bytes, int32_t* d_status,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  return launch(readv_scan_kernel, 1, 256, 0, s, reinterpret_cast<uint64_t*>(d_work),
                d_work + 2 * (n + 1), n, out_bytes, d_status);
}

// ---------------------------------------------------------------------------
// update and ranged update (xec_update, xec_update_device, xec_update_range,
// xec_update_range_device).  Kernels and launcher together.
//
// update: data block i of stripe c is replaced by a new block and the class
// parity follows by the delta,
//   parity[c][i % m] ^= data[c][i] ^ new;   data[c][i] = new
// -- 3 block reads and 2 block writes per block, whatever k/m is.
//
// One writer per parity granule: a tile owns (stripe c, class j, column chunk)
// for the whole call and folds EVERY updated member of that class,
//   acc = parity;  per member: acc ^= old ^ new, data <- new;  parity <- acc
// so there are no atomics, no memset pass and no LDS.  The loads in flight per
// lane are 2 per member and the parity, independent of k/m: no NM parameter.
//
// In place: a lane stores the new data granule to the very address it loaded
// the old one from, and the parity granule likewise; a granule belongs to one
// lane of one tile, so program order within the lane is all that is relied on.
// The new data block is stored sc1, as decode stores a rebuilt block.  The
// parity block is stored nt, as encode stores parity: both were started from
// sc1, and against that a build with nt here measured 15.7 % faster at config
// 3 (185.8 against 220.4 us for one block per stripe, encode's spread
// 1.4-2.0 %), 6.8 % at config 4 and equal at config 2 (tools/update_bench.py,
// DESIGN.md §3 *Update*, profiles/update/parity_store_*.json; taken on the
// whole-block kernels these replaced, which stored the same way).
//
// ranged update: the same over bytes [offset, offset + len) of each named
// block only,
//   parity[c][i % m][range] ^= data[c][i][range] ^ new;   data[c][i][range] = new
// with the read's range addressing: a tile is (list position or class, chunk
// of the RANGE), chunk q covers block offsets offset + q*16*T*U onwards and
// g.tiles_per_block counts the chunks of the range.  A lane's granule is never
// formed below `offset` and takes part only while below offset + len.  The
// first item of a class in its stripe owns that class's parity chunk and folds
// the later ones, one lane owns a granule, and both stores go in place through
// st16_block (data sc1, parity nt).  There is no column rotation.
//
// The whole-block entry points run these kernels with offset = 0, len = bs and
// no digests (DIG = false): the tiles are then make_geometry's, and item e's
// new block is at fresh + e*bs.  They had kernels of their own once, the same
// fold without a range; DESIGN.md §3 *Update* records the comparison.
//
// New bytes.  List forms: item e's len bytes are packed at fresh + e*len, so a
// granule at block offset o is read from fresh + e*len + (o - offset).  Class
// form: fresh mirrors data, the granule comes from the same in-block address.
//
// DIG = true keeps the stored digests current in the same pass (xec_digest's
// slots, c*(k+m) + i).  digest(block) is a sum of per-word terms, so a write
// of some words changes it by sum(mix(new)) - sum(mix(old)) over those words,
// and the tile holds both sides in registers:
//   data slot    += mix(new granule) - mix(old granule), per folded member;
//   parity slot  += mix(parity after) - mix(parity before); the `before` term
//                   is subtracted when the parity is loaded, so no second copy
//                   of it stays in registers.
// Each lane sums over its granules (word index n = in-block byte address / 8),
// a wave reduces with shuffles and ONE lane per wave does ONE 64-bit atomicAdd
// into the slot (none when the wave's sum is 0, e.g. a write of equal bytes):
// ceil(len / (16*T*U)) * T/64 adds per slot, i.e. one per KiB of the range at
// the default shape.  The sum is modulo 2^64, so the order of tiles does not
// matter.  DIG = false is a separate instantiation with no multiply and no
// atomic in it.
// ---------------------------------------------------------------------------
constexpr int kPatchDataStoreAux = 16;   // sc1
constexpr int kPatchParityStoreAux = 2;  // nt

// One wave's sum of x goes to *slot.  Called from wave-uniform control flow.
__device__ __forceinline__ void patch_wave_add(uint64_t* slot, uint64_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  if ((threadIdx.x & 63u) == 0 && x != 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)x);
}

// Digest terms of this lane's active granules; z = (n + 1) * golden of the
// first word of granule 0, granule u is 2*T words on.
template <int U, int T>
__device__ __forceinline__ uint64_t patch_mix(const u32x4 (&v)[U], uint64_t off, uint64_t end,
                                              uint64_t z) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  constexpr uint64_t kStepZ = (uint64_t)(2 * T) * kSplitmixGolden;
  uint64_t s = 0;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) s += digest_granule(v[u], z + u * kStepZ);
  return s;
}

// acc ^= old ^ new over this lane's granules of the range of one data block,
// which takes the new bytes; `fr` = the new bytes of this lane's granule 0.
// Returns mix(new) - mix(old) over them (DIG), else 0.
template <int U, bool NT, int T, bool DIG>
__device__ __forceinline__ uint64_t patch_fold(u32x4 (&acc)[U], uint8_t* block, const uint8_t* fr,
                                               uint64_t off, uint64_t end, uint64_t z) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  u32x4 o[U], n[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) o[u] = ld16<NT>(block + off + u * kStep);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) n[u] = ld16<NT>(fr + u * kStep);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) acc[u] ^= o[u] ^ n[u];
  uint64_t d = 0;
  if constexpr (DIG) d = patch_mix<U, T>(n, off, end, z) - patch_mix<U, T>(o, off, end, z);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) st16_block<NT, kPatchDataStoreAux>(block, off + u * kStep, n[u]);
  return d;
}

// List tiles: one per (list position e, chunk of the range); item e is
// c << 8 | i (i < k).  The host checked the list strictly ascending, so a
// stripe's items are adjacent: tile e owns its class's parity chunk iff no
// earlier item of its stripe is of the same class, and then folds every later
// one of that class too; otherwise it has nothing to do.  `at(q)` reads item q
// with a scalar load.
template <int U, bool NT, int T, bool DIG, typename At>
__device__ __forceinline__ void patch_list_tile(uint8_t* data, uint8_t* parity,
                                                const uint8_t* __restrict__ fresh,
                                                uint64_t* digests, uint64_t e, uint64_t n,
                                                uint64_t chunk, const ReadRange& rr,
                                                const Geometry& g, At at) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t m = (uint32_t)g.m;
  const uint32_t item = at(e);
  const uint32_t c = item >> 8, j = (item & 0xFFu) % m;
  for (uint64_t q = e; q > 0;) {
    const uint32_t prev = at(--q);
    if ((prev >> 8) != c) break;
    if ((prev & 0xFFu) % m == j) return;  // an earlier item's tile folds this one
  }
  const uint64_t end = rr.offset + rr.len;
  const uint64_t rel = (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;  // from the range's start
  const uint64_t off = rr.offset + rel;
  const uint64_t z = (off / 8 + 1) * kSplitmixGolden;
  uint8_t* par = parity + ((uint64_t)c * g.m + j) * g.bs;
  uint64_t* row = digests + (uint64_t)c * (g.k + g.m);
  u32x4 acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) acc[u] = ld16<NT>(par + off + u * kStep);
  uint64_t psum = 0;
  if constexpr (DIG) psum = 0 - patch_mix<U, T>(acc, off, end, z);
  uint32_t it = item;
  for (uint64_t q = e;;) {
    const uint32_t i = it & 0xFFu;
    if (i % m == j) {
      const uint64_t d = patch_fold<U, NT, T, DIG>(acc, data + ((uint64_t)c * g.k + i) * g.bs,
                                                   fresh + q * rr.len + rel, off, end, z);
      if constexpr (DIG) patch_wave_add(row + i, d);
    }
    if (++q == n) break;
    it = at(q);
    if ((it >> 8) != c) break;
  }
  if constexpr (DIG) psum += patch_mix<U, T>(acc, off, end, z);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (off + u * kStep < end) st16_block<NT, kPatchParityStoreAux>(par, off + u * kStep, acc[u]);
  if constexpr (DIG) patch_wave_add(row + g.k + j, psum);
}

template <int U, bool NT, int T, bool DIG>
__global__ __launch_bounds__(T) void patch_list_kernel(uint8_t* data, uint8_t* parity,
                                                       const uint8_t* __restrict__ fresh,
                                                       const uint32_t* __restrict__ items,
                                                       uint64_t* digests, ReadRange rr,
                                                       Geometry g) {
  const uint64_t n = g.total_tiles / g.tiles_per_block;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the list, as decode_list_kernel
    patch_list_tile<U, NT, T, DIG>(data, parity, fresh, digests, t / g.tiles_per_block, n,
                                   t % g.tiles_per_block, rr, g,
                                   [&](uint64_t q) { return *(const_u32_as4)(items + q); });
  }
}

template <int U, bool NT, int T, bool DIG, uint32_t CAP>
__global__ __launch_bounds__(T) void patch_arglist_kernel(uint8_t* data, uint8_t* parity,
                                                          const uint8_t* __restrict__ fresh,
                                                          uint64_t* digests, ReadRange rr,
                                                          Geometry g, ArgItems<CAP> items) {
  const uint64_t n = g.total_tiles / g.tiles_per_block;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    patch_list_tile<U, NT, T, DIG>(data, parity, fresh, digests, t / g.tiles_per_block, n,
                                   t % g.tiles_per_block, rr, g,
                                   [&](uint64_t q) { return items.v[q]; });
  }
}

// Class tiles over a device mask (xec_update_device, xec_update_range_device):
// (stripe, class, chunk of the range); mask[c*k + i] != 0 means "take block i
// of stripe c from the shadow buffer", which mirrors data's layout.  The tile
// scans its class's k/m mask bytes (scalar dword loads, as repair_class_kernel)
// and folds the marked members; a class with none reads and writes nothing.
template <int U, bool NT, int T, bool DIG>
__global__ __launch_bounds__(T) void patch_class_kernel(uint8_t* data, uint8_t* parity,
                                                        const uint8_t* __restrict__ fresh,
                                                        const uint8_t* __restrict__ mask,
                                                        uint64_t* digests, ReadRange rr,
                                                        Geometry g) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t nm = (uint32_t)g.nm;
  const uint64_t stride = g.m * g.bs;
  const uint64_t end = rr.offset + rr.len;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const TileCoord tc = tile_coord(t, g);
    const uint64_t mrow = reinterpret_cast<uint64_t>(mask + tc.c * g.k) + tc.j;
    const uint64_t first = (tc.c * g.k + tc.j) * g.bs;
    const uint64_t off = rr.offset + (tc.chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
    const uint64_t z = (off / 8 + 1) * kSplitmixGolden;
    uint8_t* par = parity + (tc.c * g.m + tc.j) * g.bs;
    uint64_t* row = digests + tc.c * (g.k + g.m);
    u32x4 acc[U];
    uint64_t psum = 0;
    bool any = false;
    for (uint32_t r = 0; r < nm; ++r) {
      if (sbyte(mrow + (uint64_t)r * g.m) == 0) continue;
      if (!any) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (off + u * kStep < end) acc[u] = ld16<NT>(par + off + u * kStep);
        if constexpr (DIG) psum = 0 - patch_mix<U, T>(acc, off, end, z);
      }
      any = true;
      const uint64_t d = patch_fold<U, NT, T, DIG>(acc, data + first + r * stride,
                                                   fresh + first + r * stride + off, off, end, z);
      if constexpr (DIG) patch_wave_add(row + tc.j + (uint64_t)r * g.m, d);
    }
    if (!any) continue;
    if constexpr (DIG) psum += patch_mix<U, T>(acc, off, end, z);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (off + u * kStep < end) st16_block<NT, kPatchParityStoreAux>(par, off + u * kStep, acc[u]);
    if constexpr (DIG) patch_wave_add(row + g.k + tc.j, psum);
  }
}

hipError_t launch_update_range(void* d_data, void* d_parity, const void* d_new, const void* d_sel,
                               uint64_t* d_digests, const Geometry& g_class, const LaunchShape& ls,
                               int tiling, uint64_t offset, uint64_t len, hipStream_t s,
                               uint64_t n_items, const uint32_t* h_items) {
  if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset + len > g_class.bs ||
      tiling < kUpdateClassTiles || tiling > kUpdateArgListTiles)
    return hipErrorInvalidValue;
  const Geometry g = range_geometry(
      g_class, ls, len, tiling == kUpdateClassTiles ? g_class.S * g_class.m : n_items);
  if (g.total_tiles == 0) return hipSuccess;
  if (g.k > 256 && tiling != kUpdateClassTiles) return hipErrorInvalidValue;
  if (tiling == kUpdateArgListTiles && (n_items > kArgItems || h_items == nullptr))
    return hipErrorInvalidValue;
  if (tiling != kUpdateArgListTiles && d_sel == nullptr) return hipErrorInvalidValue;
  const ReadRange rr{offset, len};
  uint8_t* d = static_cast<uint8_t*>(d_data);
  uint8_t* p = static_cast<uint8_t*>(d_parity);
  const uint8_t* f = static_cast<const uint8_t*>(d_new);
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  return with_shape(ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    return with_bool(d_digests != nullptr, [&](auto dig) {
      constexpr bool DIG = decltype(dig)::value;
      switch (tiling) {
        case kUpdateArgListTiles:
          return with_capacity(n_items, [&](auto cap) {
            constexpr uint32_t CAP = decltype(cap)::value;
            return launch_codec(patch_arglist_kernel<U, NT, T, DIG, CAP>, grid, T, lds, s, d, p, f,
                                d_digests, rr, g, arg_items<CAP>(h_items, n_items));
          });
        case kUpdateListTiles:
          return launch_codec(patch_list_kernel<U, NT, T, DIG>, grid, T, lds, s, d, p, f,
                              static_cast<const uint32_t*>(d_sel), d_digests, rr, g);
        default:
          return launch_codec(patch_class_kernel<U, NT, T, DIG>, grid, T, lds, s, d, p, f,
                              static_cast<const uint8_t*>(d_sel), d_digests, rr, g);
      }
    });
  });
}

// ---------------------------------------------------------------------------
// degraded write (xec_write, xec_write_device).  Kernels and launchers
// together; they stand beside patch_* and share only its lane helpers
// (patch_fold, patch_mix, patch_wave_add), so the patch kernels stay what they
// were.
//
// The ranged update above under a loss bitmap: a lost block is never read and
// never written.  Tiles, range addressing, ownership (the first item of a
// (stripe, class) owns the class's parity granules and folds every item of the
// class) and store policies (new data sc1, parity nt) are the ranged update's.
// The owning tile picks one of three modes for its class from scalar state --
// the two loss bits that travel with each item of a host-checked list, or the
// class's mask and bitmap bytes in the device form -- so the branch is uniform
// per workgroup:
//   delta      parity present, no written member lost: patch_list_tile's body.
//              A lost member that is not written is not touched.
//   data-only  parity lost: each written (present) member takes its new bytes,
//              parity is neither read nor written.  The old bytes are read only
//              with DIG.
//   rebuild    one written member x lost, every other block present:
//                parity[range] = XOR over all members r of
//                                (new_r if r is written else data_r)[range]
//              -- x's term is new_x, so every member has a source and x itself
//              is never addressed.  Present written members take their new
//              bytes from the registers the reduction loaded.  The member count
//              is a run-time loop, 8 loads in flight per granule (the ragged
//              path of xor_members_to): no member-count template parameter.
//              Old parity is read only with DIG.
// Which members are written: the list is ascending, so walking members 0..nm-1
// beside the list is a merge (ListWritten); the class form reads the mask byte.
//
// DIG in the rebuild mode.  Present written member: += mix(new) - mix(old), as
// data-only.  Parity: += mix(P_new) - mix(P_old).  Lost member x: its slot held
// the digest of the bytes it virtually holds, P_old ^ XOR_{r != x} old_r, so it
// gets += mix(new_x) - mix(P_old ^ XOR_{r != x} old_r).
//
// Bounds are the ranged update's: no granule below `offset` is formed, a
// granule takes part only while below offset + len, item e's new bytes are
// read inside [fresh + e*len, fresh + (e+1)*len).
// ---------------------------------------------------------------------------
constexpr int kWriteDelta = 0;
constexpr int kWriteDataOnly = 1;
constexpr int kWriteRebuild = 2;

// Where a tile stands in its block, shared by the three modes.
struct WriteLane {
  uint64_t off, end, z;  // first granule's block offset, the range's end, digest z of `off`
};

// A present written block takes its new bytes; with DIG the old ones are read
// as well and mix(new) - mix(old) is returned (else 0).
template <int U, bool NT, int T, bool DIG>
__device__ __forceinline__ uint64_t write_plain(uint8_t* block, const uint8_t* fr,
                                                const WriteLane& w) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  u32x4 n[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (w.off + u * kStep < w.end) n[u] = ld16<NT>(fr + u * kStep);
  uint64_t d = 0;
  if constexpr (DIG) {
    u32x4 o[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (w.off + u * kStep < w.end) o[u] = ld16<NT>(block + w.off + u * kStep);
    d = patch_mix<U, T>(n, w.off, w.end, w.z) - patch_mix<U, T>(o, w.off, w.end, w.z);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (w.off + u * kStep < w.end)
      st16_block<NT, kPatchDataStoreAux>(block, w.off + u * kStep, n[u]);
  return d;
}

// One class of one stripe over this lane's granules.  `src` answers which
// members are written and where this lane's first granule of their new bytes
// is: src.each(f) calls f(i, fr) for every written member in ascending order
// (i = its block index in the stripe); src.written(r, fr), called with r
// ascending from 0, says whether member r (block j + r*m) is written.
// `x` = the lost written member's block index (rebuild only).
template <int U, bool NT, int T, bool DIG, typename Src>
__device__ __forceinline__ void write_tile(uint8_t* data, uint8_t* parity, uint64_t* digests,
                                           int mode, uint64_t c, uint32_t j, uint32_t x,
                                           const WriteLane& w, const Geometry& g, Src src) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  uint8_t* par = parity + (c * g.m + j) * g.bs;
  uint8_t* blocks = data + c * g.k * g.bs;  // the stripe's data blocks
  uint64_t* row = digests + c * (g.k + g.m);
  if (mode == kWriteDataOnly) {
    src.each([&](uint32_t i, const uint8_t* fr) {
      const uint64_t d = write_plain<U, NT, T, DIG>(blocks + (uint64_t)i * g.bs, fr, w);
      if constexpr (DIG) patch_wave_add(row + i, d);
    });
    return;
  }
  u32x4 acc[U];
  uint64_t psum = 0;
  if (mode == kWriteDelta) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (w.off + u * kStep < w.end) acc[u] = ld16<NT>(par + w.off + u * kStep);
    if constexpr (DIG) psum = 0 - patch_mix<U, T>(acc, w.off, w.end, w.z);
    src.each([&](uint32_t i, const uint8_t* fr) {
      const uint64_t d = patch_fold<U, NT, T, DIG>(acc, blocks + (uint64_t)i * g.bs, fr, w.off,
                                                   w.end, w.z);
      if constexpr (DIG) patch_wave_add(row + i, d);
    });
  } else {
    // rebuild: every member has a source; acc becomes the new parity
    const uint32_t nm = (uint32_t)g.nm, m = (uint32_t)g.m;
    u32x4 oldx[U];  // DIG: XOR of the old bytes of every member but x
    uint64_t dx = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[u] = u32x4{0u, 0u, 0u, 0u};
      oldx[u] = u32x4{0u, 0u, 0u, 0u};
    }
    // member block i with its bytes v loaded from `written ? new : data`
    auto absorb = [&](uint32_t i, bool written, const u32x4(&v)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) acc[u] ^= v[u];
      if (!written) {
        if constexpr (DIG) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (w.off + u * kStep < w.end) oldx[u] ^= v[u];
        }
        return;
      }
      if (i == x) {  // the lost member: its new bytes went into the parity only
        if constexpr (DIG) dx = patch_mix<U, T>(v, w.off, w.end, w.z);
        return;
      }
      uint8_t* block = blocks + (uint64_t)i * g.bs;
      if constexpr (DIG) {
        u32x4 o[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (w.off + u * kStep < w.end) {
            o[u] = ld16<NT>(block + w.off + u * kStep);
            oldx[u] ^= o[u];
          }
        patch_wave_add(row + i, patch_mix<U, T>(v, w.off, w.end, w.z) -
                                    patch_mix<U, T>(o, w.off, w.end, w.z));
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end)
          st16_block<NT, kPatchDataStoreAux>(block, w.off + u * kStep, v[u]);
    };
    uint32_t r = 0;
    // 8 members' loads in flight per granule.  Not with DIG: the 8 granules held
    // beside the digest arithmetic took the instantiation to 111 VGPRs, and the
    // delta mode of the same kernel -- every write of a healthy store -- ran
    // 1.4x xec_update_range's time at 4 waves per SIMD.
    for (; !DIG && r + 8 <= nm; r += 8) {
      const uint8_t* from[8];
      bool wr[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint32_t i = j + (r + q) * m;
        const uint8_t* fr = nullptr;
        wr[q] = src.written(r + q, fr);
        from[q] = wr[q] ? fr : blocks + (uint64_t)i * g.bs + w.off;
      }
      u32x4 v[8][U];
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (w.off + u * kStep < w.end) v[q][u] = ld16<NT>(from[q] + u * kStep);
#pragma unroll
      for (int q = 0; q < 8; ++q) absorb(j + (r + q) * m, wr[q], v[q]);
    }
    for (; r < nm; ++r) {
      const uint32_t i = j + r * m;
      const uint8_t* fr = nullptr;
      const bool wr = src.written(r, fr);
      const uint8_t* from = wr ? fr : blocks + (uint64_t)i * g.bs + w.off;
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) v[u] = ld16<NT>(from + u * kStep);
      absorb(i, wr, v);
    }
    if constexpr (DIG) {
      u32x4 pold[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) {
          pold[u] = ld16<NT>(par + w.off + u * kStep);
          oldx[u] ^= pold[u];  // what block x virtually held
        }
      psum = 0 - patch_mix<U, T>(pold, w.off, w.end, w.z);
      patch_wave_add(row + x, dx - patch_mix<U, T>(oldx, w.off, w.end, w.z));
    }
  }
  if constexpr (DIG) psum += patch_mix<U, T>(acc, w.off, w.end, w.z);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (w.off + u * kStep < w.end)
      st16_block<NT, kPatchParityStoreAux>(par, w.off + u * kStep, acc[u]);
  if constexpr (DIG) patch_wave_add(row + g.k + j, psum);
}

// The written members of class j of stripe c as the ascending list names them,
// from list position q on; item t's new bytes are at fresh + t*len.
template <typename At>
struct ListWritten {
  At at;
  uint64_t q, n;
  uint32_t c, j, m;
  const uint8_t* fresh;  // + rel: this lane's first granule of item 0
  uint64_t len;

  template <typename F>
  __device__ __forceinline__ void each(F f) {
    for (uint64_t t = q; t < n; ++t) {
      const uint32_t it = at(t);
      if ((it >> 8) != c) break;
      const uint32_t i = it & 0xFFu;
      if (i % m == j) f(i, fresh + t * len);
    }
  }
  // a merge: members and list both ascend
  __device__ __forceinline__ bool written(uint32_t r, const uint8_t*& fr) {
    const uint32_t want = j + r * m;
    while (q < n) {
      const uint32_t it = at(q);
      if ((it >> 8) != c || (it & 0xFFu) >= want) break;
      ++q;
    }
    if (q >= n) return false;
    const uint32_t it = at(q);
    if ((it >> 8) != c || (it & 0xFFu) != want) return false;
    fr = fresh + q * len;
    ++q;
    return true;
  }
};

// The two loss bits of list position t: bit 0 = this block is lost, bit 1 =
// this class's parity block is lost (16 items per word).
template <typename Word>
__device__ __forceinline__ uint32_t write_bits(Word word_at, uint64_t t) {
  return (word_at(t >> 4) >> (2u * (uint32_t)(t & 15u))) & 3u;
}

// List tiles: one per (list position e, chunk of the range), ownership as
// patch_list_tile; the owner reads the mode off the bits of its class's items.
template <int U, bool NT, int T, bool DIG, typename At, typename Word>
__device__ __forceinline__ void write_list_tile(uint8_t* data, uint8_t* parity,
                                                const uint8_t* __restrict__ fresh,
                                                uint64_t* digests, uint64_t e, uint64_t n,
                                                uint64_t chunk, const ReadRange& rr,
                                                const Geometry& g, At at, Word word_at) {
  const uint32_t m = (uint32_t)g.m;
  const uint32_t item = at(e);
  const uint32_t c = item >> 8, j = (item & 0xFFu) % m;
  for (uint64_t q = e; q > 0;) {
    const uint32_t prev = at(--q);
    if ((prev >> 8) != c) break;
    if ((prev & 0xFFu) % m == j) return;  // an earlier item's tile handles this one
  }
  uint32_t any = 0, x = 0;
  for (uint64_t q = e; q < n; ++q) {
    const uint32_t it = at(q);
    if ((it >> 8) != c) break;
    if ((it & 0xFFu) % m != j) continue;
    const uint32_t b = write_bits(word_at, q);
    any |= b;
    if (b & 1u) x = it & 0xFFu;
  }
  const int mode = (any & 2u) ? kWriteDataOnly : (any & 1u) ? kWriteRebuild : kWriteDelta;
  const uint64_t rel = (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;  // from the range's start
  WriteLane w;
  w.off = rr.offset + rel;
  w.end = rr.offset + rr.len;
  w.z = (w.off / 8 + 1) * kSplitmixGolden;
  write_tile<U, NT, T, DIG>(data, parity, digests, mode, c, j, x, w, g,
                            ListWritten<At>{at, e, n, c, j, m, fresh + rel, rr.len});
}

// The list in device memory: n items, then their loss bits (xec_kernels.h).
template <int U, bool NT, int T, bool DIG>
__global__ __launch_bounds__(T) void write_list_kernel(uint8_t* data, uint8_t* parity,
                                                       const uint8_t* __restrict__ fresh,
                                                       const uint32_t* __restrict__ items,
                                                       uint64_t* digests, ReadRange rr,
                                                       Geometry g) {
  const uint64_t n = g.total_tiles / g.tiles_per_block;
  const uint32_t* bits = items + n;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the list, as patch_list_kernel
    write_list_tile<U, NT, T, DIG>(data, parity, fresh, digests, t / g.tiles_per_block, n,
                                   t % g.tiles_per_block, rr, g,
                                   [&](uint64_t q) { return *(const_u32_as4)(items + q); },
                                   [&](uint64_t q) { return *(const_u32_as4)(bits + q); });
  }
}

// The same with items and bits in the kernel arguments (at most CAP items).
template <int U, bool NT, int T, bool DIG, uint32_t CAP>
__global__ __launch_bounds__(T) void write_arglist_kernel(uint8_t* data, uint8_t* parity,
                                                          const uint8_t* __restrict__ fresh,
                                                          uint64_t* digests, ReadRange rr,
                                                          Geometry g, ArgItems<CAP> items,
                                                          ArgItems<CAP / 16> bits) {
  const uint64_t n = g.total_tiles / g.tiles_per_block;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    write_list_tile<U, NT, T, DIG>(data, parity, fresh, digests, t / g.tiles_per_block, n,
                                   t % g.tiles_per_block, rr, g,
                                   [&](uint64_t q) { return items.v[q]; },
                                   [&](uint64_t q) { return bits.v[q]; });
  }
}

// The written members of a class as the device mask marks them; fresh mirrors
// data, `first` = this lane's first granule in the class's member 0.
struct MaskWritten {
  uint64_t mrow;  // address of the mask byte of member 0
  uint32_t nm, j, m;
  const uint8_t* first;
  uint64_t stride;

  template <typename F>
  __device__ __forceinline__ void each(F f) {
    for (uint32_t r = 0; r < nm; ++r)
      if (sbyte(mrow + (uint64_t)r * m) != 0) f(j + r * m, first + r * stride);
  }
  __device__ __forceinline__ bool written(uint32_t r, const uint8_t*& fr) {
    if (sbyte(mrow + (uint64_t)r * m) == 0) return false;
    fr = first + r * stride;
    return true;
  }
};

// Class tiles over a device mask and bitmap (xec_write_device), gated on
// write_check_kernel's verdict: (stripe, class, chunk of the range).  A class
// without a marked member is skipped after its mask bytes; bitmap == nullptr
// means everything is present.
template <int U, bool NT, int T, bool DIG>
__global__ __launch_bounds__(T) void write_class_kernel(uint8_t* data, uint8_t* parity,
                                                        const uint8_t* __restrict__ fresh,
                                                        const uint8_t* __restrict__ mask,
                                                        const uint8_t* __restrict__ bitmap,
                                                        uint64_t* digests, ReadRange rr,
                                                        Geometry g) {
  if (*(const_i32_as4)g.gate != 0) return;
  const uint32_t nm = (uint32_t)g.nm, m = (uint32_t)g.m;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as patch_class_kernel
    const TileCoord tc = tile_coord(t, g);
    const uint32_t j = (uint32_t)tc.j;
    const uint64_t mrow = reinterpret_cast<uint64_t>(mask + tc.c * g.k) + j;
    const uint64_t brow = reinterpret_cast<uint64_t>(bitmap) + tc.c * (g.k + g.m);
    bool any = false, lost = false;
    uint32_t x = 0;
    for (uint32_t r = 0; r < nm; ++r) {
      if (sbyte(mrow + (uint64_t)r * m) == 0) continue;
      any = true;
      if (bitmap != nullptr && sbyte(brow + j + (uint64_t)r * m) == 0) {
        lost = true;
        x = j + r * m;
      }
    }
    if (!any) continue;
    const bool plost = bitmap != nullptr && sbyte(brow + g.k + j) == 0;
    const int mode = plost ? kWriteDataOnly : lost ? kWriteRebuild : kWriteDelta;
    WriteLane w;
    w.off = rr.offset + (tc.chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
    w.end = rr.offset + rr.len;
    w.z = (w.off / 8 + 1) * kSplitmixGolden;
    write_tile<U, NT, T, DIG>(data, parity, digests, mode, tc.c, j, x, w, g,
                              MaskWritten{mrow, nm, j, m,
                                          fresh + (tc.c * g.k + j) * g.bs + w.off, m * g.bs});
  }
}

// One thread per (stripe, class): *status = 4 if a marked member of the class
// is lost while another block of the class (a member or the parity) is lost.
__global__ __launch_bounds__(256) void write_check_kernel(const uint8_t* __restrict__ bitmap,
                                                         const uint8_t* __restrict__ mask,
                                                         Geometry g, int32_t* status) {
  const uint64_t row = g.k + g.m, n = g.S * g.m;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n;
       t += (uint64_t)gridDim.x * 256) {
    const uint64_t c = t / g.m, j = t % g.m;
    const uint8_t* b = bitmap + c * row;
    const uint8_t* mk = mask + c * g.k;
    uint32_t lost = b[g.k + j] == 0, marked_lost = 0;
    for (uint64_t l = j; l < g.k; l += g.m) {
      if (b[l] != 0) continue;
      ++lost;
      marked_lost |= mk[l] != 0;
    }
    if (marked_lost != 0 && lost > 1) atomicMax(status, 4 /* XEC_DECODE_FAILURE */);
  }
}

hipError_t launch_write(void* d_data, void* d_parity, const void* d_new, const void* d_sel,
                        const uint8_t* d_bitmap, uint64_t* d_digests, const Geometry& g_class,
                        const LaunchShape& ls, int tiling, uint64_t offset, uint64_t len,
                        hipStream_t s, uint64_t n_items, const uint32_t* h_items,
                        const uint32_t* h_bits) {
  if (len == 0 || offset % 16 != 0 || len % 16 != 0 || offset + len > g_class.bs ||
      tiling < kUpdateClassTiles || tiling > kUpdateArgListTiles)
    return hipErrorInvalidValue;
  const Geometry g = range_geometry(
      g_class, ls, len, tiling == kUpdateClassTiles ? g_class.S * g_class.m : n_items);
  if (g.total_tiles == 0) return hipSuccess;
  if (g.k > 256 && tiling != kUpdateClassTiles) return hipErrorInvalidValue;
  if (tiling == kUpdateArgListTiles &&
      (n_items > kArgItems || h_items == nullptr || h_bits == nullptr))
    return hipErrorInvalidValue;
  if (tiling != kUpdateArgListTiles && d_sel == nullptr) return hipErrorInvalidValue;
  if (tiling == kUpdateClassTiles && g.gate == nullptr) return hipErrorInvalidValue;
  const ReadRange rr{offset, len};
  uint8_t* d = static_cast<uint8_t*>(d_data);
  uint8_t* p = static_cast<uint8_t*>(d_parity);
  const uint8_t* f = static_cast<const uint8_t*>(d_new);
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  const uint32_t lds = ls.lds_bytes;
  return with_shape(ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    return with_bool(d_digests != nullptr, [&](auto dig) {
      constexpr bool DIG = decltype(dig)::value;
      switch (tiling) {
        case kUpdateArgListTiles:
          return with_capacity(n_items, [&](auto cap) {
            constexpr uint32_t CAP = decltype(cap)::value;  // and two bits per item
            return launch_codec(write_arglist_kernel<U, NT, T, DIG, CAP>, grid, T, lds, s, d, p, f,
                                d_digests, rr, g, arg_items<CAP>(h_items, n_items),
                                arg_items<CAP / 16>(h_bits, (n_items + 15) / 16));
          });
        case kUpdateListTiles:
          return launch_codec(write_list_kernel<U, NT, T, DIG>, grid, T, lds, s, d, p, f,
                              static_cast<const uint32_t*>(d_sel), d_digests, rr, g);
        default:
          return launch_codec(write_class_kernel<U, NT, T, DIG>, grid, T, lds, s, d, p, f,
                              static_cast<const uint8_t*>(d_sel), d_bitmap, d_digests, rr, g);
      }
    });
  });
}

hipError_t launch_write_check(const uint8_t* d_bitmap, const uint8_t* d_mask, const Geometry& g,
                              int32_t* d_status, hipStream_t s) {
  const uint64_t n = g.S * g.m;
  if (n == 0 || d_bitmap == nullptr) return hipSuccess;
  return launch(write_check_kernel, grid_for((n + 255) / 256, 8192, 256), 256, 0, s, d_bitmap,
                d_mask, g, d_status);
}

// ---------------------------------------------------------------------------
// Shard-major layout (xec_encode_shards, xec_repair_shards_device,
// xec_verify_shards): the layout-aware siblings of encode_kernel,
// repair_class_kernel and verify_kernel.  The class tile, its walk from the end
// of the batch, the column rotation, the fast path and the store policies are
// theirs; what differs is where a block lives.  The k + m shard base pointers
// travel by value in the kernel arguments (ShardTab<CAP>, xec_kernels.h), so
//   member r of class j, stripe c : tab.v[j + r*m] + c*dstride
//   parity block j of stripe c    : tab.v[k + j]   + c*pstride
// -- each a scalar load from the argument segment at a wave-uniform index plus
// a wave-uniform stripe offset; only the lane's byte offset is per lane.  The
// index is below k + m <= CAP for every tile (the launcher checks it).  No
// LDS, no atomics, and the older kernels and their helpers above are
// untouched: these are emitted after them.
// ---------------------------------------------------------------------------

// xor_members over a shard table: member r is tab.v[first + r*m] + doff, except
// member `subst`, whose bytes come from `sub` (the class's parity block).
template <int NM, int U, bool NT, int T, int SAUX, uint32_t CAP>
__device__ __forceinline__ void xor_shard_members(const ShardTab<CAP>& tab, uint64_t first,
                                                  uint64_t m, uint64_t doff, const uint8_t* sub,
                                                  int subst, uint8_t* dst, uint64_t off,
                                                  uint64_t bs, uint32_t nm_rt) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  if constexpr (NM > 0) {
    const bool whole = off + (U - 1) * kStep < bs;  // the tile's last granule row is inside
    if (whole) {
      u32x4 v[NM][U];
#pragma unroll
      for (int r = 0; r < NM; ++r) {
        const uint8_t* src = (r == subst ? sub : tab.v[first + (uint64_t)r * m] + doff) + off;
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(src + u * kStep);
      }
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);  // as xor_members
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r < NM; ++r) acc ^= v[r][u];
        st16_block<NT, SAUX>(dst, off + u * kStep, acc);
      }
      return;
    }
  }
  // Ragged tail of a block, or a member count without a compiled unroll.
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= bs) continue;
    u32x4 acc = {0u, 0u, 0u, 0u};
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rr = (int)(r + q);
        v[q] = ld16<NT>((rr == subst ? sub : tab.v[first + (uint64_t)rr * m] + doff) + o);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r)
      acc ^= ld16<NT>(((int)r == subst ? sub : tab.v[first + (uint64_t)r * m] + doff) + o);
    st16_block<NT, SAUX>(dst, o, acc);
  }
}

// reduce_members over a shard table: the class's members and its parity block
// at `extra`, nothing stored.
template <int NM, int U, bool NT, int T, uint32_t CAP>
__device__ __forceinline__ u32x4 reduce_shard_members(const ShardTab<CAP>& tab, uint64_t first,
                                                      uint64_t m, uint64_t doff,
                                                      const uint8_t* extra, uint64_t off,
                                                      uint64_t bs, uint32_t nm_rt) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  u32x4 any = {0u, 0u, 0u, 0u};
  if constexpr (NM > 0) {
    const bool whole = off + (U - 1) * kStep < bs;
    if (whole) {
      u32x4 v[NM + 1][U];
#pragma unroll
      for (int r = 0; r < NM; ++r) {
        const uint8_t* src = tab.v[first + (uint64_t)r * m] + doff + off;
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(src + u * kStep);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) v[NM][u] = ld16<NT>(extra + off + u * kStep);
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);  // as xor_members
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r <= NM; ++r) acc ^= v[r][u];
        any |= acc;
      }
      return any;
    }
  }
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= bs) continue;
    u32x4 acc = ld16<NT>(extra + o);
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = ld16<NT>(tab.v[first + (uint64_t)(r + q) * m] + doff + o);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r) acc ^= ld16<NT>(tab.v[first + (uint64_t)r * m] + doff + o);
    any |= acc;
  }
  return any;
}

template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void encode_shards_kernel(Geometry g, uint64_t dstride,
                                                          uint64_t pstride, ShardTab<CAP> tab) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the batch, as encode
    const TileCoord tc = tile_coord(t, g);
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    xor_shard_members<NM, U, NT, T, kEncodeStoreAux>(tab, tc.j, g.m, tc.c * dstride, nullptr, -1,
                                                     tab.v[g.k + tc.j] + tc.c * pstride, off, g.bs,
                                                     (uint32_t)g.nm);
  }
}

// Gated on the check's verdict and reading its class's bitmap bytes as
// repair_class_kernel does: a lost parity block is encode's reduction (stored
// nt), a lost member decode's with the parity block in its place (stored sc1).
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void repair_shards_kernel(const uint8_t* __restrict__ bitmap,
                                                          Geometry g, uint64_t dstride,
                                                          uint64_t pstride, ShardTab<CAP> tab) {
  if (g.gate != nullptr && *(const_i32_as4)g.gate != 0) return;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    const TileCoord tc = tile_coord(t, g);
    const uint64_t row = reinterpret_cast<uint64_t>(bitmap + tc.c * (g.k + g.m));
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    uint8_t* par = tab.v[g.k + tc.j] + tc.c * pstride;
    if (sbyte(row + g.k + tc.j) == 0) {
      xor_shard_members<NM, U, NT, T, kEncodeStoreAux>(tab, tc.j, g.m, tc.c * dstride, nullptr, -1,
                                                       par, off, g.bs, nm);
      continue;
    }
    uint32_t lost = nm;
    for (uint32_t r = 0; r < nm; ++r)
      if (sbyte(row + tc.j + (uint64_t)r * g.m) == 0) { lost = r; break; }
    if (lost == nm) continue;
    xor_shard_members<NM, U, NT, T, kDecodeStoreAux>(
        tab, tc.j, g.m, tc.c * dstride, par, (int)lost,
        tab.v[tc.j + (uint64_t)lost * g.m] + tc.c * dstride, off, g.bs, nm);
  }
}

template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void verify_shards_kernel(uint8_t* __restrict__ flags, Geometry g,
                                                          uint64_t dstride, uint64_t pstride,
                                                          ShardTab<CAP> tab) {
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    const TileCoord tc = tile_coord(t, g);
    const uint64_t off = (rotated(tc.chunk, tc.c, g) * (uint64_t)(T * U) + threadIdx.x) * 16;
    const u32x4 v = reduce_shard_members<NM, U, NT, T>(tab, tc.j, g.m, tc.c * dstride,
                                                       tab.v[g.k + tc.j] + tc.c * pstride, off,
                                                       g.bs, (uint32_t)g.nm);
    // every lane of the workgroup gets here: the tile loop is uniform
    const uint64_t bad = __ballot((v.x | v.y | v.z | v.w) != 0u);
    if (bad != 0 && (threadIdx.x & 63u) == 0) flags[tc.c * g.m + tc.j] = 1;
  }
}

// ---------------------------------------------------------------------------
// Shard-major digest, locate and degraded read (xec_digest_shards,
// xec_locate_shards, xec_read_shards_device): digest_kernel and read_dev_kernel
// with a block's address taken from the shard table,
//   block i of stripe c : tab.v[i] + c * (i < k ? dstride : pstride)
// -- the tile's block index is uniform per workgroup, so that is one scalar
// load from the argument segment and a scalar multiply-add per tile.  Segments,
// loads in flight, the reduction and its one 64-bit atomic add per (block,
// segment), the gate, the range tiles, the store through the item's slot: all
// theirs.  digest_zero_kernel, locate_compare_kernel and read_check_kernel touch
// no block and serve both layouts.  Emitted after everything above, which stays
// instruction for instruction what it was.
// ---------------------------------------------------------------------------
template <bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void digest_shards_kernel(const uint8_t* __restrict__ gate,
                                                          int mode, uint64_t* out, Geometry g,
                                                          uint64_t dstride, uint64_t pstride,
                                                          ShardTab<CAP> tab) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  constexpr uint64_t kStepZ = (uint64_t)(2 * T) * kSplitmixGolden;  // 2*T words per step
  constexpr int kInFlight = 8;                                      // as digest_kernel
  __shared__ uint64_t wave_sum[T / 64];
  const uint64_t tot = g.k + g.m;
  for (uint64_t t = blockIdx.x; t < g.total_tiles; t += gridDim.x) {
    const uint64_t seg = t % g.tiles_per_block, b = t / g.tiles_per_block;
    const uint64_t c = b / tot, i = b % tot;
    if (!digest_wanted(gate, mode, c, i, g)) continue;  // uniform: scalar loads only
    const uint8_t* blk = tab.v[i] + c * (i < g.k ? dstride : pstride);
    const uint64_t begin = seg * kDigestSegmentBytes;
    const uint64_t end = g.bs - begin < kDigestSegmentBytes ? g.bs : begin + kDigestSegmentBytes;
    uint64_t off = begin + threadIdx.x * 16ull;
    uint64_t z = (off / 8 + 1) * kSplitmixGolden;  // (n + 1) * golden of this lane's first word
    uint64_t acc = 0;
    for (; off + (kInFlight - 1) * kStep < end; off += kInFlight * kStep, z += kInFlight * kStepZ) {
      u32x4 v[kInFlight];
#pragma unroll
      for (int q = 0; q < kInFlight; ++q) v[q] = ld16<NT>(blk + off + q * kStep);
#pragma unroll
      for (int q = 0; q < kInFlight; ++q) acc += digest_granule(v[q], z + q * kStepZ);
    }
    // the tail issues every load before the first multiply, as digest_kernel's
    if (off < end) {
      u32x4 v[kInFlight - 1];
#pragma unroll
      for (int q = 0; q < kInFlight - 1; ++q)
        if (off + q * kStep < end) v[q] = ld16<NT>(blk + off + q * kStep);
#pragma unroll
      for (int q = 0; q < kInFlight - 1; ++q)
        if (off + q * kStep < end) acc += digest_granule(v[q], z + q * kStepZ);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    if constexpr (T > 64) {  // the tile loop is uniform per workgroup: every wave gets here
      if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        acc = 0;
#pragma unroll
        for (int w = 0; w < T / 64; ++w) acc += wave_sum[w];
      }
      __syncthreads();  // wave_sum is free for the next tile
    }
    if (threadIdx.x == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(out + b), (unsigned long long)acc);
  }
}

// xor_shard_members with the store left to the caller: to xor_shard_members what
// xor_members_to is to xor_members (and a copy for the reason given there).
// store(o, v) takes the granule at block offset o; `end` is the end of what the
// tile may touch, the range's end inside the block.
template <int NM, int U, bool NT, int T, uint32_t CAP, typename Store>
__device__ __forceinline__ void xor_shard_members_to(const ShardTab<CAP>& tab, uint64_t first,
                                                     uint64_t m, uint64_t doff,
                                                     const uint8_t* sub, int subst, uint64_t off,
                                                     uint64_t end, uint32_t nm_rt, Store store) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  if constexpr (NM > 0) {
    const bool whole = off + (U - 1) * kStep < end;  // the tile's last granule row is in the range
    if (whole) {
      u32x4 v[NM][U];
#pragma unroll
      for (int r = 0; r < NM; ++r) {
        const uint8_t* src = (r == subst ? sub : tab.v[first + (uint64_t)r * m] + doff) + off;
#pragma unroll
        for (int u = 0; u < U; ++u) v[r][u] = ld16<NT>(src + u * kStep);
      }
      if constexpr (NM >= 32) __builtin_amdgcn_sched_barrier(0);  // as xor_members
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 acc = v[0][u];
#pragma unroll
        for (int r = 1; r < NM; ++r) acc ^= v[r][u];
        store(off + u * kStep, acc);
      }
      return;
    }
  }
  // Ragged tail of the range, or a member count without a compiled unroll.
  const uint32_t nm = NM > 0 ? (uint32_t)NM : nm_rt;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t o = off + u * kStep;
    if (o >= end) continue;
    u32x4 acc = {0u, 0u, 0u, 0u};
    uint32_t r = 0;
    for (; r + 8 <= nm; r += 8) {
      u32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rr = (int)(r + q);
        v[q] = ld16<NT>((rr == subst ? sub : tab.v[first + (uint64_t)rr * m] + doff) + o);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc ^= v[q];
    }
    for (; r < nm; ++r)
      acc ^= ld16<NT>(((int)r == subst ? sub : tab.v[first + (uint64_t)r * m] + doff) + o);
    store(o, acc);
  }
}

// read_dev_kernel over a shard table: gated on read_check_kernel's verdict (so
// every item it sees is in range -- i < k + m <= CAP -- and servable), the
// verdict of an item its own bitmap byte, tiles walked from the end of the list.
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void read_shards_kernel(uint8_t* out,
                                                        const uint32_t* __restrict__ items,
                                                        const uint8_t* __restrict__ bitmap,
                                                        ReadRange rr, Geometry g, uint64_t dstride,
                                                        uint64_t pstride, ShardTab<CAP> tab) {
  if (*(const_i32_as4)g.gate != 0) return;
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m, k = (uint32_t)g.k;
  const uint64_t end = rr.offset + rr.len;
  const uint32_t len = (uint32_t)rr.len;
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;
    const uint64_t e = t / g.tiles_per_block, chunk = t % g.tiles_per_block;
    const uint32_t item = *(const_u32_as4)(items + e);
    const uint64_t c = item >> 8;
    const uint32_t i = item & 0xFFu;
    const bool lost = bitmap != nullptr &&
                      sbyte(reinterpret_cast<uint64_t>(bitmap) + c * (g.k + g.m) + i) == 0;
    const uint64_t off = rr.offset + (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
    uint8_t* slot = out + e * rr.len;
    auto store = [&](uint64_t o, u32x4 v) { st16_slot<NT>(slot, len, o - rr.offset, v); };
    if (!lost) {
      const uint8_t* blk = tab.v[i] + c * (i < k ? dstride : pstride);
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (off + u * kStep < end) v[u] = ld16<NT>(blk + off + u * kStep);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (off + u * kStep < end) store(off + u * kStep, v[u]);
      continue;
    }
    const uint32_t j = i < k ? i % m : i - k;  // the item's class
    if (i < k)  // a data block: the other members and the class parity, as decode
      xor_shard_members_to<NM, U, NT, T>(tab, j, g.m, c * dstride, tab.v[g.k + j] + c * pstride,
                                         (int)(i / m), off, end, nm, store);
    else  // a parity block: every data member, as encode
      xor_shard_members_to<NM, U, NT, T>(tab, j, g.m, c * dstride, nullptr, -1, off, end, nm,
                                         store);
  }
}

// ---------------------------------------------------------------------------
// Shard-major degraded write and vectored read (xec_write_shards_device,
// xec_readv_shards_device).
//
// The write is the list-tiled degraded write (write_list_kernel) with the list
// checked on the device instead of the host: write_items_check_kernel leaves its
// verdict in *status and write_shards_kernel is gated on it, so every item the
// write sees is in range (c < S, i < k <= CAP), strictly ascending and servable.
// Ownership is write_list_tile's; the two loss bits a host-checked list carries
// per item are read here from the bitmap by the owner (scalar byte loads, as
// write_class_kernel): the item's own byte and its class's parity byte.  Blocks
// are addressed through the table,
//   data block i of stripe c   : tab.v[i]     + c*dstride
//   parity block j of stripe c : tab.v[k + j] + c*pstride
// index and stripe offset wave-uniform and 64-bit.  write_shard_tile is
// write_tile with those addresses -- a sibling, as xor_shard_members is
// xor_members', so that write_tile and the batch write kernels stay instruction
// for instruction what they were.  The lane helpers (write_plain, patch_fold,
// patch_mix, patch_wave_add), the three modes, the store policies (new data
// sc1, parity nt), the digest upkeep and the bounds argument are the batch
// write's.  readv_shards_kernel is readv_dev_kernel with read_shards_kernel's
// tile.  Emitted after everything above.
// ---------------------------------------------------------------------------
template <int U, bool NT, int T, bool DIG, uint32_t CAP, typename Src>
__device__ __forceinline__ void write_shard_tile(const ShardTab<CAP>& tab, uint64_t doff,
                                                 uint8_t* par, uint64_t* digests, int mode,
                                                 uint64_t c, uint32_t j, uint32_t x,
                                                 const WriteLane& w, const Geometry& g, Src src) {
  constexpr uint64_t kStep = (uint64_t)T * 16;
  uint64_t* row = digests + c * (g.k + g.m);
  if (mode == kWriteDataOnly) {
    src.each([&](uint32_t i, const uint8_t* fr) {
      const uint64_t d = write_plain<U, NT, T, DIG>(tab.v[i] + doff, fr, w);
      if constexpr (DIG) patch_wave_add(row + i, d);
    });
    return;
  }
  u32x4 acc[U];
  uint64_t psum = 0;
  if (mode == kWriteDelta) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (w.off + u * kStep < w.end) acc[u] = ld16<NT>(par + w.off + u * kStep);
    if constexpr (DIG) psum = 0 - patch_mix<U, T>(acc, w.off, w.end, w.z);
    src.each([&](uint32_t i, const uint8_t* fr) {
      const uint64_t d = patch_fold<U, NT, T, DIG>(acc, tab.v[i] + doff, fr, w.off, w.end, w.z);
      if constexpr (DIG) patch_wave_add(row + i, d);
    });
  } else {
    // rebuild: every member has a source; acc becomes the new parity
    const uint32_t nm = (uint32_t)g.nm, m = (uint32_t)g.m;
    u32x4 oldx[U];  // DIG: XOR of the old bytes of every member but x
    uint64_t dx = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[u] = u32x4{0u, 0u, 0u, 0u};
      oldx[u] = u32x4{0u, 0u, 0u, 0u};
    }
    // member block i with its bytes v loaded from `written ? new : data`
    auto absorb = [&](uint32_t i, bool written, const u32x4(&v)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) acc[u] ^= v[u];
      if (!written) {
        if constexpr (DIG) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (w.off + u * kStep < w.end) oldx[u] ^= v[u];
        }
        return;
      }
      if (i == x) {  // the lost member: its new bytes went into the parity only
        if constexpr (DIG) dx = patch_mix<U, T>(v, w.off, w.end, w.z);
        return;
      }
      uint8_t* block = tab.v[i] + doff;
      if constexpr (DIG) {
        u32x4 o[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (w.off + u * kStep < w.end) {
            o[u] = ld16<NT>(block + w.off + u * kStep);
            oldx[u] ^= o[u];
          }
        patch_wave_add(row + i, patch_mix<U, T>(v, w.off, w.end, w.z) -
                                    patch_mix<U, T>(o, w.off, w.end, w.z));
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end)
          st16_block<NT, kPatchDataStoreAux>(block, w.off + u * kStep, v[u]);
    };
    uint32_t r = 0;
    // 8 members' loads in flight per granule, and not with DIG: as write_tile
    for (; !DIG && r + 8 <= nm; r += 8) {
      const uint8_t* from[8];
      bool wr[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint32_t i = j + (r + q) * m;
        const uint8_t* fr = nullptr;
        wr[q] = src.written(r + q, fr);
        from[q] = wr[q] ? fr : tab.v[i] + doff + w.off;
      }
      u32x4 v[8][U];
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (w.off + u * kStep < w.end) v[q][u] = ld16<NT>(from[q] + u * kStep);
#pragma unroll
      for (int q = 0; q < 8; ++q) absorb(j + (r + q) * m, wr[q], v[q]);
    }
    for (; r < nm; ++r) {
      const uint32_t i = j + r * m;
      const uint8_t* fr = nullptr;
      const bool wr = src.written(r, fr);
      const uint8_t* from = wr ? fr : tab.v[i] + doff + w.off;
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) v[u] = ld16<NT>(from + u * kStep);
      absorb(i, wr, v);
    }
    if constexpr (DIG) {
      u32x4 pold[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (w.off + u * kStep < w.end) {
          pold[u] = ld16<NT>(par + w.off + u * kStep);
          oldx[u] ^= pold[u];  // what block x virtually held
        }
      psum = 0 - patch_mix<U, T>(pold, w.off, w.end, w.z);
      patch_wave_add(row + x, dx - patch_mix<U, T>(oldx, w.off, w.end, w.z));
    }
  }
  if constexpr (DIG) psum += patch_mix<U, T>(acc, w.off, w.end, w.z);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (w.off + u * kStep < w.end)
      st16_block<NT, kPatchParityStoreAux>(par, w.off + u * kStep, acc[u]);
  if constexpr (DIG) patch_wave_add(row + g.k + j, psum);
}

// (list position, chunk of the range) tiles over a device list and bitmap,
// gated on write_items_check_kernel's verdict.  The first item of a (stripe,
// class) owns the class; an item of another stripe ends the walk back, so the
// same class index in the previous stripe is not an earlier owner.
template <int U, bool NT, int T, bool DIG, uint32_t CAP>
__global__ __launch_bounds__(T) void write_shards_kernel(const uint8_t* __restrict__ fresh,
                                                         const uint32_t* __restrict__ items,
                                                         const uint8_t* __restrict__ bitmap,
                                                         uint64_t* digests, ReadRange rr,
                                                         Geometry g, uint64_t dstride,
                                                         uint64_t pstride, ShardTab<CAP> tab) {
  if (*(const_i32_as4)g.gate != 0) return;
  const uint64_t n = g.total_tiles / g.tiles_per_block;
  const uint32_t m = (uint32_t)g.m;
  auto at = [&](uint64_t q) { return *(const_u32_as4)(items + q); };
  for (uint64_t t0 = blockIdx.x; t0 < g.total_tiles; t0 += gridDim.x) {
    const uint64_t t = g.total_tiles - 1 - t0;  // from the end of the list, as write_list_kernel
    const uint64_t e = t / g.tiles_per_block, chunk = t % g.tiles_per_block;
    const uint32_t item = at(e);
    const uint32_t c = item >> 8, j = (item & 0xFFu) % m;
    bool owner = true;
    for (uint64_t q = e; q > 0;) {
      const uint32_t prev = at(--q);
      if ((prev >> 8) != c) break;
      if ((prev & 0xFFu) % m == j) { owner = false; break; }  // an earlier item's tile handles it
    }
    if (!owner) continue;
    const uint64_t brow = reinterpret_cast<uint64_t>(bitmap) + (uint64_t)c * (g.k + g.m);
    bool lost = false, plost = false;
    uint32_t x = 0;
    if (bitmap != nullptr) {
      for (uint64_t q = e; q < n; ++q) {
        const uint32_t it = at(q);
        if ((it >> 8) != c) break;
        const uint32_t i = it & 0xFFu;
        if (i % m != j) continue;
        if (sbyte(brow + i) == 0) {
          lost = true;
          x = i;
        }
      }
      plost = sbyte(brow + g.k + j) == 0;
    }
    const int mode = plost ? kWriteDataOnly : lost ? kWriteRebuild : kWriteDelta;
    WriteLane w;
    w.off = rr.offset + (chunk * (uint64_t)(T * U) + threadIdx.x) * 16;
    w.end = rr.offset + rr.len;
    w.z = (w.off / 8 + 1) * kSplitmixGolden;
    // item t's new bytes of this lane's first granule: fresh + t*len + its distance from `offset`
    write_shard_tile<U, NT, T, DIG>(tab, (uint64_t)c * dstride,
                                    tab.v[g.k + j] + (uint64_t)c * pstride, digests, mode, c, j, x,
                                    w, g,
                                    ListWritten<decltype(at)>{at, e, n, c, j, m,
                                                              fresh + (w.off - rr.offset), rr.len});
  }
}

// One thread per item: *status = max(*status, verdict) over the items, verdict
// 3 for c >= S, i >= k or an item not above its predecessor (raw words, so
// disorder and repeats alike), 4 for a lost block with another block of its
// class lost too.  An item out of range never indexes the bitmap; bitmap ==
// nullptr means everything is present and leaves the order rule.
__global__ __launch_bounds__(256) void write_items_check_kernel(const uint8_t* __restrict__ bitmap,
                                                               const uint32_t* __restrict__ items,
                                                               uint64_t n, Geometry g,
                                                               int32_t* status) {
  const uint64_t row = g.k + g.m;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n;
       t += (uint64_t)gridDim.x * 256) {
    const uint32_t item = items[t];
    const uint64_t c = item >> 8, i = item & 0xFFu;
    const bool in_range = c < g.S && i < g.k;
    int32_t verdict = !in_range || (t > 0 && items[t - 1] >= item) ? 3 : 0;
    if (in_range && bitmap != nullptr && bitmap[c * row + i] == 0) {
      const uint8_t* r = bitmap + c * row;
      const uint64_t j = i % g.m;
      uint32_t others = r[g.k + j] == 0;
      for (uint64_t l = j; l < g.k; l += g.m) others += l != i && r[l] == 0;
      if (others != 0) verdict = 4;
    }
    if (verdict != 0) atomicMax(status, verdict);
  }
}

// readv_dev_kernel over a shard table: gated on the verdict of readv_check_kernel
// and readv_scan_kernel, the schedule in `work` as there, the tile
// read_shards_kernel's with the entry's own range and slot.
template <int NM, int U, bool NT, int T, uint32_t CAP>
__global__ __launch_bounds__(T) void readv_shards_kernel(uint8_t* out,
                                                         const uint32_t* __restrict__ iov,
                                                         const uint8_t* __restrict__ bitmap,
                                                         const uint32_t* __restrict__ work,
                                                         uint32_t n, Geometry g, uint64_t dstride,
                                                         uint64_t pstride, ShardTab<CAP> tab) {
  if (*(const_i32_as4)g.gate != 0) return;
  constexpr uint64_t kStep = (uint64_t)T * 16;
  const uint32_t nm = NM > 0 ? (uint32_t)NM : (uint32_t)g.nm;
  const uint32_t m = (uint32_t)g.m, k = (uint32_t)g.k;
  const uint32_t* tiles = work + 2 * ((uint64_t)n + 1);
  auto tile = [&](uint32_t x) { return *(const_u32_as4)(tiles + x); };
  const uint32_t total = tile(n);
  for (uint64_t t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
    const uint32_t t = total - 1 - (uint32_t)t0;
    const uint32_t e = readv_find(tile, n, t);
    const uint32_t* ent = iov + 3 * (uint64_t)e;
    const uint32_t item = *(const_u32_as4)ent;
    const ReadRange rr{*(const_u32_as4)(ent + 1), *(const_u32_as4)(ent + 2)};
    const uint64_t start = (uint64_t) * (const_u32_as4)(work + 2 * (uint64_t)e + 1) << 32 |
                           *(const_u32_as4)(work + 2 * (uint64_t)e);
    const uint64_t c = item >> 8;
    const uint32_t i = item & 0xFFu;
    const bool lost = bitmap != nullptr &&
                      sbyte(reinterpret_cast<uint64_t>(bitmap) + c * (g.k + g.m) + i) == 0;
    const uint64_t end = rr.offset + rr.len;
    const uint32_t len = (uint32_t)rr.len;
    const uint64_t off = rr.offset + ((uint64_t)(t - tile(e)) * (uint64_t)(T * U) + threadIdx.x) * 16;
    uint8_t* slot = out + start;
    auto store = [&](uint64_t o, u32x4 v) { st16_slot<NT>(slot, len, o - rr.offset, v); };
    if (!lost) {
      const uint8_t* blk = tab.v[i] + c * (i < k ? dstride : pstride);
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (off + u * kStep < end) v[u] = ld16<NT>(blk + off + u * kStep);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (off + u * kStep < end) store(off + u * kStep, v[u]);
      continue;
    }
    const uint32_t j = i < k ? i % m : i - k;  // the entry's class
    if (i < k)  // a data block: the other members and the class parity, as decode
      xor_shard_members_to<NM, U, NT, T>(tab, j, g.m, c * dstride, tab.v[g.k + j] + c * pstride,
                                         (int)(i / m), off, end, nm, store);
    else  // a parity block: every data member, as encode
      xor_shard_members_to<NM, U, NT, T>(tab, j, g.m, c * dstride, nullptr, -1, off, end, nm,
                                         store);
  }
}

namespace {

// The k + m of h_shards in a ShardTab<CAP>, the rest null (never indexed).
template <uint32_t CAP>
ShardTab<CAP> shard_tab(const void* const* h_shards, uint64_t n) {
  ShardTab<CAP> t;
  for (uint64_t i = 0; i < CAP; ++i)
    t.v[i] = i < n ? static_cast<uint8_t*>(const_cast<void*>(h_shards[i])) : nullptr;
  return t;
}

// with_shape and with_shard_capacity (xec_dispatch.h) in one: f(shape, capacity).
template <class F>
hipError_t with_shard_shape(const Geometry& g, const LaunchShape& ls, F&& f) {
  return with_shape(g.nm, ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    return with_shard_capacity(g.k + g.m, [&](auto cap) { return f(sh, cap); });
  });
}

bool shard_launch_ok(const void* const* h_shards, const Geometry& g) {
  return h_shards != nullptr && g.k + g.m <= kShardPtrs;
}

}  // namespace

hipError_t launch_encode_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const Geometry& g, const LaunchShape& ls, hipStream_t s) {
  if (g.total_tiles == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g)) return hipErrorInvalidValue;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shard_shape(g, ls, [&](auto sh, auto cap) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch_codec(encode_shards_kernel<NM, U, NT, T, CAP>, grid, T, ls.lds_bytes, s, g,
                        dstride, pstride, shard_tab<CAP>(h_shards, g.k + g.m));
  });
}

hipError_t launch_repair_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const uint8_t* d_bitmap, const Geometry& g, const LaunchShape& ls,
                                hipStream_t s) {
  if (g.total_tiles == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g) || g.gate == nullptr) return hipErrorInvalidValue;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shard_shape(g, ls, [&](auto sh, auto cap) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch_codec(repair_shards_kernel<NM, U, NT, T, CAP>, grid, T, ls.lds_bytes, s,
                        d_bitmap, g, dstride, pstride, shard_tab<CAP>(h_shards, g.k + g.m));
  });
}

hipError_t launch_verify_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                uint8_t* d_flags, const Geometry& g, const LaunchShape& ls,
                                hipStream_t s) {
  if (g.total_tiles == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g)) return hipErrorInvalidValue;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shard_shape(g, ls, [&](auto sh, auto cap) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch_codec(verify_shards_kernel<NM, U, NT, T, CAP>, grid, T, ls.lds_bytes, s,
                        d_flags, g, dstride, pstride, shard_tab<CAP>(h_shards, g.k + g.m));
  });
}

// launch_digest over a shard table: the same zeroing, tiles and grid.
hipError_t launch_digest_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                                const uint8_t* d_gate, int mode, uint64_t* d_out,
                                const Geometry& g_class, const LaunchShape& ls, hipStream_t s) {
  Geometry g = g_class;
  g.tiles_per_block = (g.bs + kDigestSegmentBytes - 1) / kDigestSegmentBytes;
  g.total_tiles = g.S * (g.k + g.m) * g.tiles_per_block;
  if (g.total_tiles == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g) || d_out == nullptr ||
      (mode != kDigestAll && d_gate == nullptr) || mode < kDigestAll || mode > kDigestFlags)
    return hipErrorInvalidValue;
  const uint64_t slots = g.S * (g.k + g.m);
  const hipError_t e =
      mode == kDigestAll
          ? hipMemsetAsync(d_out, 0, slots * sizeof(uint64_t), s)
          : launch(digest_zero_kernel, grid_for((slots + 255) / 256, 8192, 256), 256, 0, s, d_gate,
                   mode, d_out, g);
  if (e != hipSuccess) return e;
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_bool(ls.nt, [&](auto ntc) {
    constexpr bool NT = decltype(ntc)::value;
    return with_shard_capacity(g.k + g.m, [&](auto cap) {
      constexpr uint32_t CAP = decltype(cap)::value;
      const ShardTab<CAP> tab = shard_tab<CAP>(h_shards, g.k + g.m);
      if (ls.threads == 256)
        return launch_codec(digest_shards_kernel<NT, 256, CAP>, grid, 256, ls.lds_bytes, s, d_gate,
                            mode, d_out, g, dstride, pstride, tab);
      return launch_codec(digest_shards_kernel<NT, 64, CAP>, grid, 64, ls.lds_bytes, s, d_gate,
                          mode, d_out, g, dstride, pstride, tab);
    });
  });
}

// launch_read with kReadDevTiles over a shard table (g.gate must be set).
hipError_t launch_read_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                              void* d_out, const Geometry& g_class, const LaunchShape& ls,
                              uint64_t offset, uint64_t len, uint64_t n_items,
                              const uint32_t* d_items, const uint8_t* d_bitmap, hipStream_t s) {
  if (n_items == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g_class) || d_out == nullptr || d_items == nullptr || len == 0 ||
      offset % 16 != 0 || len % 16 != 0 || offset + len > g_class.bs || g_class.gate == nullptr)
    return hipErrorInvalidValue;
  const Geometry g = range_geometry(g_class, ls, len, n_items);
  const ReadRange rr{offset, len};
  uint8_t* out = static_cast<uint8_t*>(d_out);
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shard_shape(g, ls, [&](auto sh, auto cap) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch_codec(read_shards_kernel<NM, U, NT, T, CAP>, grid, T, ls.lds_bytes, s, out,
                        d_items, d_bitmap, rr, g, dstride, pstride,
                        shard_tab<CAP>(h_shards, g.k + g.m));
  });
}

// launch_write's list tiles over a shard table, list and bitmap on the device
// (g.gate must be set: launch_write_items_check's verdict).
hipError_t launch_write_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                               const void* d_new, const uint32_t* d_items,
                               const uint8_t* d_bitmap, uint64_t* d_digests,
                               const Geometry& g_class, const LaunchShape& ls, uint64_t offset,
                               uint64_t len, uint64_t n_items, hipStream_t s) {
  if (n_items == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g_class) || d_new == nullptr || d_items == nullptr || len == 0 ||
      offset % 16 != 0 || len % 16 != 0 || offset + len > g_class.bs || g_class.gate == nullptr)
    return hipErrorInvalidValue;
  const Geometry g = range_geometry(g_class, ls, len, n_items);
  const ReadRange rr{offset, len};
  const uint8_t* f = static_cast<const uint8_t*>(d_new);
  const uint32_t grid = grid_for(g.total_tiles, ls.max_grid, ls.threads);
  return with_shape(ls.unroll, ls.nt, ls.threads, [&](auto sh) {
    constexpr int U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    return with_bool(d_digests != nullptr, [&](auto dig) {
      constexpr bool DIG = decltype(dig)::value;
      return with_shard_capacity(g.k + g.m, [&](auto cap) {
        constexpr uint32_t CAP = decltype(cap)::value;
        return launch_codec(write_shards_kernel<U, NT, T, DIG, CAP>, grid, T, ls.lds_bytes, s, f,
                            d_items, d_bitmap, d_digests, rr, g, dstride, pstride,
                            shard_tab<CAP>(h_shards, g.k + g.m));
      });
    });
  });
}

hipError_t launch_write_items_check(const uint8_t* d_bitmap, const uint32_t* d_items, uint64_t n,
                                    const Geometry& g, int32_t* d_status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return launch(write_items_check_kernel, grid_for((n + 255) / 256, 8192, 256), 256, 0, s,
                d_bitmap, d_items, n, g, d_status);
}

// launch_readv with kReadDevTiles over a shard table (g.gate must be set).
hipError_t launch_readv_shards(const void* const* h_shards, uint64_t dstride, uint64_t pstride,
                               void* d_out, const Geometry& g, const LaunchShape& ls, uint64_t n,
                               uint64_t tiles, const uint32_t* d_iov, const uint8_t* d_bitmap,
                               const uint32_t* d_work, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!shard_launch_ok(h_shards, g) || d_out == nullptr || d_iov == nullptr ||
      d_work == nullptr || n > 0xFFFFFFFFull || tiles > 0xFFFFFFFFull || g.gate == nullptr)
    return hipErrorInvalidValue;
  uint8_t* out = static_cast<uint8_t*>(d_out);
  const uint32_t grid = grid_for(tiles, ls.max_grid, ls.threads);
  return with_shard_shape(g, ls, [&](auto sh, auto cap) {
    constexpr int NM = decltype(sh)::NM, U = decltype(sh)::U, T = decltype(sh)::T;
    constexpr bool NT = decltype(sh)::NT;
    constexpr uint32_t CAP = decltype(cap)::value;
    return launch_codec(readv_shards_kernel<NM, U, NT, T, CAP>, grid, T, ls.lds_bytes, s, out,
                        d_iov, d_bitmap, d_work, (uint32_t)n, g, dstride, pstride,
                        shard_tab<CAP>(h_shards, g.k + g.m));
  });
}

// Test hook only (tests/host/error_preserve.cpp).  A user who finds it set
// is told once, on stderr, that every launch of the library will fail
// (a silent hook in the shipped library).
thread_local KernelEvents t_kernel_events;

bool fail_launch_for_test() {
  static const bool on = [] {
    const char* e = std::getenv("XEC_TEST_FAIL_LAUNCH");
    const bool set = e != nullptr && e[0] == '1';
    if (set)
      std::fprintf(stderr,
                   "xec: XEC_TEST_FAIL_LAUNCH=1 is set: a TEST hook -- every kernel launch of "
                   "libxec_hip.so will fail on purpose\n");
    return set;
  }();
  return on;
}

// Loads this file's code object onto the current device (see xec_kernels.h).
hipError_t preload_kernels() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&fill_kernel));
}

}  // namespace xec
