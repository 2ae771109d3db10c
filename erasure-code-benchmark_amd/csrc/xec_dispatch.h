// xec_dispatch.h -- run-time launch shape to template arguments, once, for every
// kernel family of xec_kernels.hip.  Plain C++17 and nothing of HIP, so that
// the mapping is testable on the host alone (tests/host/dispatch_map.cpp): a
// launch that picked the generic NM = 0 kernel for 16 members, or an NT = false
// one, would still compute the right bytes, and no GPU test could tell.
#pragma once

#include <cstdint>
#include <type_traits>

namespace xec {

// What a codec kernel is compiled for: NM members per class fully unrolled
// (0 = the generic loop, and unused by the families that have no such
// parameter), U granules per lane, NT non-temporal access, T threads.
template <int NM_, int U_, bool NT_, int T_>
struct Shape {
  static constexpr int NM = NM_, U = U_, T = T_;
  static constexpr bool NT = NT_;
};

// f(std::true_type{}) or f(std::false_type{}): NT below, and the DIG of the
// ranged update and the degraded write.
template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(Shape<NM, U, NT, T>{}) with U = 2 for unroll == 2 and else 1, T = 256 for
// threads == 256 and else 64.  Called without NM by the families that have no
// member-count parameter (update, ranged update, degraded write).
template <int NM = 0, class F>
auto with_shape(int unroll, bool nt, int threads, F&& f) {
  return with_bool(nt, [&](auto ntc) {
    constexpr bool NT = decltype(ntc)::value;
    if (unroll == 2)
      return threads == 256 ? f(Shape<NM, 2, NT, 256>{}) : f(Shape<NM, 2, NT, 64>{});
    return threads == 256 ? f(Shape<NM, 1, NT, 256>{}) : f(Shape<NM, 1, NT, 64>{});
  });
}

// Member counts (k/m) compiled fully unrolled: those of the reference's sweep
// (bm_config.cpp:7-11) and BASELINE.json -- 1, 2, 4, 8, 16, 32; others run the
// generic loop (NM = 0).
template <class F>
auto with_shape(uint64_t nm, int unroll, bool nt, int threads, F&& f) {
  switch (nm) {
    case 1: return with_shape<1>(unroll, nt, threads, f);
    case 2: return with_shape<2>(unroll, nt, threads, f);
    case 4: return with_shape<4>(unroll, nt, threads, f);
    case 8: return with_shape<8>(unroll, nt, threads, f);
    case 16: return with_shape<16>(unroll, nt, threads, f);
    case 32: return with_shape<32>(unroll, nt, threads, f);
    default: return with_shape<0>(unroll, nt, threads, f);
  }
}

// A list that travels in the kernel arguments ships the whole array whatever
// its length, so each kernel that takes one is compiled for three capacities
// and a launch picks the smallest that holds the list (xec_kernels.h).
inline uint32_t arg_items_capacity(uint64_t n) { return n <= 64 ? 64 : n <= 256 ? 256 : 1024; }

template <class F>
auto with_capacity(uint64_t n, F&& f) {
  switch (arg_items_capacity(n)) {
    case 64: return f(std::integral_constant<uint32_t, 64>{});
    case 256: return f(std::integral_constant<uint32_t, 256>{});
    default: return f(std::integral_constant<uint32_t, 1024>{});
  }
}

// The vectored read's table is six words per entry where the lists above are
// one: its capacities stop at 256 entries (6 KiB of arguments).
inline uint32_t readv_capacity(uint64_t n) { return n <= 64 ? 64 : 256; }

template <class F>
auto with_readv_capacity(uint64_t n, F&& f) {
  if (readv_capacity(n) == 64) return f(std::integral_constant<uint32_t, 64>{});
  return f(std::integral_constant<uint32_t, 256>{});
}

// A shard table (xec_encode_shards and its siblings) is k + m 64-bit pointers by
// value in the kernel arguments: two capacities, 64 pointers (512 B) and 256
// (2 KiB), which is also the most shards a call takes.
inline uint32_t shard_tab_capacity(uint64_t n) { return n <= 64 ? 64 : 256; }

template <class F>
auto with_shard_capacity(uint64_t n, F&& f) {
  if (shard_tab_capacity(n) == 64) return f(std::integral_constant<uint32_t, 64>{});
  return f(std::integral_constant<uint32_t, 256>{});
}

}  // namespace xec
