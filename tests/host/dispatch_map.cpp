// Host-only check of csrc/xec_dispatch.h (tests/test_host_sanitizers.py builds
// it with ASan + UBSan): with_shape hands its callable the Shape whose
// constants equal the run-time launch shape, with_capacity the smallest
// capacity that holds the list, with_bool the bool.  A wrong tag still gives
// bit-exact results on the GPU -- the generic NM = 0 kernel for 16 members, an
// NT = false kernel -- so only this program can see one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "xec_dispatch.h"

namespace {

struct Seen {
  int nm, u, t;
  bool nt;
};

int g_failures = 0;

void expect(bool ok, const char* what, uint64_t nm, int unroll, bool nt, int threads) {
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "dispatch_map: %s wrong at nm=%llu unroll=%d nt=%d threads=%d\n", what,
               (unsigned long long)nm, unroll, (int)nt, threads);
}

void check(const Seen& s, int want_nm, uint64_t nm, int unroll, bool nt, int threads) {
  expect(s.nm == want_nm, "NM", nm, unroll, nt, threads);
  expect(s.u == (unroll == 2 ? 2 : 1), "U", nm, unroll, nt, threads);
  expect(s.nt == nt, "NT", nm, unroll, nt, threads);
  expect(s.t == (threads == 256 ? 256 : 64), "T", nm, unroll, nt, threads);
}

}  // namespace

int main() {
  auto see = [](auto sh) {
    using S = decltype(sh);
    return Seen{S::NM, S::U, S::T, S::NT};
  };
  const int unrolls[] = {0, 1, 2, 3}, threads[] = {0, 64, 256};
  int calls = 0;
  for (int unroll : unrolls)
    for (bool nt : {false, true})
      for (int t : threads) {
        for (uint64_t nm = 0; nm <= 70; ++nm, ++calls) {
          const bool compiled = nm == 1 || nm == 2 || nm == 4 || nm == 8 || nm == 16 || nm == 32;
          check(xec::with_shape(nm, unroll, nt, t, see), compiled ? (int)nm : 0, nm, unroll, nt, t);
        }
        // the families without a member count: NM = 0, unused
        check(xec::with_shape(unroll, nt, t, see), 0, 0, unroll, nt, t);
      }
  for (bool b : {false, true})
    if (xec::with_bool(b, [](auto c) { return decltype(c)::value; }) != b) {
      ++g_failures;
      std::fprintf(stderr, "dispatch_map: with_bool(%d)\n", (int)b);
    }
  for (uint64_t n = 1; n <= 1024; ++n) {
    const uint32_t cap = xec::with_capacity(n, [](auto c) { return (uint32_t) decltype(c)::value; });
    const uint32_t want = n <= 64 ? 64 : n <= 256 ? 256 : 1024;
    if (cap != want || cap != xec::arg_items_capacity(n) || cap < n) {
      ++g_failures;
      std::fprintf(stderr, "dispatch_map: capacity %u for a list of %llu\n", cap,
                   (unsigned long long)n);
    }
  }
  if (g_failures != 0) return EXIT_FAILURE;
  std::printf("dispatch_map ok: %d shapes, 1024 list lengths\n", calls);
  return EXIT_SUCCESS;
}
