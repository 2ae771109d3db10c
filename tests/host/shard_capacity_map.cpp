// Host-only check of the shard-table capacity mapping of csrc/xec_dispatch.h
// (tests/test_shards_abi.py builds it with ASan + UBSan): with_shard_capacity
// hands its callable the smaller of the two compiled capacities, 64 and 256
// pointers, that holds a table of k + m entries.  A launch that always took 256
// would compute the same bytes with 2 KiB of kernel arguments, and a GPU test
// could see that only through xec_shards_arg_capacity_used.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "xec_dispatch.h"

int main() {
  int failures = 0;
  for (uint64_t n = 1; n <= 256; ++n) {
    const uint32_t cap =
        xec::with_shard_capacity(n, [](auto c) { return (uint32_t) decltype(c)::value; });
    const uint32_t want = n <= 64 ? 64 : 256;
    if (cap != want || cap != xec::shard_tab_capacity(n) || cap < n) {
      ++failures;
      std::fprintf(stderr, "shard_capacity_map: capacity %u for a table of %llu\n", cap,
                   (unsigned long long)n);
    }
  }
  // the list capacities next to it are unchanged
  if (xec::arg_items_capacity(65) != 256 || xec::arg_items_capacity(257) != 1024 ||
      xec::readv_capacity(257) != 256)
    ++failures;
  if (failures != 0) return EXIT_FAILURE;
  std::printf("shard_capacity_map ok: 256 table lengths\n");
  return EXIT_SUCCESS;
}
