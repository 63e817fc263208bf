// Host driver of k_gatherSum's grid rule (planGatherSum,
// dietgpu_fork_amd/csrc/decode_plan.h), built by tests/test_gather_sum_plan.py
// with a plain C++ compiler.  Every argument triple "numBags rowWords slots"
// prints one line "valid tileWords tiles tasks groups gridX".
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "decode_plan.h"

int main(int argc, char** argv) {
  if ((argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: %s (numBags rowWords slots)...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3) {
    const uint32_t numBags = uint32_t(std::strtoull(argv[a], nullptr, 10));
    const uint32_t rowWords = uint32_t(std::strtoull(argv[a + 1], nullptr, 10));
    const uint32_t slots = uint32_t(std::strtoull(argv[a + 2], nullptr, 10));
    const dietgpu::GatherSumPlan p = dietgpu::planGatherSum(numBags, rowWords, slots);
    std::printf("%d %u %u %llu %u %u\n", int(p.valid), p.tileWords, p.tiles, (unsigned long long)p.tasks, p.groups,
                p.gridX);
  }
  return 0;
}
