// Host driver of the fused reduce's pass and grid rules (planReduce,
// planReduceGrid, dietgpu_fork_amd/csrc/decode_plan.h), built by
// tests/test_reduce_plan.py with a plain C++ compiler.  Every argument
// sextuple "K nsMax partialWords maxBlocks ny slots" prints one line
//   valid numPasses partialBytes gridX chunksPerWG | first count init out ...
// (init / out: 1 when the pass reads / writes the fp32 partial).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "decode_plan.h"

int main(int argc, char** argv) {
  if ((argc - 1) % 6 != 0) {
    std::fprintf(stderr, "usage: %s (K nsMax partialWords maxBlocks ny slots)...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 5 < argc; a += 6) {
    uint64_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = std::strtoull(argv[a + i], nullptr, 10);
    const dietgpu::ReducePlan p = dietgpu::planReduce(uint32_t(v[0]), uint32_t(v[1]), v[2]);
    const dietgpu::DecodePlan g = dietgpu::planReduceGrid(uint32_t(v[3]), 8, uint32_t(v[4]), uint32_t(v[5]));
    std::printf("%d %u %llu %u %u", int(p.valid), p.numPasses, (unsigned long long)p.partialBytes, g.gridX,
                g.chunksPerWG);
    for (uint32_t i = 0; p.valid && i < p.numPasses; ++i)
      std::printf(" %u %u %d %d", p.passes[i].first, p.passes[i].count, int(p.passes[i].initIsPartial),
                  int(p.passes[i].outIsPartial));
    std::printf("\n");
  }
  return 0;
}
