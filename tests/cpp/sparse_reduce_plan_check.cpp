// Host driver of the fused sparse reduce's plan (planSparseReduce,
// dietgpu_fork_amd/csrc/sparse_plan.h), built by
// tests/test_sparse_reduce_plan.py with a plain C++ compiler.  Every argument
// sextuple "wordBytes nb K nsMax maxCap hasInit" prints one line
//   valid ns rows chunks cblocks gridX denseCapacity listStride listBytes
//   chunkPre blockTot tableBytes partialWords densePtrs sizes denseOk verdict
//   firstN scratchBytes numPasses | first count init out ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "sparse_plan.h"

int main(int argc, char** argv) {
  if ((argc - 1) % 6 != 0) {
    std::fprintf(stderr, "usage: %s (wordBytes nb K nsMax maxCap hasInit)...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 5 < argc; a += 6) {
    uint64_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = std::strtoull(argv[a + i], nullptr, 10);
    const dietgpu::SparseReducePlan p = dietgpu::planSparseReduce(uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]),
                                                                  uint32_t(v[3]), uint32_t(v[4]), v[5] != 0);
    using ull = unsigned long long;
    std::printf("%d %u %u %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u", int(p.valid), p.ns,
                p.rows, p.d.chunks, p.d.cblocks, p.d.gridX, p.d.denseCapacity, ull(p.d.listStride), ull(p.d.listBytes),
                ull(p.d.chunkPre), ull(p.d.blockTot), ull(p.tableBytes), ull(p.partialWords), ull(p.densePtrs),
                ull(p.sizes), ull(p.denseOk), ull(p.verdict), ull(p.firstN), ull(p.scratchBytes),
                p.valid ? p.passes.numPasses : 0u);
    for (uint32_t i = 0; p.valid && i < p.passes.numPasses; ++i)
      std::printf(" %u %u %d %d", p.passes.passes[i].first, p.passes.passes[i].count,
                  int(p.passes.passes[i].initIsPartial), int(p.passes.passes[i].outIsPartial));
    std::printf("\n");
  }
  return 0;
}
