// Host driver of the matmul on a sparse weight archive: floatMatmulSparseRows
// of include/dietgpu/GpuFloatCodec.h (k_sparseMatmul, k_sparseMatmulFinish,
// sparse_matmul.h).  A translation unit of its own, as
// matmul.hip is: kernels added to sparse.hip re-scheduled their neighbours
// (DESIGN.md 5.2l), so sparse.hip keeps the kernels it had, and the helpers
// both units need live in sparse_expand.h.
#include <type_traits>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "profile.h"
#include "sparse_matmul.h"
#include "sparse_plan.h"

namespace dietgpu {

namespace {

static_assert(kChunkWords == splan::kChunkWords && kThreads == splan::kThreads && kWaves == splan::kWaves &&
                  smm::kGroupWords == kMatmulSegWords,
              "sparse_plan.h restates the kernels' constants");

struct SparseMatmulCall {
  hipStream_t s;
  const SparseMatmulPlan& plan;
  SparseMatmulArgs a;
  const uint8_t* x;
  uint64_t xRowStrideBytes;
  uint32_t M;
  float* part;
  uint8_t* out;
  uint64_t outRowStride;
  uint8_t* outSuccess;
};

// k_sparseMatmul<FT, MT> for every pass in one launch, then the finish.
template <int FT, bool OUT32>
void launchSparseMatmul(const SparseMatmulCall& c) {
  static_assert(kSparseMatmulMaxMT == 8, "one case per instance");
  const dim3 grid(c.plan.gridX, c.plan.passes);
  auto launch = [&](auto mt) {
    k_sparseMatmul<FT, decltype(mt)::value><<<grid, kThreads, 0, c.s>>>(c.a, c.x, c.xRowStrideBytes, c.M, c.part);
  };
  switch (c.plan.rowsPerPass) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    default: DG_CHECK(false, "no k_sparseMatmul instance of " << c.plan.rowsPerPass << " rows");
  }
  HIP_LAUNCH_CHECK();
  k_sparseMatmulFinish<FT, OUT32><<<c.plan.finishGrid, kThreads, 0, c.s>>>(c.a, c.M, c.part, c.out, c.outRowStride,
                                                                         c.outSuccess);
  HIP_LAUNCH_CHECK();
}

SparseMatmulPlan checkedPlan(const FloatDecompressConfig& config, uint32_t rowWords, uint32_t numRows, uint32_t M,
                             uint64_t xRowStrideWords, bool outIsFp32, uint64_t outRowStrideWords,
                             uint32_t listCapacityWords) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kMatmul);
  const int ft = int(config.floatType);
  checkProbBits(config.ansConfig.probBits);
  checkMatmulShape(ft, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords);
  checkSparseListCapacity(listCapacityWords);
  const SparseMatmulPlan plan = planSparseMatmul(floatWordBytes(ft), numRows, rowWords, M, listCapacityWords);
  DG_CHECK(plan.valid, "no sparse matmul plan for " << numRows << " rows of " << rowWords << " words and M = " << M);
  return plan;
}

}  // namespace

uint64_t floatMatmulSparseScratchBytes(FloatType floatType, uint32_t rowWords, uint32_t numRows, uint32_t M,
                                       uint32_t listCapacityWords) {
  const FloatDecompressConfig config(floatType, ANSCodecConfig(kANSDefaultProbBits), false, false);
  const bool out32 = floatType == FloatType::kFloat32;
  return checkedPlan(config, rowWords, numRows, M, rowWords, out32, numRows, listCapacityWords).scratchBytes;
}

void floatMatmulSparseRows(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                           uint32_t rowWords, uint32_t numRows, const void* x_dev, uint32_t M,
                           uint64_t xRowStrideWords, void* out_dev, bool outIsFp32, uint64_t outRowStrideWords,
                           uint32_t listCapacityWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  // every host check before the first allocation and launch
  const SparseMatmulPlan plan =
      checkedPlan(config, rowWords, numRows, M, xRowStrideWords, outIsFp32, outRowStrideWords, listCapacityWords);
  DG_CHECK(archive_dev && x_dev && out_dev, "archive_dev, x_dev and out_dev must not be null");
  checkArchiveAligned(reinterpret_cast<uintptr_t>(archive_dev), 0, 16);
  DG_CHECK(reinterpret_cast<uintptr_t>(x_dev) % 16 == 0, "x_dev must be 16-byte aligned");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (outIsFp32 ? 4 : 2) == 0, "out_dev not aligned to its word size");

  const hipStream_t s = stream;
  const uint32_t xWord = floatWordBytes(int(config.floatType));
  auto densePtrs = res.alloc<uint64_t>(s, plan.densePtrs);
  auto sizes = res.alloc<uint32_t>(s, plan.sizes);
  auto denseOk = res.alloc<uint8_t>(s, plan.denseOk);
  auto list = res.alloc<uint8_t>(s, plan.listBytes);
  auto chunkPre = res.alloc<uint32_t>(s, plan.chunkPre);
  auto blockTot = res.alloc<uint32_t>(s, plan.blockTot);
  auto part = res.alloc<float>(s, plan.partWords);

  // the chunk counts of the table's chunks and the dense decode of the whole
  // nonzero list, a batch of one: sparseReduceT's sequence (sparse.hip)
  {
    prof::Scope p("sparse_matmul", s);
    k_sparseChunks<<<dim3(plan.cblocks, 1), kThreads, 0, s>>>(BatchDesc::strided(archive_dev, 0, 0), 0, plan.chunks,
                                                             plan.cblocks, densePtrs.data(), sizes.data(),
                                                             chunkPre.data(), blockTot.data());
    HIP_LAUNCH_CHECK();
  }
  DecodeCall dense{res, s};
  dense.nb = 1;
  dense.in = BatchDesc::pointers(densePtrs.data(), nullptr);
  dense.out = BatchDesc::strided(list.data(), plan.listBytes, listCapacityWords);
  dense.maxCapacity = listCapacityWords;
  dense.outSuccess_dev = denseOk.data();
  dense.streamOut = false;  // the matmul reads it, once per pass
  dense.capacityOnly = true;
  floatDecompressDescs(config, dense);

  const SparseMatmulCall c{s,
                           plan,
                           SparseMatmulArgs{static_cast<const uint8_t*>(archive_dev), numRows, rowWords, plan.chunks,
                                            plan.cblocks, chunkPre.data(), blockTot.data(), list.data(),
                                            listCapacityWords, denseOk.data(), plan.pieces},
                           static_cast<const uint8_t*>(x_dev),
                           xRowStrideWords * xWord,
                           M,
                           part.data(),
                           static_cast<uint8_t*>(out_dev),
                           outRowStrideWords,
                           outSuccess_dev};
  prof::Scope p("sparse_matmul", s);
  switch (config.floatType) {
    case FloatType::kFloat16: return outIsFp32 ? launchSparseMatmul<1, true>(c) : launchSparseMatmul<1, false>(c);
    case FloatType::kBFloat16: return outIsFp32 ? launchSparseMatmul<2, true>(c) : launchSparseMatmul<2, false>(c);
    default: return launchSparseMatmul<3, true>(c);
  }
}

}  // namespace dietgpu
