// Host drivers of the matmul on a compressed weight table: floatMatmulRows
// (k_matmulRows, k_matmulFinish, matmul.h) and floatMatmulTile
// (k_matmulTile, matmul_tile.h) of
// include/dietgpu/GpuFloatCodec.h.  A translation unit of its own, as
// reduce.hip is, so that its instances compile beside codec.hip's kernels.
#include <algorithm>
#include <tuple>
#include <type_traits>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "matmul.h"
#include "matmul_tile.h"
#include "profile.h"
#include "sync_arena.h"

namespace dietgpu {

namespace {

// the workgroups of a k_matmulRows or k_matmulTile instance resident on the
// current device at once (cached per device, instance and LDS size)
uint32_t matmulSlots(const void* kernel, uint32_t lds) {
  return cachedPerDevice<uint32_t>(std::make_tuple(kernel, lds), [&](int dev) {
    int cus = 0, perCU = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, dec::kThreads, lds));
    return uint32_t(std::max(1, cus) * std::max(1, perCU));
  });
}

// the plan's grid under dietgpu_set_matmul_grid (0: none)
uint32_t cappedGrid(uint32_t gridX) {
  const uint32_t cap = matmulGrid();
  return cap ? std::min(gridX, cap) : gridX;
}

struct MatmulCall {
  hipStream_t s;
  int pb;
  const uint8_t* archive;
  uint32_t rowWords, numRows;
  const uint8_t* x;  // the pass's first activation row
  uint64_t xRowStrideBytes;
  uint32_t mRows;    // the pass's rows
  float* part;
  uint32_t pieces;
  uint8_t* out;      // the pass's first output row
  uint64_t outRowStride;
  uint8_t* outSuccess;  // the call's first pass writes the status
};

// One pass: k_matmulRows<FT, MT> over the table's blocks, then k_matmulFinish.
template <int FT, int MT, bool OUT32>
void launchMatmulPass(const MatmulCall& c) {
  const uint32_t lds = DecCfg<FT>::ldsBytes(c.pb);
  const uint32_t slots = matmulSlots(reinterpret_cast<const void*>(&k_matmulRows<FT, MT>), lds);
  const MatmulPlan plan = planMatmul(c.numRows, c.rowWords, c.mRows, MT, slots);
  k_matmulRows<FT, MT><<<cappedGrid(plan.gridX), dec::kThreads, lds, c.s>>>(c.archive, c.numRows, c.rowWords, c.x,
                                                                 c.xRowStrideBytes, c.mRows, c.part, c.pieces, c.pb);
  HIP_LAUNCH_CHECK();
  k_matmulFinish<FT, OUT32><<<divUp(c.mRows * c.numRows, uint32_t(dec::kThreads)), dec::kThreads, 0, c.s>>>(
      c.archive, c.numRows, c.rowWords, c.mRows, c.part, c.pieces, c.out, c.outRowStride, c.pb, c.outSuccess);
  HIP_LAUNCH_CHECK();
}

// ... with the smallest instance that holds the pass's rows
template <int FT, bool OUT32>
void launchMatmulPassMT(const MatmulCall& c) {
  static_assert(kMatmulRowsPerPass == 4, "one case per instance");
  if (c.mRows == 1) return launchMatmulPass<FT, 1, OUT32>(c);
  if (c.mRows == 2) return launchMatmulPass<FT, 2, OUT32>(c);
  DG_CHECK(c.mRows <= 4, "no k_matmulRows instance of " << c.mRows << " rows");
  launchMatmulPass<FT, 4, OUT32>(c);
}

}  // namespace

void floatMatmulRows(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                     uint32_t rowWords, uint32_t numRows, const void* x_dev, uint32_t M, uint64_t xRowStrideWords,
                     void* out_dev, bool outIsFp32, uint64_t outRowStrideWords, uint8_t* outSuccess_dev,
                     hipStream_t stream) {
  // every host check before the allocation and the first launch
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kMatmul);
  const int ft = int(config.floatType), pb = config.ansConfig.probBits;
  checkProbBits(pb);
  checkMatmulShape(ft, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords);
  const MatmulPlan plan = planMatmul(numRows, rowWords, M, kMatmulRowsPerPass, 1);
  DG_CHECK(plan.valid, "no matmul plan for " << numRows << " rows of " << rowWords << " words and M = " << M);
  DG_CHECK(archive_dev && x_dev && out_dev, "archive_dev, x_dev and out_dev must not be null");
  checkArchiveAligned(reinterpret_cast<uintptr_t>(archive_dev), 0, 4);
  DG_CHECK(reinterpret_cast<uintptr_t>(x_dev) % 16 == 0, "x_dev must be 16-byte aligned");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (outIsFp32 ? 4 : 2) == 0, "out_dev not aligned to its word size");

  const uint32_t xWord = floatWordBytes(ft), outWord = outIsFp32 ? 4 : 2;
  auto part = res.alloc<uint8_t>(stream, size_t(plan.partialBytes));
  prof::Scope p("matmul_rows", stream);
  auto run = [&](auto tag, auto out32) {
    constexpr int FT = decltype(tag)::value;
    for (uint32_t i = 0; i < plan.numPasses; ++i) {
      const MatmulPass& ps = plan.passes[i];
      const MatmulCall c{stream,
                         pb,
                         static_cast<const uint8_t*>(archive_dev),
                         rowWords,
                         numRows,
                         static_cast<const uint8_t*>(x_dev) + uint64_t(ps.first) * xRowStrideWords * xWord,
                         xRowStrideWords * xWord,
                         ps.count,
                         reinterpret_cast<float*>(part.data()),
                         plan.pieces,
                         static_cast<uint8_t*>(out_dev) + uint64_t(ps.first) * outRowStrideWords * outWord,
                         outRowStrideWords,
                         i == 0 ? outSuccess_dev : nullptr};
      launchMatmulPassMT<FT, decltype(out32)::value>(c);
    }
  };
  constexpr std::true_type f32;
  constexpr std::false_type own;
  switch (config.floatType) {
    case FloatType::kFloat16:
      return outIsFp32 ? run(std::integral_constant<int, 1>{}, f32) : run(std::integral_constant<int, 1>{}, own);
    case FloatType::kBFloat16:
      return outIsFp32 ? run(std::integral_constant<int, 2>{}, f32) : run(std::integral_constant<int, 2>{}, own);
    default:
      return run(std::integral_constant<int, 3>{}, f32);
  }
}

void floatMatmulTile(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                     uint32_t rowWords, uint32_t numRows, const void* x_dev, uint32_t M, uint64_t xRowStrideWords,
                     void* out_dev, bool outIsFp32, uint64_t outRowStrideWords, uint8_t* outSuccess_dev,
                     hipStream_t stream) {
  // every host check before the allocation and the first launch
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kMatmul);
  const int ft = int(config.floatType), pb = config.ansConfig.probBits;
  checkProbBits(pb);
  checkMatmulTileShape(ft, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords);
  DG_CHECK(planMatmulTile(numRows, rowWords, M, 1).valid,
           "no matmul plan for " << numRows << " rows of " << rowWords << " words and M = " << M);
  DG_CHECK(archive_dev && x_dev && out_dev, "archive_dev, x_dev and out_dev must not be null");
  checkArchiveAligned(reinterpret_cast<uintptr_t>(archive_dev), 0, 4);
  DG_CHECK(reinterpret_cast<uintptr_t>(x_dev) % 16 == 0, "x_dev must be 16-byte aligned");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (outIsFp32 ? 4 : 2) == 0, "out_dev not aligned to its word size");

  auto run = [&](auto tag, auto out32) {
    constexpr int FT = decltype(tag)::value;
    const uint32_t lds = mmt::ldsBytes(DecCfg<FT>::ldsBytes(pb));
    const MatmulTilePlan plan = planMatmulTile(
        numRows, rowWords, M, matmulSlots(reinterpret_cast<const void*>(&k_matmulTile<FT>), lds));
    auto part = res.alloc<uint8_t>(stream, size_t(plan.partialBytes));
    float* partial = reinterpret_cast<float*>(part.data());
    const auto* archive = static_cast<const uint8_t*>(archive_dev);
    const auto* x = static_cast<const uint8_t*>(x_dev);
    const uint32_t finishGrid = divUp(M * numRows, uint32_t(dec::kThreads));
    prof::Scope p("matmul_tile", stream);
    k_matmulTile<FT><<<cappedGrid(plan.gridX), dec::kThreads, lds, stream>>>(archive, numRows, rowWords, x, xRowStrideWords * 2, M,
                                                                  partial, plan.pieces, plan.period, pb);
    HIP_LAUNCH_CHECK();
    k_matmulFinish<FT, decltype(out32)::value><<<finishGrid, dec::kThreads, 0, stream>>>(
        archive, numRows, rowWords, M, partial, plan.pieces, static_cast<uint8_t*>(out_dev), outRowStrideWords, pb,
        outSuccess_dev);
    HIP_LAUNCH_CHECK();
  };
  constexpr std::true_type f32;
  constexpr std::false_type own;
  if (config.floatType == FloatType::kFloat16)
    return outIsFp32 ? run(std::integral_constant<int, 1>{}, f32) : run(std::integral_constant<int, 1>{}, own);
  return outIsFp32 ? run(std::integral_constant<int, 2>{}, f32) : run(std::integral_constant<int, 2>{}, own);
}

}  // namespace dietgpu
