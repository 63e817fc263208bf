// Host driver of the grouped matmul on compressed expert tables:
// floatMatmulGrouped (k_matmulGroupPlan, k_matmulTileGrouped,
// k_matmulFinishGrouped, matmul_grouped.h) of
// include/dietgpu/GpuFloatCodec.h.  A translation unit of its own, beside
// matmul.hip: the kernels of floatMatmulRows and floatMatmulTile compile as
// they did before this one existed.
#include <algorithm>
#include <tuple>
#include <type_traits>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "matmul_grouped.h"
#include "profile.h"
#include "sync_arena.h"

namespace dietgpu {

namespace {

// the workgroups of a k_matmulTileGrouped instance resident on the current
// device at once (cached per device, instance and LDS size)
uint32_t groupedSlots(const void* kernel, uint32_t lds) {
  return cachedPerDevice<uint32_t>(std::make_tuple(kernel, lds), [&](int dev) {
    int cus = 0, perCU = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, dec::kThreads, lds));
    return uint32_t(std::max(1, cus) * std::max(1, perCU));
  });
}

}  // namespace

void floatMatmulGrouped(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archives_dev,
                        uint32_t numExperts, uint32_t rowWords, uint32_t numRows, const void* x_dev, uint32_t T,
                        uint64_t xRowStrideWords, const void* offsets_dev, bool offsetsAre64, void* out_dev,
                        bool outIsFp32, uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  // every host check before the allocation and the first launch
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kMatmul);
  const int ft = int(config.floatType), pb = config.ansConfig.probBits;
  checkProbBits(pb);
  checkMatmulGroupedShape(ft, outIsFp32, rowWords, numRows, numExperts, T, xRowStrideWords, outRowStrideWords);
  DG_CHECK(archives_dev && x_dev && offsets_dev && out_dev,
           "archives_dev, x_dev, offsets_dev and out_dev must not be null");
  DG_CHECK(reinterpret_cast<uintptr_t>(archives_dev) % 8 == 0, "archives_dev must be 8-byte aligned");
  DG_CHECK(reinterpret_cast<uintptr_t>(offsets_dev) % (offsetsAre64 ? 8 : 4) == 0,
           "offsets_dev not aligned to its entry size");
  DG_CHECK(reinterpret_cast<uintptr_t>(x_dev) % 16 == 0, "x_dev must be 16-byte aligned");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (outIsFp32 ? 4 : 2) == 0, "out_dev not aligned to its word size");

  auto run = [&](auto tag, auto out32) {
    constexpr int FT = decltype(tag)::value;
    const uint32_t lds = mmg::ldsBytes(DecCfg<FT>::ldsBytes(pb));
    const MatmulGroupedPlan plan =
        planMatmulGrouped(numExperts, numRows, rowWords, T,
                          groupedSlots(reinterpret_cast<const void*>(&k_matmulTileGrouped<FT>), lds), matmulGroupedGrid());
    auto scratch = res.alloc<uint8_t>(stream, size_t(plan.partialBytes));
    uint8_t* base = scratch.data();
    auto* head = reinterpret_cast<uint32_t*>(base);
    uint8_t* status = base + plan.statusOffset;
    auto* entries = reinterpret_cast<u32x4*>(base + plan.entriesOffset);
    auto* partial = reinterpret_cast<float*>(base + plan.partOffset);
    const auto* archives = static_cast<const uint64_t*>(archives_dev);
    const auto* x = static_cast<const uint8_t*>(x_dev);
    const uint32_t is64 = offsetsAre64 ? 1 : 0;
    prof::Scope p("matmul_grouped", stream);
    k_matmulGroupPlan<FT><<<1, dec::kThreads, 0, stream>>>(archives, numExperts, offsets_dev, is64, T, numRows,
                                                           rowWords, pb, head, status, entries, outSuccess_dev);
    HIP_LAUNCH_CHECK();
    k_matmulTileGrouped<FT><<<plan.gridX, dec::kThreads, lds, stream>>>(
        archives, numRows, rowWords, x, xRowStrideWords * 2, head, entries, partial, plan.pieces, plan.period,
        plan.groups, pb);
    HIP_LAUNCH_CHECK();
    k_matmulFinishGrouped<FT, decltype(out32)::value>
        <<<divUp(T * numRows, uint32_t(dec::kThreads)), dec::kThreads, 0, stream>>>(
            offsets_dev, is64, numExperts, T, numRows, rowWords, head, status, partial, plan.pieces,
            static_cast<uint8_t*>(out_dev), outRowStrideWords);
    HIP_LAUNCH_CHECK();
  };
  constexpr std::true_type f32;
  constexpr std::false_type own;
  if (config.floatType == FloatType::kFloat16)
    return outIsFp32 ? run(std::integral_constant<int, 1>{}, f32) : run(std::integral_constant<int, 1>{}, own);
  return outIsFp32 ? run(std::integral_constant<int, 2>{}, f32) : run(std::integral_constant<int, 2>{}, own);
}

uint64_t floatMatmulGroupedScratchBytes(uint32_t numExperts, uint32_t rowWords, uint32_t numRows, uint32_t T) {
  const MatmulGroupedPlan plan = planMatmulGrouped(numExperts, numRows, rowWords, T, 1, 0);
  DG_CHECK(plan.valid, "no grouped matmul plan for " << numExperts << " tables of " << numRows << " rows of "
                                                     << rowWords << " words and T = " << T);
  return plan.partialBytes;
}

}  // namespace dietgpu
