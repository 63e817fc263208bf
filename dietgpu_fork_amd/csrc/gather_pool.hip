// Host driver of the pooled row gather with a mode, weights and a padding
// index: floatGatherRowsPool of include/dietgpu/GpuFloatCodec.h over
// k_gatherPool (gather_pool.h).  A translation unit of its own,
// as reduce.hip and matmul.hip are, so that codec.hip and k_gatherSum compile
// to what they compiled to before.
#include <algorithm>
#include <tuple>
#include <type_traits>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "entry_checks.h"
#include "gather_pool.h"
#include "profile.h"

namespace dietgpu {

namespace {

// the workgroups of a k_gatherPool instance resident on the current device at
// once (cached per device, instance and LDS size)
uint32_t poolSlots(const void* kernel, uint32_t lds) {
  return cachedPerDevice<uint32_t>(std::make_tuple(kernel, lds), [&](int dev) {
    int cus = 0, perCU = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, dec::kThreads, lds));
    return uint32_t(std::max(1, cus) * std::max(1, perCU));
  });
}

struct PoolCall {
  hipStream_t s;
  int pb;
  const void *archive, *idx, *offsets, *weights;
  int64_t padIdx;
  bool idxIs64;
  uint32_t numBags, numIdx, rowWords;
  void* out;
  uint64_t outRowStride;
  uint8_t* outSuccess;
};

// One launch of a persistent grid (planGatherSum, decode_plan.h): nothing is
// uploaded, allocated or read back.
template <int FT, bool OUT32, int MODE, int WT>
void launchPool(const PoolCall& c) {
  const uint32_t lds = DecCfg<FT>::ldsBytes(c.pb);
  const uint32_t slots = poolSlots(reinterpret_cast<const void*>(&k_gatherPool<FT, OUT32, MODE, WT>), lds);
  const GatherSumPlan plan = planGatherSum(c.numBags, c.rowWords, slots);
  prof::Scope p("decode_gather_pool", c.s);
  k_gatherPool<FT, OUT32, MODE, WT><<<plan.gridX, dec::kThreads, lds, c.s>>>(
      static_cast<const uint8_t*>(c.archive), c.idx, c.offsets, c.weights, c.padIdx, c.idxIs64 ? 1u : 0u, c.numBags,
      c.numIdx, c.rowWords, plan.tiles, static_cast<uint8_t*>(c.out), c.outRowStride, c.pb, c.outSuccess);
  HIP_LAUNCH_CHECK();
}

// ... of the instance of the mode and the weights: the reachable combinations
// alone (weights go with the sum; 16-bit weights with a 16-bit archive)
template <int FT, bool OUT32>
void launchPoolMode(const PoolCall& c, PoolMode mode, int wt) {
  if (mode == PoolMode::kMean) return launchPool<FT, OUT32, kPoolMean, kPoolWNone>(c);
  if (mode == PoolMode::kMax) return launchPool<FT, OUT32, kPoolMax, kPoolWNone>(c);
  if (wt == kPoolWNone) return launchPool<FT, OUT32, kPoolSum, kPoolWNone>(c);
  if (wt == kPoolW32) return launchPool<FT, OUT32, kPoolSum, kPoolW32>(c);
  if constexpr (FT != 3) return launchPool<FT, OUT32, kPoolSum, kPoolW16>(c);
  DG_CHECK(false, "no k_gatherPool instance of 16-bit weights for an fp32 archive");
}

}  // namespace

void floatGatherRowsPool(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                         uint32_t rowWords, uint32_t numBags, uint32_t numIdx, const void* idx_dev,
                         const void* offsets_dev, bool idxIs64, PoolMode mode, const void* weights_dev,
                         FloatType weightType, int64_t paddingIdx, void* out_dev, bool outIsFp32,
                         uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  // every host check before the first launch
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kGatherSum);
  const int ft = int(config.floatType), pb = config.ansConfig.probBits;
  checkProbBits(pb);
  checkGatherSumShape(ft, outIsFp32, rowWords, outRowStrideWords);
  const int weightT = weights_dev ? int(weightType) : 0;
  checkGatherPoolMode(ft, int(mode), weightT);
  (void)res;  // nothing is allocated: the call can be captured in a graph
  const GatherSumPlan bound = planGatherSum(numBags, rowWords, 1);
  DG_CHECK(bound.valid, "too many bags: numBags (" << numBags << ") times the " << bound.tiles
                                                   << " column tiles of a row of " << rowWords
                                                   << " words must be below 2^32");
  if (numBags == 0) return;
  DG_CHECK(archive_dev && offsets_dev && out_dev && (idx_dev || numIdx == 0),
           "archive_dev, idx_dev, offsets_dev and out_dev must not be null");
  checkArchiveAligned(reinterpret_cast<uintptr_t>(archive_dev), 0, 4);
  const uintptr_t ib = idxIs64 ? 8 : 4;
  DG_CHECK(reinterpret_cast<uintptr_t>(idx_dev) % ib == 0 && reinterpret_cast<uintptr_t>(offsets_dev) % ib == 0,
           "idx_dev / offsets_dev not aligned to their index size");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (outIsFp32 ? 4 : 2) == 0, "out_dev not aligned to its word size");
  const int wt = weightT == 0 ? kPoolWNone : (weightT == 3 ? kPoolW32 : kPoolW16);
  DG_CHECK(reinterpret_cast<uintptr_t>(weights_dev) % (wt == kPoolW16 ? 2 : 4) == 0,
           "weights_dev not aligned to its word size");

  const PoolCall c{stream,  pb,     archive_dev, idx_dev, offsets_dev, weights_dev,       paddingIdx,
                   idxIs64, numBags, numIdx,     rowWords, out_dev,    outRowStrideWords, outSuccess_dev};
  switch (config.floatType) {
    case FloatType::kFloat16:
      return outIsFp32 ? launchPoolMode<1, true>(c, mode, wt) : launchPoolMode<1, false>(c, mode, wt);
    case FloatType::kBFloat16:
      return outIsFp32 ? launchPoolMode<2, true>(c, mode, wt) : launchPoolMode<2, false>(c, mode, wt);
    default:
      return launchPoolMode<3, true>(c, mode, wt);
  }
}

}  // namespace dietgpu
