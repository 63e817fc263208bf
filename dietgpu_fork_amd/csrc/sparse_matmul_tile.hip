// Host driver of the matmul on a sparse weight archive through the matrix
// pipe: floatMatmulSparseTile of include/dietgpu/GpuFloatCodec.h
// (k_sparseChunkOffsets, k_sparseMatmulTile, k_sparseMatmulTileFinish,
// sparse_matmul_tile.h).  A translation unit of its own, as
// sparse_matmul.hip is: the kernels of the other units keep
// their schedules.
#include <type_traits>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "profile.h"
#include "sparse_matmul_tile.h"
#include "sparse_plan.h"

namespace dietgpu {

namespace {

static_assert(kChunkWords == splan::kChunkWords && kThreads == splan::kThreads && kWaves == splan::kWaves &&
                  smm::kGroupWords == kMatmulSegWords && smt::kBlockRows == kSparseTileRows &&
                  smt::kSliceWords == kSparseTileWords && kMatmulMaxRows == 16 * kWaves,
              "sparse_plan.h restates the kernels' constants; a wave per 16 rows of x");

struct SparseMatmulTileCall {
  hipStream_t s;
  const SparseMatmulTilePlan& plan;
  SparseMatmulTileArgs a;
  const uint8_t* x;
  uint64_t xRowStrideBytes;
  uint32_t M;
  float* part;
  uint8_t* out;
  uint64_t outRowStride;
  uint8_t* outSuccess;
};

template <int FT, bool OUT32>
void launchSparseMatmulTile(const SparseMatmulTileCall& c) {
  k_sparseMatmulTile<FT><<<c.plan.tasks, kThreads, 0, c.s>>>(c.a, c.x, c.xRowStrideBytes, c.M, c.part);
  HIP_LAUNCH_CHECK();
  k_sparseMatmulTileFinish<FT, OUT32><<<c.plan.finishGrid, kThreads, 0, c.s>>>(c.a, c.M, c.part, c.out,
                                                                               c.outRowStride, c.outSuccess);
  HIP_LAUNCH_CHECK();
}

SparseMatmulTilePlan checkedPlan(const FloatDecompressConfig& config, uint32_t rowWords, uint32_t numRows, uint32_t M,
                                 uint64_t xRowStrideWords, bool outIsFp32, uint64_t outRowStrideWords,
                                 uint32_t listCapacityWords) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kMatmul);
  const int ft = int(config.floatType);
  checkProbBits(config.ansConfig.probBits);
  checkMatmulSparseTileShape(ft, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords,
                             listCapacityWords);
  const SparseMatmulTilePlan plan = planSparseMatmulTile(floatWordBytes(ft), numRows, rowWords, M, listCapacityWords);
  DG_CHECK(plan.valid,
           "no tiled sparse matmul plan for " << numRows << " rows of " << rowWords << " words and M = " << M);
  return plan;
}

}  // namespace

uint64_t floatMatmulSparseTileScratchBytes(FloatType floatType, uint32_t rowWords, uint32_t numRows, uint32_t M,
                                           uint32_t listCapacityWords) {
  const FloatDecompressConfig config(floatType, ANSCodecConfig(kANSDefaultProbBits), false, false);
  return checkedPlan(config, rowWords, numRows, M, rowWords, false, numRows, listCapacityWords).scratchBytes;
}

void floatMatmulSparseTile(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                           uint32_t rowWords, uint32_t numRows, const void* x_dev, uint32_t M,
                           uint64_t xRowStrideWords, void* out_dev, bool outIsFp32, uint64_t outRowStrideWords,
                           uint32_t listCapacityWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  // every host check before the first allocation and launch
  const SparseMatmulTilePlan plan =
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
  auto chunkOff = res.alloc<uint32_t>(s, plan.chunkOff);
  auto part = res.alloc<float>(s, plan.partWords);

  // the chunk counts of the table's chunks, their list offsets, and the dense
  // decode of the whole nonzero list, a batch of one (floatMatmulSparseRows')
  {
    prof::Scope p("sparse_matmul", s);
    k_sparseChunks<<<dim3(plan.cblocks, 1), kThreads, 0, s>>>(BatchDesc::strided(archive_dev, 0, 0), 0, plan.chunks,
                                                             plan.cblocks, densePtrs.data(), sizes.data(),
                                                             chunkPre.data(), blockTot.data());
    HIP_LAUNCH_CHECK();
    k_sparseChunkOffsets<<<plan.cblocks, kThreads, 0, s>>>(chunkPre.data(), blockTot.data(), plan.chunks,
                                                          chunkOff.data());
    HIP_LAUNCH_CHECK();
  }
  DecodeCall dense{res, s};
  dense.nb = 1;
  dense.in = BatchDesc::pointers(densePtrs.data(), nullptr);
  dense.out = BatchDesc::strided(list.data(), plan.listBytes, listCapacityWords);
  dense.maxCapacity = listCapacityWords;
  dense.outSuccess_dev = denseOk.data();
  dense.streamOut = false;  // the tiles read it next
  dense.capacityOnly = true;
  floatDecompressDescs(config, dense);

  const SparseMatmulTileCall c{
      s,
      plan,
      SparseMatmulTileArgs{SparseMatmulArgs{static_cast<const uint8_t*>(archive_dev), numRows, rowWords, plan.chunks,
                                            plan.cblocks, chunkPre.data(), blockTot.data(), list.data(),
                                            listCapacityWords, denseOk.data(), plan.slices},
                           chunkOff.data()},
      static_cast<const uint8_t*>(x_dev),
      xRowStrideWords * xWord,
      M,
      part.data(),
      static_cast<uint8_t*>(out_dev),
      outRowStrideWords,
      outSuccess_dev};
  prof::Scope p("sparse_matmul", s);
  if (config.floatType == FloatType::kFloat16)
    return outIsFp32 ? launchSparseMatmulTile<1, true>(c) : launchSparseMatmulTile<1, false>(c);
  return outIsFp32 ? launchSparseMatmulTile<2, true>(c) : launchSparseMatmulTile<2, false>(c);
}

}  // namespace dietgpu
