// Host driver of the fused multi-archive reduce (k_reduce, reduce.h;
// DESIGN.md 5.2g): floatReduceArchives of include/dietgpu/GpuFloatCodec.h, on
// the batch-table rails of the other entry points.  A translation unit of its
// own, so that the k_reduce instances compile beside codec.hip's kernels.
#include <algorithm>
#include <tuple>
#include <vector>

#include "codec_internal.h"
#include "dietgpu/GpuFloatCodec.h"
#include "profile.h"
#include "reduce.h"
#include "sync_arena.h"

namespace dietgpu {

namespace {

// The resident workgroups of a k_reduce instance at `lds` bytes of dynamic
// LDS on the current device; raises the instance's dynamic LDS limit first
// (above 64 KB the launch needs it).  Cached per device, instance and size.
uint32_t reduceSlots(const void* kernel, uint32_t lds) {
  return cachedPerDevice<uint32_t>(std::make_tuple(kernel, lds), [&](int dev) {
    HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    int cus = 0, perCU = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, dec::kThreads, lds));
    return uint32_t(std::max(1, cus) * std::max(1, perCU));
  });
}

struct ReduceCall {
  hipStream_t s;
  const DeviceTables* tabs;
  uint32_t nb, K, maxCapacity;
  int pb;
  uint8_t* outSuccess_dev;
  uint32_t* outSize_dev;
};

// One pass: sources [k0, k0 + NS) of every member on top of `init`, to `out`.
template <int FT, int NS>
void launchReducePass(const ReduceCall& c, const BatchDesc& in, const BatchDesc& init, const BatchDesc& out,
                      uint32_t k0, uint32_t initKind, bool outF32, bool last) {
  using Cfg = RedCfg<NS>;
  const uint32_t lds = Cfg::ldsBytes(c.pb);
  const void* kernel = reinterpret_cast<const void*>(&k_reduce<FT, NS>);
  const uint32_t slots = reduceSlots(kernel, lds);
  forGridYSlices(c.nb, [&](uint32_t y0, uint32_t ny) {
    prof::Scope p("reduce", c.s);
    const DecodePlan plan = planReduceGrid(divUp(c.maxCapacity, kBlockSize), Cfg::kBlocksPerWG, ny, slots);
    RedArgs a;
    a.batchOffset = y0;
    a.nb = c.nb;
    a.K = c.K;
    a.k0 = k0;
    a.pb = c.pb;
    a.chunksPerWG = plan.chunksPerWG;
    a.initKind = initKind;
    a.outF32 = outF32 ? 1u : 0u;
    a.writeStatus = last ? 1u : 0u;
    k_reduce<FT, NS><<<dim3(plan.gridX, ny), dec::kThreads, lds, c.s>>>(kernargTable(c.tabs), in, init, out, a,
                                                                          c.outSuccess_dev, c.outSize_dev);
    HIP_LAUNCH_CHECK();
  });
}

template <int FT>
void launchReducePassNS(uint32_t ns, const ReduceCall& c, const BatchDesc& in, const BatchDesc& init,
                        const BatchDesc& out, uint32_t k0, uint32_t initKind, bool outF32, bool last) {
  static_assert(kReduceMaxNS == 4, "one case per instance");
  switch (ns) {
    case 1: return launchReducePass<FT, 1>(c, in, init, out, k0, initKind, outF32, last);
    case 2: return launchReducePass<FT, 2>(c, in, init, out, k0, initKind, outF32, last);
    case 3: return launchReducePass<FT, 3>(c, in, init, out, k0, initKind, outF32, last);
    case 4: return launchReducePass<FT, 4>(c, in, init, out, k0, initKind, outF32, last);
  }
  DG_CHECK(false, "no k_reduce instance of " << ns << " sources");
}

}  // namespace

void floatReduceArchives(StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch,
                         uint32_t numSources, const void** in, const void** init, FloatType initType, void** out,
                         const uint32_t* outCapacity, FloatType outType, uint8_t* outSuccess_dev,
                         uint32_t* outSize_dev, hipStream_t stream) {
  // every host check before the first allocation, upload or launch
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kReduce);
  const int ft = int(config.floatType);
  checkReduceShape(ft, numSources, init != nullptr, int(initType), int(outType));
  const int pb = config.ansConfig.probBits;
  checkProbBits(pb);
  const uint32_t nb = numInBatch, K = numSources;
  if (nb == 0) return;
  DG_CHECK(uint64_t(nb) * K < (1ull << 32), "numInBatch x numSources must be below 2^32");
  DG_CHECK(in && out && outCapacity, "in, out and outCapacity must not be null");
  const bool outF32 = outType == FloatType::kFloat32;
  const uint32_t initKind = !init ? 0u : (initType == FloatType::kFloat32 ? 2u : 1u);
  const auto ip = addressColumn(in, nb * K), op = addressColumn(out, nb);
  const auto np = init ? addressColumn(init, nb) : std::vector<uint64_t>();
  for (uint32_t i = 0; i < nb * K; ++i) checkArchiveAligned(ip[i], i, 4);
  for (uint32_t i = 0; i < nb; ++i) {
    DG_CHECK(op[i] % (outF32 ? 4 : 2) == 0, "float output " << i << " not aligned to its word size");
    DG_CHECK(!init || np[i] % (initKind == 2 ? 4 : 2) == 0, "init " << i << " not aligned to its word size");
  }
  const SizeColumn cap(outCapacity, nb);
  uint64_t partialWords = 0;
  for (uint32_t x : cap.sizes) partialWords += roundUp64(x, 4);
  const uint32_t hook = reduceMaxSources();
  const uint32_t nsMax = hook >= 1 && hook < uint32_t(kReduceMaxNS) ? hook : uint32_t(kReduceMaxNS);
  const ReducePlan plan = planReduce(K, nsMax, partialWords);
  DG_CHECK(plan.valid, "numSources (" << K << ") must be in 1 .. " << kReduceMaxSources);

  // the fp32 partial of a chained call, and each member's place in it
  auto partial = res.alloc<uint8_t>(stream, size_t(plan.partialBytes));
  std::vector<uint64_t> pp;
  if (plan.numPasses > 1) {
    pp.resize(nb);
    uint64_t at = reinterpret_cast<uint64_t>(partial.data());
    for (uint32_t i = 0; i < nb; ++i) {
      pp[i] = at;
      at += 4 * roundUp64(cap.sizes[i], 4);
    }
  }
  const DeviceTables t = uploadTables(res, stream, {&ip, &op, &np, &pp}, cap.sizes, true);
  const BatchDesc inD = t.tag(BatchDesc::pointers(t.u64[0], nullptr));
  const BatchDesc outD = t.tag(BatchDesc::pointers(t.u64[1], t.u32));
  const BatchDesc initD = t.tag(BatchDesc::pointers(t.u64[2], nullptr));
  const BatchDesc partD = t.tag(BatchDesc::pointers(t.u64[3], t.u32));

  const ReduceCall c{stream, &t, nb, K, cap.maxSize, pb, outSuccess_dev, outSize_dev};
  dispatchFloatType(config.floatType, [&](auto tag) {
    constexpr int FT = decltype(tag)::value;
    if constexpr (FT <= 3) {
      for (uint32_t i = 0; i < plan.numPasses; ++i) {
        const ReducePass& ps = plan.passes[i];
        launchReducePassNS<FT>(ps.count, c, inD, ps.initIsPartial ? partD : initD, ps.outIsPartial ? partD : outD,
                               ps.first, ps.initIsPartial ? 2u : initKind, ps.outIsPartial || outF32,
                               !ps.outIsPartial);
      }
    }
  });
}

}  // namespace dietgpu
