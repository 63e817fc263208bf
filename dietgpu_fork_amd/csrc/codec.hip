// Host orchestration of the MI355X rANS byte codec and float codec.
// Implements the C++ API of include/dietgpu/GpuANSCodec.h and
// include/dietgpu/GpuFloatCodec.h (reference: ans/GpuANSEncode.cu,
// ans/GpuANSDecode.cu, ans/GpuANSInfo.cu, float/GpuFloatCompress.cu,
// float/GpuFloatDecompress.cu, float/GpuFloatInfo.cu).
//
// Launch sequence per call (all stream-ordered, no host sync unless a
// checksum has to be verified):
//   compress:   k_pcompress (single pass, compressPersistent) or
//               k_hist -> a normalisation route -> k_encode (+ k_coalesce
//               for fp64) (compressThreeKernel), as planCompress
//               (compress_plan.h) decides: DESIGN.md 5.1c
//   decompress: k_decode (table build + rANS decode + float join fused)
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <tuple>
#include <type_traits>
#include <vector>

#include "codec_internal.h"
#include "dietgpu/GpuANSCodec.h"
#include "dietgpu/GpuFloatCodec.h"
#include "pcompress.h"
#include "decode.h"
#include "gather.h"
#include "gather_sum.h"
#include "encode.h"
#include "profile.h"

namespace dietgpu {

namespace {
// workgroups of `kernel` resident on the whole device `dev` at once
uint32_t occupancySlots(int dev, const void* kernel, int threads, uint32_t dynLds) {
  int cus = 0, perCU = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, threads, dynLds));
  return uint32_t(std::max(1, cus) * std::max(1, perCU));
}

// ... of the current device (cached per device, kernel and LDS size)
uint32_t residentSlots(const void* kernel, int threads, uint32_t dynLds) {
  return cachedPerDevice<uint32_t>(std::make_tuple(kernel, threads, dynLds),
                                   [&](int dev) { return occupancySlots(dev, kernel, threads, dynLds); });
}

}  // namespace

// ---------------------------------------------------------------------------
// generic drivers
// ---------------------------------------------------------------------------
// Device error words (one pair per device, code object global): [0] elements
// the compressor poisoned (a bounded wait ran out, pcompress.h; their outSize
// is 0), [1] k_pcompress team-barrier fallbacks (a workgroup that counted its
// element from the input after the time budget; archives stay exact).
__device__ uint32_t g_dgErrors[2];

uint32_t* deviceErrorWord() {
  return cachedPerDevice<uint32_t*>(0, [](int) {
    void* p = nullptr;
    HIP_CHECK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_dgErrors)));
    return static_cast<uint32_t*>(p);
  });
}

static uint32_t readErrorWord(uint32_t k, bool reset) {
  uint32_t* p = deviceErrorWord() + k;
  HIP_CHECK(hipDeviceSynchronize());
  uint32_t v = 0;
  HIP_CHECK(hipMemcpy(&v, p, sizeof(v), hipMemcpyDeviceToHost));
  if (reset && v) HIP_CHECK(hipMemset(p, 0, sizeof(v)));
  return v;
}

uint32_t deviceErrorCount(bool reset) { return readErrorWord(0, reset); }
uint32_t barrierFallbackCount(bool reset) { return readErrorWord(1, reset); }

// One slice (elements y0 .. y0 + ny) of the XOR checksums of the first
// in.size(b) bytes of each element, into ck (zeroed by the caller).  The
// float codecs pass word counts: the reference checksums float-word counts
// as byte counts (float/GpuFloatCompress.cuh:709).
static void launchChecksum(const BatchDesc& in, uint32_t y0, uint32_t ny, uint32_t maxSize, uint32_t* ck,
                           hipStream_t s) {
  const uint32_t ckChunk = 1u << 20;
  dim3 g(std::max(1u, divUp(maxSize, ckChunk)), ny);
  k_checksum<<<g, kThreads, 0, s>>>(in, y0, 1, ckChunk, ck);
  HIP_LAUNCH_CHECK();
}

// What the compress rule needs to know of the device: the resident workgroups
// of k_pcompress (its instances have the same resources: one occupancy query)
// and of k_encode's prologue instance, and the CUs (cached per device).
template <int FT>
CompressShape deviceShape() {
  return cachedPerDevice<CompressShape>(0, [](int dev) {
    CompressShape sh;
    int cus = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    sh.cus = uint32_t(std::max(1, cus));
    if constexpr (FloatTraits<FT>::kSegs == 1)
      sh.pcompressSlots =
          occupancySlots(dev, reinterpret_cast<const void*>(&k_pcompress<FT, false, true>), pc::kThreads, 0);
    sh.encodeProSlots = occupancySlots(dev, reinterpret_cast<const void*>(&k_encode<FT, true>), enc::kThreads, 0);
    return sh;
  });
}

// The plan (compress_plan.h) of a compress call on the
// current device, in the current compressPath() mode.
template <int FT>
CompressPlan planCall(uint32_t nb, uint32_t maxSize, bool useChecksum, bool userHist, const PartialHist* pre,
                      bool inAligned16) {
  CompressShape sh = deviceShape<FT>();
  sh.segs = FloatTraits<FT>::kSegs;
  sh.byteCodec = FT == 0;
  sh.nb = nb;
  sh.maxSize = maxSize;
  sh.useChecksum = useChecksum;
  sh.userHist = userHist;
  sh.pre = !pre ? PreHist::kNone : pre->table ? PreHist::kRowsAndTable : PreHist::kRows;
  sh.preRows = pre ? pre->nRows : 0;
  sh.inAligned16 = inAligned16;
  sh.mode = compressPath();
  return planCompress(sh);
}

CompressPlan planCompressCall(int ft, uint32_t nb, uint32_t maxSize, bool useChecksum, bool userHist,
                              bool inAligned16) {
  DG_CHECK(ft >= 0 && ft <= 4 && nb >= 1, "float type 0..4 and at least one element");
  DG_CHECK(!userHist || ft == 0, "only the byte codec takes a histogram");
  if (ft == 0) return planCall<0>(nb, maxSize, useChecksum, userHist, nullptr, inAligned16);
  return dispatchFloatType(FloatType(ft), [&](auto t) {
    return planCall<decltype(t)::value>(nb, maxSize, useChecksum, false, nullptr, inAligned16);
  });
}

// Single-pass compression (k_pcompress, pcompress.h): one generation of
// resident workgroups, plan.teamsPerRound teams of plan.team, pulls items off
// the work queue.
template <int FT, bool kCk, bool kXcd>
void launchPersistent(uint32_t grid, hipStream_t s, const DeviceTables* tabs, const BatchDesc& in,
                      const BatchDesc& out, const PCompArgs& a) {
  k_pcompress<FT, kCk, kXcd><<<grid, pc::kThreads, 0, s>>>(kernargTable(tabs), in, out, a);
  HIP_LAUNCH_CHECK();
}

template <int FT, bool kCk>
void compressPersistent(const CompressCall& c, const CompressPlan& plan) {
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const uint32_t nb = c.nb;
  const bool floatCk = FT != 0 && c.useChecksum;
  DG_CHECK(!plan.tooManyItems, "batch too large for one compress call");

  auto slotMem = res.alloc<uint8_t>(s, size_t(plan.spillSlots) * kSlotDataBytes);
  auto ck = res.alloc<uint32_t>(s, plan.floatCkWords);
  DeviceDescs dd(res, s, floatCk ? c.tabs : nullptr, nb);  // k_checksum's view
  // epoch-tagged state in this stream's persistent arena (no per-call
  // zeroing), one region per kind of word: the dequeue counters (at a fixed
  // place: a call zeroes the next call's), the look-back flags, the tagged
  // partial histograms then the tagged partial byte checksums, the per-team
  // element log.
  const size_t regions[kSyncRegions] = {kSyncCounterBytes, size_t(plan.flagBytes), size_t(plan.partialBytes),
                                        size_t(plan.logBytes), 0};
  SyncLease lease(res, s, regions, /*dequeue=*/true);
  if (floatCk) {
    zeroAsync(ck.data(), sizeof(uint32_t) * nb, s);
    forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) { launchChecksum(dd.map(c.in), y0, ny, c.maxSize, ck.data(), s); });
  }
  PCompArgs a;
  a.ctr = static_cast<uint64_t*>(lease.base[kSyncCounters]);
  a.flags = static_cast<uint64_t*>(lease.base[kSyncFlags]);
  a.part = static_cast<uint32_t*>(lease.base[kSyncPartials]);
  a.partCk = kCk ? a.part + size_t(plan.items) * kNumSymbols : nullptr;
  a.elog = static_cast<uint64_t*>(lease.base[kSyncLog]);
  a.maxR = plan.maxR;
  a.slotSpan = plan.slotSpan;
  a.err = deviceErrorWord();
  a.slots = slotMem.data();
  a.ckIn = floatCk ? ck.data() : nullptr;
  a.outSize = c.outSize_dev;
  a.sparseN = c.sparseN;
  a.items = plan.items;
  a.team = plan.team;
  a.nb = nb;
  a.grid = plan.grid;
  a.teams = plan.teamsPerRound;  // (the kernel divides by nothing but `team`, once per workgroup)
  a.epoch = lease.epoch;
  a.spinCap = spinCap();
  a.fallbackTicks = barrierBudgetTicks();
  a.pb = c.pb;
  a.useChecksum = c.useChecksum;
  prof::Scope p("compress", s);
  if (plan.xcd) launchPersistent<FT, kCk, true>(plan.grid, s, c.tabs, c.in, c.out, a);
  else launchPersistent<FT, kCk, false>(plan.grid, s, c.tabs, c.in, c.out, a);
}

// The three-kernel path: k_hist -> (k_histReduce / k_normalize) -> k_encode
// (+ k_coalesce for fp64), on plain device tables.  plan.normalise names the
// route from the histograms to the encode tables.
template <int FT>
void compressThreeKernel(const CompressCall& c, const CompressPlan& plan) {
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const uint32_t nb = c.nb, maxSize = c.maxSize;
  const int pb = c.pb;
  const bool useChecksum = c.useChecksum;
  const PartialHist* const pre = c.pre;
  constexpr int kSegs = FloatTraits<FT>::kSegs;
  constexpr bool kFused = kSegs == 1;  // k_encode writes the archive itself
  const uint32_t MB = std::max(plan.maxBlocks, 1u);
  const uint32_t chunks = plan.chunks, groups = plan.groups, nW = plan.encodeWGs;
  const bool rawCk = plan.rawCk;
  const Normalise route = plan.normalise;
  const bool reduce2 = route == Normalise::kInReduce;  // first-level sums (k_histReduce)
  DeviceDescs dd(res, s, c.tabs, nb);
  const BatchDesc in = dd.map(c.in), out = dd.map(c.out);

  auto partHist = res.alloc<uint32_t>(s, plan.partHist);
  auto partCk = res.alloc<uint32_t>(s, plan.partCk);
  const uint32_t* chunkRows = pre ? pre->rows : partHist.data();
  auto groupHist = res.alloc<uint32_t>(s, plan.groupHist);
  auto groupCk = res.alloc<uint32_t>(s, plan.groupCk);
  auto ck = res.alloc<uint32_t>(s, plan.ck);
  auto tableMem = res.alloc<uint4>(s, plan.table);
  auto pdfMem = res.alloc<uint16_t>(s, plan.pdf);
  const bool preNorm = route == Normalise::kCaller;
  const uint4* table = preNorm ? pre->table : tableMem.data();
  const uint16_t* pdf = preNorm ? pre->pdf : pdfMem.data();
  auto slots = res.alloc<uint8_t>(s, size_t(plan.slots) * kSlotBytes);
  auto cw = res.alloc<uint32_t>(s, plan.cw);
  // k_encode's look-back flags, the last-arrival counters and (kPrologue) the
  // histogram rows, in this stream's sync arena
  const size_t regions[kSyncRegions] = {0, size_t(plan.lookbackBytes), 0, 0, size_t(plan.arriveBytes), 0};
  SyncLease lease(res, s, regions, false, size_t(plan.rowsBytes));
  uint64_t* const flagsFor = plan.coalesceFromFlags ? static_cast<uint64_t*>(lease.base[kSyncFlags]) : nullptr;
  const bool userHist = FT == 0 && c.hist_dev != nullptr;
  NormArgs na;
  na.in = in;
  na.hist = userHist ? c.hist_dev : (reduce2 ? groupHist.data() : chunkRows);
  na.rows = userHist ? 1u : (reduce2 ? groups : chunks);
  na.pb = pb;
  na.table = tableMem.data();
  na.pdf = pdfMem.data();
  na.partCk = rawCk ? (reduce2 ? groupCk.data() : partCk.data()) : nullptr;
  na.ckRows = reduce2 ? groups : chunks;
  na.ckOut = ck.data();
  na.arrive = nullptr;
  // the last arrival of k_hist or k_histReduce normalises
  NormArgs naFinal = na;
  naFinal.arrive = static_cast<uint32_t*>(lease.base[kSyncArrive]);

  if (FT != 0 && useChecksum) {
    zeroAsync(ck.data(), sizeof(uint32_t) * nb, s);
  }
  // histogram -> (normalise) -> encode per slice of elements
  forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) {
    if (plan.runHist) {
      prof::Scope p("hist", s);
      dim3 g(chunks, ny);
      const NormArgs& nh = route == Normalise::kInHist ? naFinal : na;
      switch (plan.hist) {
        case HistKernel::kRows:
          k_hist<FT, false, true><<<g, kThreads, 0, s>>>(in, y0, nb, plan.chunkWords, chunks,
                                                         static_cast<uint32_t*>(lease.rows[0]), nullptr, na,
                                                         static_cast<uint32_t*>(lease.rows[1]));
          break;
        case HistKernel::kChecksum:
          k_hist<FT, true><<<g, kThreads, 0, s>>>(in, y0, nb, plan.chunkWords, chunks, partHist.data(),
                                                  partCk.data(), nh);
          break;
        case HistKernel::kPlain:
          k_hist<FT, false><<<g, kThreads, 0, s>>>(in, y0, nb, plan.chunkWords, chunks, partHist.data(),
                                                   nullptr, nh);
          break;
      }
      HIP_LAUNCH_CHECK();
    }
    if (FT != 0 && useChecksum) launchChecksum(in, y0, ny, maxSize, ck.data(), s);
    if (route == Normalise::kInReduce) {
      prof::Scope p("normalize", s);
      dim3 g(groups, ny, kSegs);
      k_histReduce<<<g, kThreads, 0, s>>>(y0, nb, chunks, groups, chunkRows, rawCk ? partCk.data() : nullptr,
                                          groupHist.data(), rawCk ? groupCk.data() : nullptr, naFinal, kSegs);
      HIP_LAUNCH_CHECK();
    } else if (route == Normalise::kKernel) {
      prof::Scope p("normalize", s);
      dim3 g(ny, kSegs);
      k_normalize<<<g, kThreads, 0, s>>>(na, y0, nb);
      HIP_LAUNCH_CHECK();
    }
    if (plan.encodeRuns) {
      prof::Scope p("encode", s);
      dim3 g(nW, ny);
      EncTail tail{pdf, ck.data(), c.outSize_dev, flagsFor, nW, pb, useChecksum, spinCap(), deviceErrorWord(),
                   c.sparseN};
      tail.epoch = lease.epoch;
      tail.skew = dispatchSkew();
      if (route == Normalise::kPrologue) {
        tail.rows = static_cast<const uint32_t*>(lease.rows[0]);
        tail.rowsPer = plan.rowsPer;
        tail.pdfOut = pdfMem.data();
        k_encode<FT, true><<<g, enc::kThreads, 0, s>>>(in, out, y0, nb, MB, table, slots.data(), cw.data(), tail);
      } else {
        k_encode<FT><<<g, enc::kThreads, 0, s>>>(in, out, y0, nb, MB, table, slots.data(), cw.data(), tail);
      }
      HIP_LAUNCH_CHECK();
    }
    if (!kFused) {
      prof::Scope p("coalesce", s);
      // blocks per workgroup: 4 (c4 fp64: 2,048 workgroups for the two
      // segments' 4,096 blocks each; 32 gave 256 and a latency-bound copy:
      // coalesce 28.4 -> 16 us at 8, 15.0 at 4, 19.2 at 16, same box)
      const uint32_t bpw = 4;
      dim3 g(std::max(1u, divUp(plan.maxBlocks, bpw)), ny, kSegs);
      CoalPrefix cp;
      cp.flags = flagsFor;
      cp.nW = nW;
      cp.encBlocks = EncCfg<FT>::kBlocksPerWG;
      cp.epoch = lease.epoch;
      cp.err = deviceErrorWord();
      k_coalesce<FT><<<g, kThreads, 0, s>>>(in, out, y0, nb, MB, bpw, slots.data(), cw.data(), pdf, pb,
                                            useChecksum, ck.data(), c.outSize_dev, c.sparseN, cp);
      HIP_LAUNCH_CHECK();
    }
  });
}

// One compress call: planCompress (compress_plan.h) picks the compressor.
template <int FT>
void encodeBatchDevice(const CompressCall& c) {
  checkProbBits(c.pb);
  if (c.nb == 0) return;
  const CompressPlan plan =
      planCall<FT>(c.nb, c.maxSize, c.useChecksum, FT == 0 && c.hist_dev != nullptr, c.pre, c.inAligned16);
  if (!plan.singlePass) return compressThreeKernel<FT>(c, plan);
  if constexpr (FloatTraits<FT>::kSegs == 1) {
    if (plan.rawCk) compressPersistent<FT, FT == 0>(c, plan);
    else compressPersistent<FT, false>(c, plan);
  }
}

// One decode call in any form (DecodeCall, codec_internal.h): the form picks
// the k_decode instance and the profile family, planDecode (decode_plan.h) the
// grid of each slice.
template <int FT>
void decodeBatchDevice(const DecodeCall& c) {
  checkProbBits(c.pb);
  if (c.nb == 0) return;
  using Cfg = DecCfg<FT>;
  const uint32_t lds = Cfg::ldsBytes(c.pb);
  auto run = [&](const char* family, auto nt, auto rng, auto acc) {
    constexpr bool NT = decltype(nt)::value, RNG = decltype(rng)::value;
    constexpr int ACC = decltype(acc)::value;
    constexpr bool kFull = !RNG && ACC == 0;  // the only form with a BAL instance
    const uint32_t maxBlocks = RNG ? c.maxRangeBlocks : divUp(c.maxCapacity, kBlockSize);
    // the resident workgroups of the instance launched (full: of its BAL
    // instance); a range's grid does not depend on them
    const uint32_t slots =
        RNG ? 0
            : residentSlots(reinterpret_cast<const void*>(&k_decode<FT, NT, kFull, RNG, ACC>), dec::kThreads, lds);
    forGridYSlices(c.nb, [&](uint32_t y0, uint32_t ny) {
      prof::Scope p(family, c.s);
      const DecodePlan plan = planDecode(c.form, c.capacityOnly, maxBlocks, Cfg::kBlocksPerWG, ny, slots);
      // BAL is a template parameter: a runtime flag changed the step loop's
      // code (c2 +25 %)
      auto launch = [&](auto bal) {
        k_decode<FT, NT, decltype(bal)::value, RNG, ACC><<<dim3(plan.gridX, ny), dec::kThreads, lds, c.s>>>(
            kernargTable(c.tabs), c.in, c.out, y0, c.pb, plan.chunksPerWG, c.outSuccess_dev, c.outSize_dev);
        HIP_LAUNCH_CHECK();
      };
      if constexpr (kFull) {
        if (plan.balance) return launch(std::true_type{});
      }
      launch(std::false_type{});
    });
  };
  constexpr std::true_type yes;
  constexpr std::false_type no;
  constexpr std::integral_constant<int, 0> store;
  switch (c.form) {
    case DecodeForm::kFull:
      // streaming stores when nobody re-reads the output right away (fp64's
      // 8-dword rows measured slower with them)
      if constexpr (FT != 4) {
        if (c.streamOut) return run("decode", yes, no, store);
      }
      return run("decode", no, no, store);
    case DecodeForm::kRange:
      // plain stores: a range is read right after it is fetched, and its edge
      // rows are partial cache lines
      return run("decode_range", no, yes, store);
    case DecodeForm::kAccumulate:
      // plain stores: the accumulator is read again by the next peer's call
      if constexpr (FT != 0) return run("decode_accumulate", no, no, std::integral_constant<int, 1>{});
      break;
    case DecodeForm::kAccumulateFp32:
      if constexpr (FT == 1 || FT == 2) return run("decode_accumulate", no, no, std::integral_constant<int, 2>{});
      break;
  }
  DG_CHECK(false, "decode form " << int(c.form) << " does not go with float type " << FT);
}

// A row gather (k_gather, gather.h): rows idx_dev[0 .. numIdx)
// of the [R, rowWords] table that the archive holds.  One launch of a
// persistent grid (planGather, decode_plan.h); no host table, no upload, no
// allocation and no read-back, so the call can be captured in a graph.  The
// argument checks come before the device is touched.
template <int FT>
void gatherRowsDevice(int pb, const void* archive_dev, uint32_t rowWords, uint32_t numIdx, const void* idx_dev,
                      bool idxIs64, void* out_dev, uint64_t outRowStrideWords, uint8_t* outSuccess_dev,
                      hipStream_t s) {
  checkProbBits(pb);
  checkGatherRows(rowWords, outRowStrideWords);
  DG_CHECK(planGather(numIdx, rowWords, 1).valid,
           "too many indices: numIdx (" << numIdx << ") times the " << gatherBlocksPerRow(rowWords)
                                        << " blocks a row of " << rowWords << " words touches must be below 2^32");
  if (numIdx == 0) return;
  DG_CHECK(archive_dev && idx_dev && out_dev, "archive_dev, idx_dev and out_dev must not be null");
  checkArchiveAligned(reinterpret_cast<uintptr_t>(archive_dev), 0, 4);
  DG_CHECK(reinterpret_cast<uintptr_t>(idx_dev) % (idxIs64 ? 8 : 4) == 0, "idx_dev not aligned to its index size");
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % sizeof(typename FloatTraits<FT>::WordT) == 0,
           "out_dev not aligned to its word size");
  const uint32_t lds = DecCfg<FT>::ldsBytes(pb);
  const uint32_t slots = residentSlots(reinterpret_cast<const void*>(&k_gather<FT>), dec::kThreads, lds);
  const GatherPlan plan = planGather(numIdx, rowWords, slots);
  prof::Scope p("decode_gather", s);
  k_gather<FT><<<plan.gridX, dec::kThreads, lds, s>>>(static_cast<const uint8_t*>(archive_dev), idx_dev,
                                                      idxIs64 ? 1u : 0u, numIdx, rowWords, plan.K,
                                                      static_cast<uint8_t*>(out_dev), outRowStrideWords, pb,
                                                      outSuccess_dev);
  HIP_LAUNCH_CHECK();
}

// A pooled row gather (k_gatherSum, gather_sum.h): bag b =
// idx_dev[offsets_dev[b] .. offsets_dev[b + 1]) of the [R, rowWords] table that
// the archive holds, summed in fp32 into out row b.  One launch of a persistent
// grid (planGatherSum, decode_plan.h); as gatherRowsDevice, nothing is
// uploaded, allocated or read back, and the argument checks come before the
// device is touched.
template <int FT, bool OUT32>
void gatherRowsSumDevice(int pb, const void* archive_dev, uint32_t rowWords, uint32_t numBags, uint32_t numIdx,
                         const void* idx_dev, const void* offsets_dev, bool idxIs64, void* out_dev,
                         uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t s) {
  // (probability bits, types and the row shape: floatGatherRowsSum's checks)
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
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % (OUT32 ? 4 : 2) == 0, "out_dev not aligned to its word size");
  const uint32_t lds = DecCfg<FT>::ldsBytes(pb);
  const uint32_t slots = residentSlots(reinterpret_cast<const void*>(&k_gatherSum<FT, OUT32>), dec::kThreads, lds);
  const GatherSumPlan plan = planGatherSum(numBags, rowWords, slots);
  prof::Scope p("decode_gather_sum", s);
  k_gatherSum<FT, OUT32><<<plan.gridX, dec::kThreads, lds, s>>>(
      static_cast<const uint8_t*>(archive_dev), idx_dev, offsets_dev, idxIs64 ? 1u : 0u, numBags, numIdx, rowWords,
      plan.tiles, static_cast<uint8_t*>(out_dev), outRowStrideWords, pb, outSuccess_dev);
  HIP_LAUNCH_CHECK();
}

// Verify stored checksums against `unitBytes * out.size(b)` decoded bytes
// (ansDecodeBatch :557-591 / floatDecompressDevice :1077-1112; the float
// codec checksums `capacity` bytes, float words treated as bytes).  Host sync.
std::vector<std::pair<int, std::string>> verifyChecksums(const DecodeCall& c, bool isFloat) {
  std::vector<std::pair<int, std::string>> errs;
  const uint32_t nb = c.nb;
  const hipStream_t s = c.s;
  if (nb == 0) return errs;
  DeviceDescs dd(c.res, s, c.tabs, nb);
  const BatchDesc archives = dd.map(c.in), decoded = dd.map(c.out);
  auto now = c.res.alloc<uint32_t>(s, nb);
  auto old = c.res.alloc<uint32_t>(s, nb);
  zeroAsync(now.data(), sizeof(uint32_t) * nb, s);
  forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) { launchChecksum(decoded, y0, ny, c.maxCapacity, now.data(), s); });
  k_info<<<divUp(nb, 128), 128, 0, s>>>(archives, nb, isFloat, nullptr, nullptr, old.data());
  HIP_LAUNCH_CHECK();
  auto a = now.copyToHost(s);
  auto o = old.copyToHost(s);
  for (uint32_t i = 0; i < nb; ++i) {
    if (a[i] != o[i]) {
      std::ostringstream e;
      e << "Checksum mismatch in batch member " << i << ": expected checksum " << std::hex << o[i]
        << " got " << a[i] << "\n";
      errs.emplace_back(int(i), e.str());
    }
  }
  return errs;
}

// ---------------------------------------------------------------------------
// batch tables of the split-size and range entry points (the pointer ones':
// pointerBatch, batch_tables.h).  `unit` is the size of the codec's unit in
// bytes: 1 for the byte codec, the word size for the float codec (whose
// pointers must be aligned to it).
// ---------------------------------------------------------------------------
// Compress: the elements of `base` -> rows of out_dev.  Decode (archives
// non-null): archives[i] -> the elements of `base`.
static BatchTables splitBatch(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const void* base,
                              const uint32_t* splitSizes, uint32_t unit, const void** archives, void* out_dev,
                              uint32_t outStride) {
  const SplitColumns sc(splitSizes, nb, unit);
  BatchTables b;
  if (archives) {
    const auto ip = addressColumn(archives, nb);
    b.t = uploadTables(res, s, {&ip, &sc.offsets}, sc.sizes, true);
    b.in = b.t.tag(BatchDesc::pointers(b.t.u64[0], nullptr));
    b.out = b.t.tag(BatchDesc::split(base, b.t.u64[1], b.t.u32));
  } else {
    b.t = uploadTables(res, s, {&sc.offsets}, sc.sizes, true);
    b.in = b.t.tag(BatchDesc::split(base, b.t.u64[0], b.t.u32));
    b.out = BatchDesc::strided(out_dev, outStride, 0);
  }
  b.maxSize = sc.maxSize;
  b.inAligned16 = reinterpret_cast<uintptr_t>(base) % 16 == 0 && sc.aligned16;
  return b;
}

// Range decode: words [first[i], first[i] + count[i]) of in[i] -> out[i].
// The `first` column becomes the input descriptor's size column.
static BatchTables rangeBatch(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const void** in,
                              const uint32_t* first, const uint32_t* count, void** out, uint32_t unit) {
  const auto ip = addressColumn(in, nb), op = addressColumn(out, nb);
  for (uint32_t i = 0; i < nb; ++i) {
    DG_CHECK(op[i] % unit == 0, "float output " << i << " not aligned to its word size");
    checkArchiveAligned(ip[i], i, 4);
  }
  const SizeColumn cnt(count, nb), fst(first, nb);
  BatchTables b;
  b.t = uploadTables(res, s, {&ip, &op}, cnt.sizes, true, &fst.sizes);
  b.in = b.t.tag(BatchDesc::pointers(b.t.u64[0], b.t.u32b));
  b.out = b.t.tag(BatchDesc::pointers(b.t.u64[1], b.t.u32));
  // maxSize: the most blocks a range touches (a range past its element's end
  // fails on the device, where the element's size is known)
  for (uint32_t i = 0; i < nb; ++i) {
    const uint64_t end = uint64_t(first[i]) + count[i];
    b.maxSize = std::max(b.maxSize, uint32_t((end + kBlockSize - 1) / kBlockSize - first[i] / kBlockSize));
  }
  return b;
}

static void checkInteriorSplits(const uint32_t* splitSizes, uint32_t nb) {
  for (uint32_t i = 0; i + 1 < nb; ++i)
    DG_CHECK(splitSizes[i] % kANSRequiredAlignment == 0,
             "interior split sizes must be multiples of " << kANSRequiredAlignment);
}

// ... of a rangeBatch, whose maxSize counts blocks
static DecodeCall rangeCall(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const BatchTables& b,
                            uint8_t* outSuccess_dev, uint32_t* outSize_dev) {
  DecodeCall c = decodeCall(res, s, nb, b, outSuccess_dev, outSize_dev);
  c.form = DecodeForm::kRange;
  c.maxCapacity = 0;
  c.maxRangeBlocks = b.maxSize;
  return c;
}

// ---------------------------------------------------------------------------
// ANS byte codec API
// ---------------------------------------------------------------------------
uint32_t getMaxCompressedSize(uint32_t bytes) {
  // ans/GpuANSEncode.cu:13-25 (overhead term evaluated for 4096 *blocks*)
  uint64_t raw = ansOverhead(kBlockSize);
  raw += uint64_t(roundUp(kBlockSize + kBlockSize / 4, 16)) * ((uint64_t(bytes) + kBlockSize - 1) / kBlockSize);
  raw = roundUp64(raw, 16);
  DG_CHECK(raw <= uint64_t(INT32_MAX), "input too large: " << bytes << " bytes");
  return uint32_t(raw);
}

static void ansEncode(const ANSCodecConfig& config, const uint32_t* histogram_dev, CompressCall c) {
  c.pb = config.probBits;
  c.useChecksum = config.useChecksum;
  c.hist_dev = histogram_dev;
  encodeBatchDevice<0>(c);
}

void ansEncodeBatchStride(StackDeviceMemory& res, const ANSCodecConfig& config,
                          uint32_t numInBatch, const void* in_dev, uint32_t inPerBatchSize,
                          uint32_t inPerBatchStride, const uint32_t* histogram_dev,
                          void* out_dev, uint32_t outPerBatchStride,
                          uint32_t* outBatchSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return;
  checkOutAligned(out_dev, "out_dev");
  DG_CHECK(outPerBatchStride % 16 == 0, "outPerBatchStride must be a multiple of 16");
  CompressCall c{res, stream};
  c.nb = numInBatch;
  c.in = BatchDesc::strided(in_dev, inPerBatchStride, inPerBatchSize);
  c.maxSize = inPerBatchSize;
  c.out = BatchDesc::strided(out_dev, outPerBatchStride, 0);
  c.outSize_dev = outBatchSize_dev;
  c.inAligned16 = reinterpret_cast<uintptr_t>(in_dev) % 16 == 0 && inPerBatchStride % 16 == 0;
  ansEncode(config, histogram_dev, c);
}

void ansEncodeBatchPointer(StackDeviceMemory& res, const ANSCodecConfig& config,
                           uint32_t numInBatch, const void** in, const uint32_t* inSize,
                           const uint32_t* histogram_dev, void** out, uint32_t* outSize_dev,
                           hipStream_t stream) {
  if (numInBatch == 0) return;
  const auto b = pointerBatch(res, stream, numInBatch, in, out, inSize, true, 1);
  ansEncode(config, histogram_dev, compressCall(res, stream, numInBatch, b, outSize_dev));
}

void ansEncodeBatchSplitSize(StackDeviceMemory& res, const ANSCodecConfig& config,
                             uint32_t numInBatch, const void* in_dev,
                             const uint32_t* inSplitSizes, const uint32_t* histogram_dev,
                             void* out_dev, uint32_t outStride, uint32_t* outSize_dev,
                             hipStream_t stream) {
  if (numInBatch == 0) return;
  DG_CHECK(reinterpret_cast<uintptr_t>(in_dev) % kANSRequiredAlignment == 0,
           "in_dev must be " << kANSRequiredAlignment << "-byte aligned");
  checkOutAligned(out_dev, "out_dev");
  DG_CHECK(outStride % 16 == 0, "outStride must be a multiple of 16");
  checkInteriorSplits(inSplitSizes, numInBatch);
  const auto b = splitBatch(res, stream, numInBatch, in_dev, inSplitSizes, 1, nullptr, out_dev, outStride);
  ansEncode(config, histogram_dev, compressCall(res, stream, numInBatch, b, outSize_dev));
}

static ANSDecodeStatus ansDecodeCommon(const ANSCodecConfig& config, DecodeCall c) {
  c.pb = config.probBits;
  c.streamOut = !config.useChecksum;
  decodeBatchDevice<0>(c);
  return config.useChecksum ? verifiedStatus<ANSDecodeStatus>(c, false) : ANSDecodeStatus();
}

ANSDecodeStatus ansDecodeBatchStride(StackDeviceMemory& res, const ANSCodecConfig& config,
                                     uint32_t numInBatch, const void* in_dev,
                                     uint32_t inPerBatchStride, void* out_dev,
                                     uint32_t outPerBatchStride, uint32_t outPerBatchCapacity,
                                     uint8_t* outSuccess_dev, uint32_t* outSize_dev,
                                     hipStream_t stream) {
  if (numInBatch == 0) return ANSDecodeStatus();
  DecodeCall c{res, stream};
  c.nb = numInBatch;
  c.in = BatchDesc::strided(in_dev, inPerBatchStride, 0);
  c.out = BatchDesc::strided(out_dev, outPerBatchStride, outPerBatchCapacity);
  c.maxCapacity = outPerBatchCapacity;
  c.outSuccess_dev = outSuccess_dev;
  c.outSize_dev = outSize_dev;
  return ansDecodeCommon(config, c);
}

ANSDecodeStatus ansDecodeBatchPointer(StackDeviceMemory& res, const ANSCodecConfig& config,
                                      uint32_t numInBatch, const void** in, void** out,
                                      const uint32_t* outCapacity, uint8_t* outSuccess_dev,
                                      uint32_t* outSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return ANSDecodeStatus();
  const auto b = pointerBatch(res, stream, numInBatch, in, out, outCapacity, false, 1);
  return ansDecodeCommon(config, decodeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev));
}

ANSDecodeStatus ansDecodeBatchSplitSize(StackDeviceMemory& res, const ANSCodecConfig& config,
                                        uint32_t numInBatch, const void** in, void* out_dev,
                                        const uint32_t* outSplitSizes, uint8_t* outSuccess_dev,
                                        uint32_t* outSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return ANSDecodeStatus();
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % kANSRequiredAlignment == 0,
           "out_dev must be " << kANSRequiredAlignment << "-byte aligned");
  checkInteriorSplits(outSplitSizes, numInBatch);
  const auto b = splitBatch(res, stream, numInBatch, out_dev, outSplitSizes, 1, in, nullptr, 0);
  return ansDecodeCommon(config, decodeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev));
}

void ansDecodeBatchRange(StackDeviceMemory& res, const ANSCodecConfig& config, uint32_t numInBatch,
                         const void** in, const uint32_t* first, const uint32_t* count, void** out,
                         uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  checkNoChecksum(config.useChecksum, PartialDecode::kRange);
  if (numInBatch == 0) return;
  const auto b = rangeBatch(res, stream, numInBatch, in, first, count, out, 1);
  DecodeCall c = rangeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev);
  c.pb = config.probBits;
  decodeBatchDevice<0>(c);
}

void ansGatherRows(StackDeviceMemory& res, const ANSCodecConfig& config, const void* archive_dev,
                   uint32_t rowWords, uint32_t numIdx, const void* idx_dev, bool idxIs64, void* out_dev,
                   uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  checkNoChecksum(config.useChecksum, PartialDecode::kGather);
  (void)res;  // nothing is allocated: the call can be captured in a graph
  gatherRowsDevice<0>(config.probBits, archive_dev, rowWords, numIdx, idx_dev, idxIs64, out_dev, outRowStrideWords,
                      outSuccess_dev, stream);
}

// k_info over a device array of archive addresses (the byte codec has no
// type word)
static void launchInfo(const void** in_dev, uint32_t nb, bool isFloat, uint32_t* outSizes_dev,
                       uint32_t* outTypes_dev, uint32_t* outChecksum_dev, hipStream_t stream) {
  if (nb == 0 || (!outSizes_dev && !outTypes_dev && !outChecksum_dev)) return;
  auto inD = BatchDesc::pointers(reinterpret_cast<const uint64_t*>(in_dev), nullptr);
  k_info<<<divUp(nb, 128), 128, 0, stream>>>(inD, nb, isFloat, outSizes_dev, outTypes_dev, outChecksum_dev);
  HIP_LAUNCH_CHECK();
}

// ... over a host array: one upload
static void uploadAndLaunchInfo(StackDeviceMemory& res, const void** in, uint32_t nb, bool isFloat,
                                uint32_t* outSizes_dev, uint32_t* outTypes_dev, uint32_t* outChecksum_dev,
                                hipStream_t stream) {
  if (nb == 0 || (!outSizes_dev && !outTypes_dev && !outChecksum_dev)) return;
  const auto ip = addressColumn(in, nb);
  const auto t = uploadTables(res, stream, {&ip}, {});
  launchInfo(reinterpret_cast<const void**>(const_cast<uint64_t*>(t.u64[0])), nb, isFloat, outSizes_dev,
             outTypes_dev, outChecksum_dev, stream);
}

void ansGetCompressedInfoDevice(StackDeviceMemory& res, const void** in_dev, uint32_t numInBatch,
                                uint32_t* outSizes_dev, uint32_t* outChecksum_dev,
                                hipStream_t stream) {
  launchInfo(in_dev, numInBatch, false, outSizes_dev, nullptr, outChecksum_dev, stream);
}

void ansGetCompressedInfo(StackDeviceMemory& res, const void** in, uint32_t numInBatch,
                          uint32_t* outSizes_dev, uint32_t* outChecksum_dev, hipStream_t stream) {
  uploadAndLaunchInfo(res, in, numInBatch, false, outSizes_dev, nullptr, outChecksum_dev, stream);
}

// ---------------------------------------------------------------------------
// float codec API
// ---------------------------------------------------------------------------
// float/GpuFloatCompress.cu:23-47.  The result is a u32 there too and may
// exceed INT32_MAX (the reference's published batch-1 sweep compresses
// 1.07e9 bf16 words, README.md:118: 2.41e9 bytes of capacity); every archive
// offset is unsigned 32-bit, so anything up to UINT32_MAX is accepted.  The
// raw section is sized in 64 bits here so that an fp32 / fp64 size past the
// u32 range is refused instead of wrapping.
uint32_t getMaxFloatCompressedSize(FloatType ft, uint32_t size) {
  DG_CHECK(ft != FloatType::kUndefined && uint32_t(ft) <= 4, "bad float type");
  uint64_t base = uint64_t(kFloatHeaderBytes) + getMaxCompressedSize(size) + floatRawBytes(int(ft), uint64_t(size));
  if (ft == FloatType::kFloat64) base += getMaxCompressedSize(size);
  DG_CHECK(base <= uint64_t(UINT32_MAX), "input too large: " << size << " float words");
  return uint32_t(base);
}

void floatCompressDescs(const FloatCompressConfig& config, CompressCall c) {
  checkFloatConfig(config);
  c.pb = config.ansConfig.probBits;
  c.useChecksum = config.useChecksum;
  c.hist_dev = nullptr;
  dispatchFloatType(config.floatType, [&](auto ft) { encodeBatchDevice<decltype(ft)::value>(c); });
}

FloatDecompressStatus floatDecompressDescs(const FloatDecompressConfig& config, DecodeCall c) {
  checkFloatConfig(config);
  c.pb = config.ansConfig.probBits;
  const bool verify = c.form == DecodeForm::kFull && config.useChecksum;
  // streaming output stores unless the output is read back (checksum)
  c.streamOut = c.streamOut && !verify;
  dispatchFloatType(config.floatType, [&](auto ft) { decodeBatchDevice<decltype(ft)::value>(c); });
  return verify ? verifiedStatus<FloatDecompressStatus>(c, true) : FloatDecompressStatus();
}

void floatCompress(StackDeviceMemory& res, const FloatCompressConfig& config, uint32_t numInBatch,
                   const void** in, const uint32_t* inSize, void** out, uint32_t* outSize_dev,
                   hipStream_t stream) {
  if (numInBatch == 0) return;
  checkFloatConfig(config);
  const auto b = pointerBatch(res, stream, numInBatch, in, out, inSize, true, floatWordBytes(int(config.floatType)));
  floatCompressDescs(config, compressCall(res, stream, numInBatch, b, outSize_dev));
}

void floatCompressSplitSize(StackDeviceMemory& res, const FloatCompressConfig& config,
                            uint32_t numInBatch, const void* in_dev, const uint32_t* inSplitSizes,
                            void* out_dev, uint32_t outStride, uint32_t* outSize_dev,
                            hipStream_t stream) {
  if (numInBatch == 0) return;
  checkFloatConfig(config);
  checkOutAligned(out_dev, "out_dev");
  DG_CHECK(outStride % 16 == 0, "outStride must be a multiple of 16");
  const uint32_t ws = floatWordBytes(int(config.floatType));
  DG_CHECK(reinterpret_cast<uintptr_t>(in_dev) % ws == 0, "in_dev not word aligned");
  const auto b = splitBatch(res, stream, numInBatch, in_dev, inSplitSizes, ws, nullptr, out_dev, outStride);
  floatCompressDescs(config, compressCall(res, stream, numInBatch, b, outSize_dev));
}

void floatCompressBatchStride(StackDeviceMemory& res, const FloatCompressConfig& config,
                              uint32_t numInBatch, const void* in_dev, uint32_t inPerBatchWords,
                              uint64_t inPerBatchStrideBytes, void* out_dev,
                              uint64_t outPerBatchStrideBytes, uint32_t* outSize_dev,
                              hipStream_t stream) {
  if (numInBatch == 0) return;
  checkOutAligned(out_dev, "out_dev");
  DG_CHECK(outPerBatchStrideBytes % 16 == 0, "out stride must be a multiple of 16");
  CompressCall c{res, stream};
  c.nb = numInBatch;
  c.in = BatchDesc::strided(in_dev, inPerBatchStrideBytes, inPerBatchWords);
  c.maxSize = inPerBatchWords;
  c.out = BatchDesc::strided(out_dev, outPerBatchStrideBytes, 0);
  c.outSize_dev = outSize_dev;
  c.inAligned16 = reinterpret_cast<uintptr_t>(in_dev) % 16 == 0 && inPerBatchStrideBytes % 16 == 0;
  floatCompressDescs(config, c);
}

FloatDecompressStatus floatDecompress(StackDeviceMemory& res, const FloatDecompressConfig& config,
                                      uint32_t numInBatch, const void** in, void** out,
                                      const uint32_t* outCapacity, uint8_t* outSuccess_dev,
                                      uint32_t* outSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return FloatDecompressStatus();
  checkFloatConfig(config);
  const auto b =
      pointerBatch(res, stream, numInBatch, in, out, outCapacity, false, floatWordBytes(int(config.floatType)));
  return floatDecompressDescs(config, decodeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev));
}

void floatDecompressRange(StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch,
                          const void** in, const uint32_t* first, const uint32_t* count, void** out,
                          uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kRange);
  if (numInBatch == 0) return;
  const auto b = rangeBatch(res, stream, numInBatch, in, first, count, out, floatWordBytes(int(config.floatType)));
  floatDecompressDescs(config, rangeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev));
}

void floatGatherRows(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                     uint32_t rowWords, uint32_t numIdx, const void* idx_dev, bool idxIs64, void* out_dev,
                     uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kGather);
  (void)res;  // nothing is allocated: the call can be captured in a graph
  dispatchFloatType(config.floatType, [&](auto ft) {
    gatherRowsDevice<decltype(ft)::value>(config.ansConfig.probBits, archive_dev, rowWords, numIdx, idx_dev, idxIs64,
                                          out_dev, outRowStrideWords, outSuccess_dev, stream);
  });
}

void floatGatherRowsSum(StackDeviceMemory& res, const FloatDecompressConfig& config, const void* archive_dev,
                        uint32_t rowWords, uint32_t numBags, uint32_t numIdx, const void* idx_dev,
                        const void* offsets_dev, bool idxIs64, void* out_dev, bool outIsFp32,
                        uint64_t outRowStrideWords, uint8_t* outSuccess_dev, hipStream_t stream) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kGatherSum);
  checkProbBits(config.ansConfig.probBits);
  checkGatherSumShape(int(config.floatType), outIsFp32, rowWords, outRowStrideWords);
  (void)res;  // nothing is allocated: the call can be captured in a graph
  const int pb = config.ansConfig.probBits;
  auto run = [&](auto ft, auto out32) {
    gatherRowsSumDevice<decltype(ft)::value, decltype(out32)::value>(pb, archive_dev, rowWords, numBags, numIdx,
                                                                     idx_dev, offsets_dev, idxIs64, out_dev,
                                                                     outRowStrideWords, outSuccess_dev, stream);
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

void floatDecompressAccumulate(StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch,
                               const void** in, void** acc, const uint32_t* accCapacity, FloatType accType,
                               uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  accumulateEntry(res, config, numInBatch, in, acc, accCapacity, accType, outSuccess_dev, outSize_dev, stream, 4,
                  [&](const DecodeCall& c) { floatDecompressDescs(config, c); });
}

FloatDecompressStatus floatDecompressSplitSize(StackDeviceMemory& res,
                                               const FloatDecompressConfig& config,
                                               uint32_t numInBatch, const void** in, void* out_dev,
                                               const uint32_t* outSplitSizes,
                                               uint8_t* outSuccess_dev, uint32_t* outSize_dev,
                                               hipStream_t stream) {
  if (numInBatch == 0) return FloatDecompressStatus();
  checkFloatConfig(config);
  const uint32_t ws = floatWordBytes(int(config.floatType));
  DG_CHECK(reinterpret_cast<uintptr_t>(out_dev) % ws == 0, "out_dev not word aligned");
  const auto b = splitBatch(res, stream, numInBatch, out_dev, outSplitSizes, ws, in, nullptr, 0);
  return floatDecompressDescs(config, decodeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev));
}

FloatDecompressStatus floatDecompressBatchStride(StackDeviceMemory& res,
                                                 const FloatDecompressConfig& config,
                                                 uint32_t numInBatch, const void* in_dev,
                                                 uint64_t inPerBatchStrideBytes, void* out_dev,
                                                 uint64_t outPerBatchStrideBytes,
                                                 uint32_t outPerBatchCapacityWords,
                                                 uint8_t* outSuccess_dev, uint32_t* outSize_dev,
                                                 hipStream_t stream) {
  if (numInBatch == 0) return FloatDecompressStatus();
  DecodeCall c{res, stream};
  c.nb = numInBatch;
  c.in = BatchDesc::strided(in_dev, inPerBatchStrideBytes, 0);
  c.out = BatchDesc::strided(out_dev, outPerBatchStrideBytes, outPerBatchCapacityWords);
  c.maxCapacity = outPerBatchCapacityWords;
  c.outSuccess_dev = outSuccess_dev;
  c.outSize_dev = outSize_dev;
  return floatDecompressDescs(config, c);
}

void floatGetCompressedInfoDevice(StackDeviceMemory& res, const void** in_dev, uint32_t numInBatch,
                                  uint32_t* outSizes_dev, uint32_t* outTypes_dev,
                                  uint32_t* outChecksum_dev, hipStream_t stream) {
  launchInfo(in_dev, numInBatch, true, outSizes_dev, outTypes_dev, outChecksum_dev, stream);
}

void floatGetCompressedInfo(StackDeviceMemory& res, const void** in, uint32_t numInBatch,
                            uint32_t* outSizes_dev, uint32_t* outTypes_dev,
                            uint32_t* outChecksum_dev, hipStream_t stream) {
  uploadAndLaunchInfo(res, in, numInBatch, true, outSizes_dev, outTypes_dev, outChecksum_dev, stream);
}

}  // namespace dietgpu
