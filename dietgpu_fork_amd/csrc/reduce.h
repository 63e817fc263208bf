// Fused multi-archive reduce for gfx950: decode the same
// blocks of NS float archives side by side and sum them in registers,
//   out[i] = round((...((init[i] + x_1[i]) + x_2[i]) + ...) + x_NS[i]),
// every add one fp32 add in source order, `init` read once, `out` written
// once, no accumulator in HBM between the sources.
//
// Built from decode.h's pieces: a wave takes a block pair and holds NS chains
// (DStream, ring set, segment buffer, decode table), one per source, stepped
// phase-ordered by decStepAll / decSteps as fp64's two chains are.  All
// sources hold the same n, so the pair's block sizes, segments and masks are
// shared.  After a segment's 8 steps each lane joins its 8 words of every
// source (Join::words on the source's raw bytes, loaded a segment ahead) and
// adds them into 8 fp32 registers on top of the init words (also loaded a
// segment ahead), then stores them once.
//
// Alignment is per pointer: a source that is not 16 B-aligned reads its raw
// bytes with dword loads and its compressed words with 2 B loads (archives are
// 4 B-aligned); `init` / `out` that are not 16 B-aligned, and the chunk that
// holds the element's tail, go word by word.  The arithmetic is the same
// registers either way.
#pragma once

#include "decode.h"

namespace dietgpu {

// One launch reduces at most this many sources (LDS per
// workgroup is NS x (table + rings + segment buffer)).
constexpr int kReduceMaxNS = 4;

template <int NS>
struct RedCfg {
  static constexpr int kBlocksPerWave = 2;
  static constexpr int kBlocksPerWG = dec::kWaves * kBlocksPerWave;
  static constexpr uint32_t kHalfStreams = dec::kWaves * NS * 2;
  static constexpr uint32_t kRingBytes = kHalfStreams * dec::kRing * 2;
  static constexpr uint32_t kSegBytes = kHalfStreams * dec::kSegWords * 2;
  __host__ __device__ static constexpr uint32_t lutBytes(int pb) { return NS * (8u << pb); }
  __host__ __device__ static constexpr uint32_t ldsBytes(int pb) { return lutBytes(pb) + kRingBytes + kSegBytes; }
};

// What a pass of the reduce reads and writes beside its archives.
struct RedArgs {
  uint32_t batchOffset;  // first member of this grid slice
  uint32_t nb;           // members: source k of member b is entry k * nb + b of `in`
  uint32_t K;            // sources of the whole call (every pass validates all of them)
  uint32_t k0;           // this pass's first source
  int pb;
  uint32_t chunksPerWG;
  uint32_t initKind;     // 0: none (the sum starts as float(x_k0)), 1: the archives' 16-bit type, 2: fp32
  uint32_t outF32;       // out words are fp32 (always for fp32 archives), else the archives' 16-bit type
  uint32_t writeStatus;  // the last pass writes outSuccess / outSize
};

// Entry e of a pointer-mode descriptor, e per lane (BatchDesc::start reads a
// wave-uniform entry).
__device__ __forceinline__ gp<const uint8_t> laneStart(const BatchDesc& d, uint32_t e) {
#if defined(__HIP_DEVICE_COMPILE__)
  uintptr_t t = reinterpret_cast<uintptr_t>(d.ptrs);
  if (d.inl & BatchDesc::kInlPtrs)
    t += reinterpret_cast<uintptr_t>((const DG_CONST uint8_t*)__builtin_amdgcn_kernarg_segment_ptr());
  return (gp<const uint8_t>)(((gp<const uint64_t>)t)[e]);
#else
  (void)d;
  (void)e;
  return nullptr;
#endif
}

// openArchive's checks on one lane's archive (single-stream float types).  The
// ANS header lies past the raw section, whose size follows from n and the
// type: it is read only once the float header has passed.
template <int FT>
__device__ __forceinline__ bool archiveValid(gp<const uint8_t> base, int pb, uint32_t& n) {
  static_assert(FT >= 1 && FT <= 3, "fp16, bf16 and fp32");
  gp<const uint32_t> fh = (gp<const uint32_t>)base;
  n = fh[kFloatSize];
  if (fh[kFloatMagic] != kFloatMagicVersion || (fh[kFloatType] & kTypeMask) != uint32_t(FT)) return false;
  gp<const uint32_t> ah = (gp<const uint32_t>)ansArchiveOf<FT>(base, n);
  return ah[kAnsMagic] == kANSMagicVersion && (ah[kAnsPrecision] & kTypeMask) == uint32_t(pb) && ah[kAnsSize] == n;
}

// grid (ceil(maxBlocks / (kBlocksPerWG * chunksPerWG)), members), dynamic LDS
// RedCfg<NS>::ldsBytes(pb).  in: pointer mode, K * nb entries; init (unless
// initKind 0) and out: one entry per member, out.size(b) the capacity in
// words.  A member succeeds iff all K archives are valid at pb, hold the same
// n and n <= out.size(b); a failing member's init and out are neither read nor
// written, nor is anything outside out[0 .. n).  out[b] may be init[b].
template <int FT, int NS>
__global__ __launch_bounds__(dec::kThreads) void k_reduce(const InlineTable, BatchDesc in, BatchDesc init,
                                                          BatchDesc out, RedArgs a,
                                                          uint8_t* __restrict__ outSuccess,
                                                          uint32_t* __restrict__ outSize) {
  using Cfg = RedCfg<NS>;
  using J = Join<FT>;
  constexpr int R = J::kR;
  static_assert(DecCfg<FT>::S == 1, "one ANS stream per word");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  lp<uint8_t> L = (lp<uint8_t>)smem;
  const int pb = a.pb;
  const uint32_t lutEach = 8u << pb;
  lp<uint16_t> ringAll = (lp<uint16_t>)(L + Cfg::lutBytes(pb));
  lp<uint16_t> segAll = (lp<uint16_t>)(L + Cfg::lutBytes(pb) + Cfg::kRingBytes);

  const uint32_t b = a.batchOffset + blockIdx.y;
  const uint32_t tid = threadIdx.x;
  const uint32_t chunksPerWG = a.chunksPerWG;

  // every archive of the member, one per thread; n: the first one's
  const uint32_t n = ((gp<const uint32_t>)startOf(in, b))[kFloatSize];
  lp<uint32_t> bad = (lp<uint32_t>)segAll;
  if (tid == 0) *bad = 0;
  __syncthreads();
  if (tid < a.K) {
    uint32_t nMine;
    const bool okMine = archiveValid<FT>(laneStart(in, tid * a.nb + b), pb, nMine);
    if (!okMine || nMine != n) *bad = 1;
  }
  __syncthreads();
  const bool ok = *bad == 0;
  __syncthreads();
  const bool success = ok && out.size(b) >= n;
  if (a.writeStatus && blockIdx.x == 0 && tid == 0) {
    if (outSuccess) outSuccess[b] = success ? 1 : 0;
    if (outSize) outSize[b] = ok ? n : 0u;
  }
  const uint32_t nBlocks = divUp(n, kBlockSize);
  if (!success || blockIdx.x * chunksPerWG * Cfg::kBlocksPerWG >= nBlocks) return;

  const uint32_t w = readfirst(tid >> 6), lane = tid & 63, l = lane & 31;
  const uint32_t hv = upperHalfMask(lane);
  const uint32_t mask = (1u << pb) - 1;

  gp<const uint8_t> arch[NS], raw[NS];
  bool vecSrc[NS];
  lp<const u32x2> lut[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) {
    gp<const uint8_t> base = startOf(in, (a.k0 + c) * a.nb + b);
    arch[c] = ansArchiveOf<FT>(base, n);
    raw[c] = rawSectionOf(base);
    vecSrc[c] = (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    lut[c] = (lp<const u32x2>)(L + c * lutEach);
  }
  const uint32_t initKind = a.initKind;
  const bool outF32 = FT == 3 || a.outF32 != 0;
  gp<const uint8_t> initB = initKind ? (gp<const uint8_t>)startOf(init, b) : nullptr;
  gp<uint8_t> outB = startOf(out, b);
  const bool initVec = (reinterpret_cast<uintptr_t>(initB) & 15) == 0;
  const bool outVec = (reinterpret_cast<uintptr_t>(outB) & 15) == 0;

#pragma unroll
  for (int c = 0; c < NS; ++c) {
    buildLut64((gp<const uint16_t>)(arch[c] + kANSHeaderBytes), (lp<u32x2>)(L + c * lutEach), pb, (uint32_t*)segAll);
    __syncthreads();
  }

  for (uint32_t pass = 0; pass < chunksPerWG; ++pass) {
    const uint32_t blk0 = (blockIdx.x * chunksPerWG + pass) * Cfg::kBlocksPerWG + w * Cfg::kBlocksPerWave;
    if (blk0 >= nBlocks) break;
    // the wave's pair: blocks blk0 (lanes 0-31) and blk0 + 1 (lanes 32-63),
    // the same blocks of every source
    uint32_t uwH[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) uwH[hh] = blockSymbols(blk0 + hh, nBlocks, n);
    const uint32_t T = max(divUp(uwH[0], 32), divUp(uwH[1], 32));
    const uint32_t nFull = min(uwH[0], uwH[1]) / dec::kSegWords;
    const int32_t nSeg = int32_t(divUp(T, dec::kSegSteps));
    const uint32_t off = dec::kChunk * l;
    const uint32_t bkMine = blk0 + (lane >> 5);
    const uint32_t uw = lane >= 32 ? uwH[1] : uwH[0];

    // every source's states and blockWords first, then the ring fills
    uint32_t x0[NS];
    uint2 bwE[NS][2];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      const AnsSections arc(arch[c], nBlocks);
      x0[c] = bkMine < nBlocks ? ((gp<const uint32_t>)(arc.states + uint64_t(kStateBytesPerBlock) * bkMine))[l]
                               : kMinState;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) bwE[c][hh] = blk0 + hh < nBlocks ? ld8(arc.bwords + blk0 + hh) : make_uint2(0, 0);
    }
    DStream st[NS];
    lp<uint16_t> segLane[NS];
    DStream* chains[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      gp<const uint16_t> data = AnsSections(arch[c], nBlocks).words;
      bindStream(st[c], segLane[c], ringAll, segAll, w * NS + c, hv, l);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) openHalf(st[c], hh, data, bwE[c][hh], blk0 + hh < nBlocks, lane, vecSrc[c]);
      st[c].x = x0[c];
      chains[c] = &st[c];
    }

    // raw bytes of every source and the init words of this lane's chunk of
    // segment g, double-buffered a segment ahead of their use.  Init words:
    // dv[k] = word k, or (16-bit init, whole aligned chunk) dv[0 .. 3] packed.
    auto loadAhead = [&](int32_t g, uint32_t (&rv)[NS][R], uint32_t (&dv)[8]) __attribute__((always_inline)) {
      const uint32_t segW0 = uint32_t(g) * dec::kSegWords;
      if (segW0 + off >= uw) return;
      const uint32_t cnt = min(dec::kChunk, uw - segW0 - off);
      const uint32_t i0 = bkMine * kBlockSize + segW0 + off;
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        // (the planes are padded past n: a tail chunk's bytes are all there)
        if (vecSrc[c]) {
          J::load(rv[c], raw[c], n, i0);
        } else if constexpr (FT == 3) {
          gp<const uint32_t> p = (gp<const uint32_t>)(raw[c] + 2 * uint64_t(i0));
          gp<const uint32_t> h = (gp<const uint32_t>)(raw[c] + floatPlane2Offset(FT, n) + i0);
          rv[c][0] = p[0]; rv[c][1] = p[1]; rv[c][2] = p[2]; rv[c][3] = p[3];
          rv[c][4] = h[0]; rv[c][5] = h[1];
        } else {
          gp<const uint32_t> p = (gp<const uint32_t>)(raw[c] + i0);
          rv[c][0] = p[0]; rv[c][1] = p[1];
        }
      }
      if (initKind == 2) {
        gp<const uint32_t> p = (gp<const uint32_t>)initB + uint64_t(i0);
        if (initVec && cnt == dec::kChunk) {
          const u32x4 v0 = ((gp<const u32x4>)p)[0], v1 = ((gp<const u32x4>)p)[1];
          dv[0] = v0.x; dv[1] = v0.y; dv[2] = v0.z; dv[3] = v0.w;
          dv[4] = v1.x; dv[5] = v1.y; dv[6] = v1.z; dv[7] = v1.w;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < dec::kChunk; ++k)
            if (k < cnt) dv[k] = p[k];
        }
      } else if (initKind == 1) {
        gp<const uint16_t> p = (gp<const uint16_t>)initB + uint64_t(i0);
        if (initVec && cnt == dec::kChunk) {
          const u32x4 v0 = *(gp<const u32x4>)p;
          dv[0] = v0.x; dv[1] = v0.y; dv[2] = v0.z; dv[3] = v0.w;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < dec::kChunk; ++k)
            if (k < cnt) dv[k] = p[k];
        }
      }
    };

    auto join = [&](int32_t g, const uint32_t (&rv)[NS][R], const uint32_t (&dv)[8]) __attribute__((always_inline)) {
      const uint32_t segW0 = uint32_t(g) * dec::kSegWords;
      if (segW0 + off >= uw) return;
      const uint32_t cnt = min(dec::kChunk, uw - segW0 - off);
      const uint32_t i0 = bkMine * kBlockSize + segW0 + off;
      const bool whole = cnt == dec::kChunk;
      float acc[dec::kChunk];
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        uint32_t sv[4], sv1[4], o[J::kW];
        lp<const uint16_t> q = segLane[c] - l + off;
        loadChunkSyms<1>(q, q, sv, sv1);
        J::words(o, sv, sv1, rv[c]);
        float x[dec::kChunk];
#pragma unroll
        for (int k = 0; k < int(dec::kChunk); ++k) {
          if constexpr (FT == 3) x[k] = __builtin_bit_cast(float, o[k]);
          else x[k] = J::widen(o[k >> 1] >> (16 * (k & 1)));
        }
        if (c == 0) {
          if (initKind == 0) {
#pragma unroll
            for (int k = 0; k < int(dec::kChunk); ++k) acc[k] = x[k];
          } else {
            float i[dec::kChunk];
            if (initKind == 2) {
#pragma unroll
              for (int k = 0; k < int(dec::kChunk); ++k) i[k] = __builtin_bit_cast(float, dv[k]);
            } else if constexpr (FT != 3) {
              if (initVec && whole) {
#pragma unroll
                for (int k = 0; k < int(dec::kChunk); ++k) i[k] = J::widen(dv[k >> 1] >> (16 * (k & 1)));
              } else {
#pragma unroll
                for (int k = 0; k < int(dec::kChunk); ++k) i[k] = J::widen(dv[k]);
              }
            }
#pragma unroll
            for (int k = 0; k < int(dec::kChunk); ++k) acc[k] = i[k] + x[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < int(dec::kChunk); ++k) acc[k] = acc[k] + x[k];
        }
      }
      if (outF32) {
        gp<uint32_t> p = (gp<uint32_t>)outB + uint64_t(i0);
        uint32_t t[dec::kChunk];
#pragma unroll
        for (int k = 0; k < int(dec::kChunk); ++k) t[k] = __builtin_bit_cast(uint32_t, acc[k]);
        if (outVec && whole) {
          ((gp<u32x4>)p)[0] = u32x4{t[0], t[1], t[2], t[3]};
          ((gp<u32x4>)p)[1] = u32x4{t[4], t[5], t[6], t[7]};
        } else {
#pragma unroll
          for (uint32_t k = 0; k < dec::kChunk; ++k)
            if (k < cnt) p[k] = t[k];
        }
      } else if constexpr (FT != 3) {
        // one rounding to nearest even
        gp<uint16_t> p = (gp<uint16_t>)outB + uint64_t(i0);
        uint32_t h[dec::kChunk];
#pragma unroll
        for (int k = 0; k < int(dec::kChunk); ++k) {
          if constexpr (FT == 1) h[k] = __builtin_bit_cast(uint16_t, _Float16(acc[k]));
          else h[k] = J::bf16Of(acc[k]);
        }
        if (outVec && whole) {
          *(gp<u32x4>)p = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        } else {
#pragma unroll
          for (uint32_t k = 0; k < dec::kChunk; ++k)
            if (k < cnt) p[k] = uint16_t(h[k]);
        }
      }
    };

    // a segment: the next one's loads, its 8 steps of every chain (masked in
    // the partial top segments of a tail pair), its join
    auto seg = [&](int32_t g, const uint32_t (&cur)[NS][R], uint32_t (&nxt)[NS][R], const uint32_t (&dcur)[8],
                   uint32_t (&dnxt)[8]) __attribute__((always_inline)) {
      if (g > 0) loadAhead(g - 1, nxt, dnxt);
      if (uint32_t(g) < nFull) {
#pragma unroll
        for (int grp = int(dec::kSegSteps / dec::kUnroll) - 1; grp >= 0; --grp) {
#pragma unroll
          for (int c = 0; c < NS; ++c) ringEnsure(st[c], lane, vecSrc[c]);
          decSteps<false, NS>(chains, lut, mask, pb, hv, segLane, grp * int(dec::kUnroll), 0, l, 0u);
        }
      } else {
        const int32_t tBot = g * int32_t(dec::kSegSteps);
#pragma unroll
        for (int grp = int(dec::kSegSteps / dec::kUnroll) - 1; grp >= 0; --grp) {
#pragma unroll
          for (int c = 0; c < NS; ++c) ringEnsure(st[c], lane, vecSrc[c]);
          decSteps<true, NS>(chains, lut, mask, pb, hv, segLane, grp * int(dec::kUnroll), tBot, l, uw);
        }
      }
      __builtin_amdgcn_wave_barrier();
      join(g, cur, dcur);
      __builtin_amdgcn_wave_barrier();
    };
    uint32_t rvA[NS][R], rvB[NS][R], dvA[8], dvB[8];
    int32_t g = nSeg - 1;
    if (g >= 0) loadAhead(g, rvA, dvA);
    for (; g >= 1; g -= 2) {
      seg(g, rvA, rvB, dvA, dvB);
      seg(g - 1, rvB, rvA, dvB, dvA);
    }
    if (g == 0) seg(0, rvA, rvB, dvA, dvB);
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace dietgpu
