// Pooled row gather with a pooling mode, per-sample weights and a padding
// index, for gfx950: torch's embedding_bag on a [R, rowWords]
// table stored as one dense float archive.  With x_t the bag's rows that are
// not the padding index, in list order, f the exact conversion to fp32 and n_b
// their count:
//
//   sum          out = round_out((..(f(x_1) + f(x_2)) + ..) + f(x_n))
//   sum, weights acc = w_1 * f(x_1); acc = fmaf(w_t, f(x_t), acc); out = round_out(acc)
//   mean         out = round_out(sum / float(n_b))      (one fp32 division)
//   max          m = f(x_1); m = (f(x_t) > m || isnan(f(x_t))) ? f(x_t) : m
//
// per column; an empty or all-padding bag gives +0.0 in every mode.
//
// A sixth outer loop around k_decode's block body (decode.h), and k_gatherSum's
// shape (gather_sum.h): a task is (bag, column tile of kGatherSumTile words)
// per half-wave, the lane that owns column j reads whichever segment word
// holds it, the two halves advance independently and the tile is stored once,
// after the bag's last row.  openArchive, buildLut64, bindStream / openHalf,
// ringEnsure, decSteps and Join::one are the decoder's.  What this file adds:
//  * the weight of idx[pos] is loaded with the index, a row ahead, made
//    wave-uniform when its row is taken and kept with the per-half task state;
//    the segment loop gains no load, its add becomes a select between a
//    multiply (the bag's first row) and an fmaf;
//  * an entry equal to the padding index is consumed in advance(): it never
//    reaches the range check or the block loop, is not counted, and leaves
//    firstH / seenH alone, so the row after a leading padding entry is still
//    the bag's first;
//  * mean counts the rows a half takes and divides in finishTask, in the lanes
//    that store;
//  * max keeps the table's *word* of the running maximum, not its value: the
//    compare widens both sides, the select moves bits, so a 16-bit out carries
//    table words bit for bit (denormals, NaN payloads) and nothing is rounded.
// MODE and WT are template parameters: the unweighted sum has k_gatherSum's
// loop, and only the combinations an entry point can reach are instantiated
// (gather_pool.hip).
#pragma once

#include "decode.h"
#include "decode_plan.h"

namespace dietgpu {

constexpr int kPoolSum = 0, kPoolMean = 1, kPoolMax = 2;
// the weights of a pooled gather: none, fp32, or the archive's 16-bit type
constexpr int kPoolWNone = 0, kPoolW32 = 1, kPoolW16 = 2;

// grid planGatherSum().gridX (decode_plan.h), dynamic LDS DecCfg<FT>::ldsBytes(pb);
// every argument of k_gatherSum as there.  weights (WT != 0): numIdx words,
// weights[i] the weight of idx[i].  padIdx: the padding index, negative for
// none.  Bag b succeeds iff the headers pass k_decode's checks, its offsets are
// ordered and inside [0, numIdx] and every index of the bag that is not padIdx
// lies in [0, n / rowWords); only the rowWords words of succeeding bags are
// written.
template <int FT, bool OUT32, int MODE, int WT>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(4))) void k_gatherPool(
    const uint8_t* __restrict__ archive, const void* __restrict__ idx, const void* __restrict__ offsets,
    const void* __restrict__ weights, int64_t padIdx, uint32_t idxIs64, uint32_t numBags, uint32_t numIdx,
    uint32_t rowWords, uint32_t tiles, uint8_t* out, uint64_t outRowStride, int pb, uint8_t* outSuccess) {
  static_assert(FT >= 1 && FT <= 3 && (OUT32 || FT != 3), "fp16, bf16 and fp32; fp32 tables leave as fp32");
  static_assert(MODE >= kPoolSum && MODE <= kPoolMax && WT >= kPoolWNone && WT <= kPoolW16, "mode and weight type");
  static_assert(WT == kPoolWNone || MODE == kPoolSum, "weights go with the sum alone");
  static_assert(WT != kPoolW16 || FT != 3, "16-bit weights are the 16-bit archive's type");
  using Cfg = DecCfg<FT>;
  using J = Join<FT, 0>;
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  constexpr int S = Cfg::S;
  static_assert(S == 1, "one ANS stream per word");
  constexpr int kCols = int(kGatherSumTile / 32);  // columns (registers) per lane
  static_assert(kGatherSumTile % 32 == 0 && kGatherSumTile <= kBlockSize, "a tile spans at most two blocks");
  constexpr bool kW = WT != kPoolWNone;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  lp<uint8_t> L = (lp<uint8_t>)smem;
  const uint32_t lutBytes = Cfg::lutBytes(pb);
  lp<uint16_t> ringAll = (lp<uint16_t>)(L + lutBytes);
  lp<uint16_t> segAll = (lp<uint16_t>)(L + lutBytes + Cfg::kRingBytes);

  const uint32_t tid = threadIdx.x;
  gp<const uint8_t> base = G(archive);

  // the headers, once per workgroup (k_decode's checks)
  gp<const uint8_t> arch[S];
  bool ok;
  const uint32_t n = openArchive<FT>(base, pb, ok, arch);
  // whole rows of the element; 0: every index fails
  const uint32_t nRows = ok ? n / rowWords : 0u;
  const uint32_t nBlocks = divUp(n, kBlockSize);
  const uint64_t total = uint64_t(numBags) * tiles;
  const uint32_t groups = uint32_t((total + kGatherTasksPerWG - 1) / kGatherTasksPerWG);

  const uint32_t w = readfirst(tid >> 6), lane = tid & 63, l = lane & 31;
  const uint32_t hv = upperHalfMask(lane);
  const bool hi = lane >= 32;
  const bool vecIn = (reinterpret_cast<uintptr_t>(archive) & 15) == 0;
  gp<const uint8_t> raw = rawSectionOf(base);
  const uint32_t mask = (1u << pb) - 1;
  lp<const u32x2> lut[S];
  lut[0] = (lp<const u32x2>)L;

  if (nRows > 0) {
    buildLut64((gp<const uint16_t>)(arch[0] + kANSHeaderBytes), (lp<u32x2>)L, pb, (uint32_t*)segAll);
    __syncthreads();
  }

  // entry i of idx / offsets, wave-uniform
  auto uniform = [](int64_t x) __attribute__((always_inline)) {
    return int64_t(uint64_t(readfirst(uint32_t(x))) | (uint64_t(readfirst(uint32_t(uint64_t(x) >> 32))) << 32));
  };
  auto entry = [&](const void* p, uint64_t i) __attribute__((always_inline)) {
    return idxIs64 ? ((gp<const int64_t>)G(p))[i] : int64_t(((gp<const int32_t>)G(p))[i]);
  };
  // the word of a table value as fp32, exactly
  auto wide = [](uint32_t x) __attribute__((always_inline)) {
    if constexpr (FT == 3) return __builtin_bit_cast(float, x);
    else return J::widen(x);
  };
  // weight i as fp32, exactly (the bits of the load; 0 without weights)
  auto weightBits = [&](uint64_t i) __attribute__((always_inline)) {
    if constexpr (WT == kPoolW32) return ((gp<const uint32_t>)G(weights))[i];
    else if constexpr (WT == kPoolW16) return __builtin_bit_cast(uint32_t, J::widen(((gp<const uint16_t>)G(weights))[i]));
    else return 0u;
  };

  // Per half (wave-uniform): the task it is in and where in it.
  uint32_t grpH[2];             // the task group the half's task comes from
  bool liveH[2];                // in a task
  uint32_t bagH[2], c0H[2], twH[2];  // its bag, the tile's first column and width
  uint32_t posH[2], endH[2];    // the bag's indices still to come: idx[pos .. end)
  bool failedH[2];              // bad offsets, a failing archive, or a bad index so far
  bool firstH[2], seenH[2];     // the row in progress is the bag's first / a row was taken
  uint32_t rloH[2];             // first element word of the tile in the row in progress
  uint32_t bkNextH[2], bkEndH[2];  // that row's blocks still to decode: [bkNext, bkEnd)
  int64_t pfH[2];               // idx[pos], loaded when the row before it was taken (per lane)
  uint32_t pfwH[2];             // ... and its weight's fp32 bits (WT != 0)
  uint32_t wH[2];               // the fp32 bits of the weight of the row in progress (WT != 0)
  uint32_t cntH[2];             // rows taken (mean)
  // this lane's columns l, l + 32, ... of its half's tile: the fp32 bits of
  // the running sum, or (max) the table word of the running maximum
  uint32_t acc[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) acc[c] = 0u;

  // the task of half hh in group grpH[hh]: offsets, validity, first index
  auto startTask = [&](int hh) __attribute__((always_inline)) {
    const uint64_t t = uint64_t(grpH[hh]) * kGatherTasksPerWG + 2 * w + uint32_t(hh);
    liveH[hh] = grpH[hh] < groups && t < total;
    bkNextH[hh] = 0, bkEndH[hh] = 0;
    if (!liveH[hh]) return;
    const uint32_t bag = tiles == 1 ? uint32_t(t) : uint32_t(t / tiles);
    const uint32_t tile = uint32_t(t - uint64_t(bag) * tiles);
    bagH[hh] = bag;
    c0H[hh] = tile * kGatherSumTile;
    twH[hh] = min(kGatherSumTile, rowWords - c0H[hh]);
    const int64_t lo = uniform(entry(offsets, bag)), up = uniform(entry(offsets, uint64_t(bag) + 1));
    const bool good = ok && lo >= 0 && lo <= up && up <= int64_t(numIdx);
    failedH[hh] = !good;
    posH[hh] = good ? uint32_t(lo) : 0u;
    endH[hh] = good ? uint32_t(up) : 0u;
    firstH[hh] = true, seenH[hh] = false;
    cntH[hh] = 0;
    if (posH[hh] < endH[hh]) {
      pfH[hh] = entry(idx, posH[hh]);
      if constexpr (kW) pfwH[hh] = weightBits(posH[hh]);
    }
    // an empty bag stores +0.0
    if (hi == (hh == 1)) {
#pragma unroll
      for (int c = 0; c < kCols; ++c) acc[c] = 0u;
    }
  };

  // the end of half hh's task: the tile, stored once, and the bag's status
  auto finishTask = [&](int hh) __attribute__((always_inline)) {
    if (hi == (hh == 1)) {
      if (!failedH[hh]) {
        gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(bagH[hh]) * outRowStride + c0H[hh]);
        // (mean) float(n_b); a bag without rows keeps its +0.0
        const float cnt = float(max(cntH[hh], 1u));
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          const uint32_t col = uint32_t(c) * 32 + l;
          if (col < twH[hh]) {
            if constexpr (MODE == kPoolMax) {
              // the table's word, widened exactly for an fp32 out
              if constexpr (!OUT32) o[col] = uint16_t(acc[c]);
              else o[col] = __builtin_bit_cast(uint32_t, wide(acc[c]));
            } else {
              float v = __builtin_bit_cast(float, acc[c]);
              if constexpr (MODE == kPoolMean) v = v / cnt;
              if constexpr (OUT32) o[col] = __builtin_bit_cast(uint32_t, v);
              else if constexpr (FT == 1) o[col] = __builtin_bit_cast(uint16_t, _Float16(v));
              else o[col] = uint16_t(J::bf16Of(v));
            }
          }
        }
      }
      if (c0H[hh] == 0 && outSuccess && l == 0) G(outSuccess)[uint64_t(bagH[hh])] = failedH[hh] ? 0 : 1;
    }
  };

  // The next block half hh decodes: bk (uwH 0: the half has run out of tasks).
  // Takes rows, skips padding entries, finishes tasks and starts new ones on
  // the way.
  uint32_t bkH[2], uwH[2];
  auto advance = [&](int hh) __attribute__((always_inline)) {
    bkH[hh] = 0, uwH[hh] = 0;
    while (liveH[hh]) {
      if (bkNextH[hh] < bkEndH[hh]) {
        bkH[hh] = bkNextH[hh]++;
        uwH[hh] = symbolsOfBlock(bkH[hh], n);
        return;
      }
      if (!failedH[hh] && posH[hh] < endH[hh]) {
        // the next entry of the bag; its successor's index and weight are
        // loaded a row ahead
        const int64_t v = uniform(pfH[hh]);
        uint32_t wv = 0;
        if constexpr (kW) wv = readfirst(pfwH[hh]);
        ++posH[hh];
        if (posH[hh] < endH[hh]) {
          pfH[hh] = entry(idx, posH[hh]);
          if constexpr (kW) pfwH[hh] = weightBits(posH[hh]);
        }
        // a padding entry: consumed here, before the range check
        if (padIdx >= 0 && v == padIdx) continue;
        firstH[hh] = !seenH[hh];
        seenH[hh] = true;
        if constexpr (kW) wH[hh] = wv;
        if constexpr (MODE == kPoolMean) ++cntH[hh];
        if (v < 0 || uint64_t(v) >= nRows) {
          failedH[hh] = true;
        } else {
          rloH[hh] = uint32_t(v) * rowWords + c0H[hh];  // (v + 1) * rowWords <= n: no wrap
          bkNextH[hh] = rloH[hh] / kBlockSize;
          bkEndH[hh] = (rloH[hh] + twH[hh] - 1) / kBlockSize + 1;
        }
        continue;
      }
      finishTask(hh);
      grpH[hh] += gridDim.x;
      startTask(hh);
    }
  };

#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    grpH[hh] = blockIdx.x;
    bagH[hh] = 0, c0H[hh] = 0, twH[hh] = 0, posH[hh] = 0, endH[hh] = 0, rloH[hh] = 0;
    failedH[hh] = true, firstH[hh] = true, seenH[hh] = false;
    pfH[hh] = 0, pfwH[hh] = 0, wH[hh] = 0, cntH[hh] = 0;
    startTask(hh);
  }

  // Persistent over the task groups, one generation of resident workgroups.
  // No workgroup barrier below: the waves run their tasks independently.
  for (;;) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) advance(hh);
    if (uwH[0] == 0 && uwH[1] == 0) break;

    // the lowest segment either half needs, and the tiles' word ranges
    uint32_t rhiH[2];
    int32_t gMin = INT32_MAX;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      rhiH[hh] = rloH[hh] + twH[hh];
      if (uwH[hh]) {
        const uint32_t b0 = bkH[hh] * kBlockSize;
        gMin = min(gMin, int32_t(rloH[hh] > b0 ? (rloH[hh] - b0) / dec::kSegWords : 0u));
      }
    }

    // this lane's half
    const uint32_t bkM = hi ? bkH[1] : bkH[0], uwM = hi ? uwH[1] : uwH[0];
    const uint32_t rloM = hi ? rloH[1] : rloH[0], twM = hi ? twH[1] : twH[0];
    const bool firstM = hi ? firstH[1] : firstH[0];
    const float wM = __builtin_bit_cast(float, hi ? wH[1] : wH[0]);
    const uint32_t twW = max(uwH[0] ? twH[0] : 0u, uwH[1] ? twH[1] : 0u);

    // states and block-words entries
    const AnsSections arc(arch[0], nBlocks);
    const uint32_t x0 = uwM ? ((gp<const uint32_t>)(arc.states + uint64_t(kStateBytesPerBlock) * bkM))[l] : kMinState;
    uint2 bwE[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) bwE[hh] = uwH[hh] ? ld8(arc.bwords + bkH[hh]) : make_uint2(0, 0);

    const uint32_t T = max(divUp(uwH[0], 32), divUp(uwH[1], 32));
    // segments [0, nFull) are full for both halves' blocks: unmasked steps
    const uint32_t nFull = min(uwH[0], uwH[1]) / dec::kSegWords;
    const int32_t nSeg = int32_t(divUp(T, dec::kSegSteps));

    DStream st[S];
    lp<uint16_t> segLane[S];
    DStream* chains[S];
    bindStream(st[0], segLane[0], ringAll, segAll, w, hv, l);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) openHalf(st[0], hh, arc.words, bwE[hh], uwH[hh] != 0, lane, vecIn);
    st[0].x = x0;
    chains[0] = &st[0];
    // this half's segment buffer: symbol (<< 8) of segment word q at segHalf[q]
    lp<const uint16_t> segHalf = segLane[0] - l;

    // A block is decoded from its top down to the lowest segment either half
    // needs: the state chain runs through the segments above a tile.
    for (int32_t g = nSeg - 1; g >= gMin; --g) {
      const bool full = uint32_t(g) < nFull;
      const int32_t tBot = g * int32_t(dec::kSegSteps);
#pragma unroll
      for (int sg = int(dec::kSegSteps / dec::kUnroll) - 1; sg >= 0; --sg) {
        ringEnsure(st[0], lane, vecIn);
        // a partial segment, or a half that idles: masked steps
        if (full) decSteps<false, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), 0, l, 0u);
        else decSteps<true, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), tBot, l, uwM);
      }
      __builtin_amdgcn_wave_barrier();
      // does the segment hold words of either half's tile?
      bool hit = false;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const uint32_t sb = bkH[hh] * kBlockSize + uint32_t(g) * dec::kSegWords;
        hit = hit || (uwH[hh] != 0 && sb < rhiH[hh] && sb + dec::kSegWords > rloH[hh]);
      }
      if (hit) {
        const uint32_t segBase = bkM * kBlockSize + uint32_t(g) * dec::kSegWords;
        // Column c * 32 + l of the tile is element word rloM + c * 32 + l: in
        // this segment or not.  A lane whose word is not reads the segment
        // buffer's slot and element word 0 all the same and drops them, so
        // that the loads of all columns are in flight together.
        uint32_t x[kCols];
        bool on[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          on[c] = false;
          x[c] = 0u;
          if (uint32_t(c) * 32 < twW) {
            const uint32_t col = uint32_t(c) * 32 + l;
            const uint32_t i = rloM + col;
            on[c] = uwM != 0 && col < twM && i >= segBase && i - segBase < dec::kSegWords;
            const uint32_t sym = segHalf[(i - segBase) & (dec::kSegWords - 1)];
            x[c] = uint32_t(J::one(sym >> 8, 0, raw, n, on[c] ? i : 0u));
          }
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          if (uint32_t(c) * 32 < twW) {
            const float f = wide(x[c]);
            if constexpr (MODE == kPoolMax) {
              // the first row, a greater value or a NaN: its word replaces the
              // maximum's.  Not fmaxf: that drops a NaN and leaves ties open.
              const bool take = firstM || f > wide(acc[c]) || f != f;
              acc[c] = (on[c] && take) ? x[c] : acc[c];
            } else {
              const float a = __builtin_bit_cast(float, acc[c]);
              float s;
              if constexpr (kW) s = firstM ? wM * f : __builtin_fmaf(wM, f, a);
              else s = firstM ? f : a + f;
              acc[c] = on[c] ? __builtin_bit_cast(uint32_t, s) : acc[c];
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace dietgpu
