// Pooled row gather kernel for gfx950: bags of rows of a
// [R, rowWords] table stored as one dense float archive, each bag summed into
// one output row -- embedding_bag(mode="sum") on a compressed table.
//
//   out[b * outRowStride + j] = round_out((..(f(x_1[j]) + f(x_2[j])) + ..) + f(x_m[j]))
//
// x_t the row named by idx[offsets[b] + t - 1], f the exact conversion to fp32,
// every add one fp32 add in list order, the sum started as f(x_1) (k_reduce's
// rule, reduce.h), one rounding to the output type.
//
// A third outer loop around k_decode's block body (decode.h), after k_decode's
// own and k_gather's (gather.h): openArchive, buildLut64, bindStream /
// openHalf, ringEnsure, decSteps and the scalar join (Join::one) are theirs.
// What this file holds is what differs from k_gather:
//  * a task is (bag, column tile of kGatherSumTile words), not (index, block):
//    the half-wave that owns it walks the bag's indices in order and decodes,
//    per row, the block(s) that hold the tile's words, from the block's top
//    down to the lowest segment the tile needs;
//  * the running sum lives in registers.  Rows of one bag start anywhere in
//    their blocks, so word j of two rows is decoded by different lanes; but
//    the segment buffer in LDS holds a segment's 256 symbols in word order,
//    so after a segment's steps the lane that *owns* column j (j % 32 == its
//    lane in the half) reads the symbol of whichever word holds column j,
//    joins it with its raw byte(s) and adds it to its register for j.  One
//    owner per column: no atomics, no LDS accumulator, program order is list
//    order.  kGatherSumTile / 32 = 4 fp32 registers per lane;
//  * the two halves of a wave advance independently: a half that finishes its
//    bag stores its tile (coalesced, once) and takes its next task while the
//    other half is still in the middle of a longer bag;
//  * a status per bag.  The tile is stored after the bag's last add, so a bad
//    index leaves the row untouched without a second pass.
#pragma once

#include "decode.h"
#include "decode_plan.h"

namespace dietgpu {

// grid planGatherSum().gridX (decode_plan.h), dynamic LDS DecCfg<FT>::ldsBytes(pb).
// Bag b = idx[offsets[b] .. offsets[b + 1]); `tiles` = planGatherSum().tiles.
// Bag b succeeds iff the headers pass k_decode's checks, 0 <= offsets[b] <=
// offsets[b + 1] <= numIdx and every index of the bag lies in [0, n / rowWords)
// (n: the element's size, from its header); an empty bag gives +0.0.  Only the
// rowWords words of succeeding bags are written; outSuccess[b] (optional) is
// written once, by the half-wave that takes the bag's first tile.
// OUT32: out words are fp32 (always for fp32 archives), else the archive's
// 16-bit type.  numBags * tiles < 2^32.
// Residency: 60 VGPRs (64 allocated: 8 waves per SIMD) and, as k_decode and
// k_gather, at most 80 SGPRs (decode.h: above 80 a CU admits 7 of these
// workgroups), so 8 workgroups per CU; the per-half task state beyond 80 SGPRs
// lives in VGPR lanes, no scratch.  A 256-column tile (8 accumulator registers,
// 8 columns' loads in flight) took 78 VGPRs: 6 per CU.
template <int FT, bool OUT32>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(4))) void k_gatherSum(
    const uint8_t* __restrict__ archive, const void* __restrict__ idx, const void* __restrict__ offsets,
    uint32_t idxIs64, uint32_t numBags, uint32_t numIdx, uint32_t rowWords, uint32_t tiles, uint8_t* out,
    uint64_t outRowStride, int pb, uint8_t* outSuccess) {
  static_assert(FT >= 1 && FT <= 3 && (OUT32 || FT != 3), "fp16, bf16 and fp32; fp32 sums leave as fp32");
  using Cfg = DecCfg<FT>;
  using J = Join<FT, 0>;
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  constexpr int S = Cfg::S;
  static_assert(S == 1, "one ANS stream per word");
  constexpr int kCols = int(kGatherSumTile / 32);  // columns (registers) per lane
  static_assert(kGatherSumTile % 32 == 0 && kGatherSumTile <= kBlockSize, "a tile spans at most two blocks");
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
  // this lane's columns l, l + 32, ... of its half's tile
  float acc[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) acc[c] = 0.f;

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
    if (posH[hh] < endH[hh]) pfH[hh] = entry(idx, posH[hh]);
    // an empty bag stores +0.0
    if (hi == (hh == 1)) {
#pragma unroll
      for (int c = 0; c < kCols; ++c) acc[c] = 0.f;
    }
  };

  // the end of half hh's task: the tile, stored once, and the bag's status
  auto finishTask = [&](int hh) __attribute__((always_inline)) {
    if (hi == (hh == 1)) {
      if (!failedH[hh]) {
        gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(bagH[hh]) * outRowStride + c0H[hh]);
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          const uint32_t col = uint32_t(c) * 32 + l;
          if (col < twH[hh]) {
            if constexpr (OUT32) o[col] = __builtin_bit_cast(uint32_t, acc[c]);
            else if constexpr (FT == 1) o[col] = __builtin_bit_cast(uint16_t, _Float16(acc[c]));
            else o[col] = uint16_t(J::bf16Of(acc[c]));
          }
        }
      }
      if (c0H[hh] == 0 && outSuccess && l == 0) G(outSuccess)[uint64_t(bagH[hh])] = failedH[hh] ? 0 : 1;
    }
  };

  // The next block half hh decodes: bk (uwH 0: the half has run out of tasks).
  // Takes rows, finishes tasks and starts new ones on the way.
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
        // the next row of the bag; its successor's index is loaded a row ahead
        const int64_t v = uniform(pfH[hh]);
        ++posH[hh];
        if (posH[hh] < endH[hh]) pfH[hh] = entry(idx, posH[hh]);
        firstH[hh] = !seenH[hh];
        seenH[hh] = true;
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
    pfH[hh] = 0;
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
        float f[kCols];
        bool on[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          on[c] = false;
          f[c] = 0.f;
          if (uint32_t(c) * 32 < twW) {
            const uint32_t col = uint32_t(c) * 32 + l;
            const uint32_t i = rloM + col;
            on[c] = uwM != 0 && col < twM && i >= segBase && i - segBase < dec::kSegWords;
            const uint32_t sym = segHalf[(i - segBase) & (dec::kSegWords - 1)];
            const auto x = J::one(sym >> 8, 0, raw, n, on[c] ? i : 0u);
            if constexpr (FT == 3) f[c] = __builtin_bit_cast(float, x);
            else f[c] = J::widen(x);
          }
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          if (uint32_t(c) * 32 < twW) acc[c] = on[c] ? (firstM ? f[c] : acc[c] + f[c]) : acc[c];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace dietgpu
