// Row gather kernel for gfx950: rows of a [R, rowWords]
// table stored as one archive, each named by an index in device memory.
//
// A new outer loop around k_decode's block body (decode.h): openArchive,
// buildLut64, bindStream / openHalf, ringEnsure, decSteps, the chunk join (loadChunkSyms,
// Join<FT>::vec, joinWords) and the range form's edge rule (clipChunk) are
// k_decode's own.  What this file holds is what differs:
//  * one persistent grid: a workgroup validates the headers and builds the
//    decode table once, then strides over groups of 8 tasks;
//  * a task (the j-th block of the row that index i names) belongs to a
//    half-wave: lanes 0-31 and lanes 32-63 decode blocks of different rows,
//    anywhere in the element.  Block index, word range, block size and
//    destination are wave-uniform per half, as uwH[2] and DStream::ptr[2] are
//    in k_decode; lanes select theirs by their half;
//  * the indices of the next pass are read a pass ahead; nothing comes from
//    the host but the kernel arguments;
//  * a status per row, not per element.
#pragma once

#include "decode.h"

namespace dietgpu {

// grid planGather().gridX (decode_plan.h), dynamic LDS DecCfg<FT>::ldsBytes(pb).
// out[i * outRowStride + j] = word idx[i] * rowWords + j of the element, for
// 0 <= j < rowWords (bytes for FT 0); nothing else is written.  Row i succeeds
// iff the headers pass k_decode's checks and 0 <= idx[i] < n / rowWords (n: the
// element's size, from its header); outSuccess[i] (optional) is written once,
// by the half-wave that takes the row's first task.  numIdx * K < 2^32.
template <int FT>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(4))) void k_gather(
    const uint8_t* __restrict__ archive, const void* __restrict__ idx, uint32_t idxIs64, uint32_t numIdx,
    uint32_t rowWords, uint32_t K, uint8_t* out, uint64_t outRowStride, int pb, uint8_t* outSuccess) {
  using Cfg = DecCfg<FT>;
  using WordT = typename FloatTraits<FT>::WordT;
  using J = Join<FT, 0>;
  constexpr int S = Cfg::S, R = J::kR;
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
  // whole rows of the element; 0: every index fails (the loop below then only
  // writes the statuses)
  const uint32_t nRows = ok ? n / rowWords : 0u;
  const uint32_t nBlocks = divUp(n, kBlockSize);
  const uint32_t total = numIdx * K;
  const uint32_t groups = total / kGatherTasksPerWG + (total % kGatherTasksPerWG != 0);

  const uint32_t w = readfirst(tid >> 6), lane = tid & 63, l = lane & 31;
  const uint32_t hv = upperHalfMask(lane);
  const bool vecIn = (reinterpret_cast<uintptr_t>(archive) & 15) == 0;
  gp<const uint8_t> raw = rawSectionOf(base);
  const uint32_t mask = (1u << pb) - 1;
  lp<const u32x2> lut[S];
#pragma unroll
  for (int s = 0; s < S; ++s) lut[s] = (lp<const u32x2>)(L + s * (lutBytes / S));

  // the indices of the wave's two tasks in group g (wave-uniform; a task past
  // the last one reads nothing and gets -1, which fails like any negative index)
  auto fetch = [&](uint32_t g, int64_t (&v)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t t = g * kGatherTasksPerWG + 2 * w + hh;
      const uint64_t i = K == 1 ? t : t / K;
      int64_t x = -1;
      if (t < total) x = idxIs64 ? ((gp<const int64_t>)G(idx))[i] : int64_t(((gp<const int32_t>)G(idx))[i]);
      v[hh] = int64_t(uint64_t(readfirst(uint32_t(x))) | (uint64_t(readfirst(uint32_t(uint64_t(x) >> 32))) << 32));
    }
  };

  int64_t vNext[2];
  if (blockIdx.x < groups) fetch(blockIdx.x, vNext);
  if (nRows > 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      buildLut64((gp<const uint16_t>)(arch[s] + kANSHeaderBytes), (lp<u32x2>)(L + s * (lutBytes / S)), pb,
                 (uint32_t*)segAll);
      __syncthreads();
    }
  }

  // Persistent over the task groups, one generation of resident workgroups.
  // No workgroup barrier below: the waves run their tasks independently.
  for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t vCur[2] = {vNext[0], vNext[1]};
    if (grp + gridDim.x < groups) fetch(grp + gridDim.x, vNext);

    // per half (wave-uniform): block, its size (0: the half idles), the row's
    // words [rlo, rhi) of the element, and where word 0 of the element would
    // lie so that word i goes to outV[i] (the range form's rule)
    uint32_t bkH[2], uwH[2], rloH[2], rhiH[2];
    uint64_t outV[2];
    int32_t gMin = INT32_MAX;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t t = grp * kGatherTasksPerWG + 2 * w + hh;
      const uint32_t i = K == 1 ? t : t / K;
      const uint32_t j = t - i * K;
      const bool rowOk = vCur[hh] >= 0 && uint64_t(vCur[hh]) < nRows;
      bkH[hh] = 0, uwH[hh] = 0, rloH[hh] = 0, rhiH[hh] = 0, outV[hh] = 0;
      if (t < total) {
        if (j == 0 && outSuccess && lane == uint32_t(hh) * 32) G(outSuccess)[uint64_t(i)] = rowOk ? 1 : 0;
        if (rowOk) {
          const uint32_t s0 = uint32_t(vCur[hh]) * rowWords;  // (idx + 1) * rowWords <= n: no wrap
          const uint32_t bk = s0 / kBlockSize + j;
          if (j < divUp((s0 & (kBlockSize - 1)) + rowWords, kBlockSize)) {
            bkH[hh] = bk;
            uwH[hh] = symbolsOfBlock(bk, n);
            rloH[hh] = s0;
            rhiH[hh] = s0 + rowWords;
            outV[hh] = reinterpret_cast<uintptr_t>(out) + (uint64_t(i) * outRowStride - s0) * sizeof(WordT);
            // the lowest segment this half needs
            gMin = min(gMin, int32_t(s0 > bk * kBlockSize ? (s0 - bk * kBlockSize) / dec::kSegWords : 0u));
          }
        }
      }
    }
    if (uwH[0] == 0 && uwH[1] == 0) continue;

    // this lane's half
    const bool hi = lane >= 32;
    const uint32_t bkM = hi ? bkH[1] : bkH[0], uwM = hi ? uwH[1] : uwH[0];
    const uint32_t rloM = hi ? rloH[1] : rloH[0], rhiM = hi ? rhiH[1] : rhiH[0];
    const uint64_t outM = hi ? outV[1] : outV[0];
    gp<uint8_t> outB = (gp<uint8_t>)outM;
    // the vector join: 16 B-aligned archive and destination (per half)
    const bool vecM = vecIn && (outM & 15) == 0;

    // states and block-words entries
    uint32_t x0[S];
    uint2 bwE[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const AnsSections arc(arch[s], nBlocks);
      x0[s] = uwM ? ((gp<const uint32_t>)(arc.states + uint64_t(kStateBytesPerBlock) * bkM))[l] : kMinState;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) bwE[s][hh] = uwH[hh] ? ld8(arc.bwords + bkH[hh]) : make_uint2(0, 0);
    }

    const uint32_t T = max(divUp(uwH[0], 32), divUp(uwH[1], 32));
    // segments [0, nFull) are full for both halves' blocks: unmasked steps
    const uint32_t nFull = min(uwH[0], uwH[1]) / dec::kSegWords;
    const int32_t nSeg = int32_t(divUp(T, dec::kSegSteps));
    const uint32_t off = dec::kChunk * l;  // this lane's chunk in a segment

    DStream st[S];
    lp<uint16_t> segLane[S];
    DStream* chains[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      gp<const uint16_t> data = AnsSections(arch[s], nBlocks).words;
      bindStream(st[s], segLane[s], ringAll, segAll, w * S + s, hv, l);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) openHalf(st[s], hh, data, bwE[s][hh], uwH[hh] != 0, lane, vecIn);
      st[s].x = x0[s];
      chains[s] = &st[s];
    }

    // whether this lane's chunk of segment g takes the vector join: whole
    // inside its block and its row, 16 B-aligned source and destination
    auto vecChunk = [&](int32_t g) __attribute__((always_inline)) {
      const uint32_t c0 = uint32_t(g) * dec::kSegWords + off;
      const uint32_t i0 = bkM * kBlockSize + c0;
      return vecM && c0 + dec::kChunk <= uwM && i0 >= rloM && i0 + dec::kChunk <= rhiM;
    };

    // A block is decoded from its top down to the lowest segment either half
    // needs: the state chain runs through the segments above a row.
    for (int32_t g = nSeg - 1; g >= gMin; --g) {
      const bool full = uint32_t(g) < nFull;
      const uint32_t c0 = uint32_t(g) * dec::kSegWords + off;
      const uint32_t i0 = bkM * kBlockSize + c0;
      // the chunk's raw float bytes, loaded ahead of the segment's steps
      uint32_t rv[R];
      const bool vc = vecChunk(g);
      if (FT != 0 && vc) J::load(rv, raw, n, i0);
      const int32_t tBot = g * int32_t(dec::kSegSteps);
#pragma unroll
      for (int sg = int(dec::kSegSteps / dec::kUnroll) - 1; sg >= 0; --sg) {
#pragma unroll
        for (int s = 0; s < S; ++s) ringEnsure(st[s], lane, vecIn);
        // a partial segment, or a half that idles: masked steps
        if (full) decSteps<false, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), 0, l, 0u);
        else decSteps<true, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), tBot, l, uwM);
      }
      __builtin_amdgcn_wave_barrier();
      // join: words [k0, k1) of the chunk lie in the block and in the row
      if (c0 < uwM) {
        uint32_t k0, k1;
        if (clipChunk(i0, min(dec::kChunk, uwM - c0), rloM, rhiM, k0, k1)) {
          lp<const uint16_t> q0 = segLane[0] - l + off;
          lp<const uint16_t> q1 = segLane[S - 1] - l + off;
          if (vc) {
            uint32_t sv[4], sv1[4];
            loadChunkSyms<S>(q0, q1, sv, sv1);
            J::template vec<false>(outB, i0, sv, sv1, rv);
          } else {
            joinWords<J>((gp<WordT>)outB, q0, q1, raw, n, i0, k0, k1);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace dietgpu
