// Matmul on a compressed weight table through the matrix pipe, for gfx950
// (DESIGN.md 5.2k): the contract of k_matmulRows (matmul.h) for fp16 and bf16
// archives, 1 <= M <= 64 activation rows in ONE pass over the archive,
//
//   out[m * outRowStride + r] = round_out(sum_k x[m, k] * W[r, k])
//
// the products exact, the sums fp32 (v_mfma_f32_16x16x32_{f16,bf16}), one
// rounding to the output type.
//
// A fifth outer loop around k_decode's block body; openArchive, buildLut64,
// bindStream / openHalf, ringEnsure, decSteps, the 8-word join and
// mm::openTable are the others'.  What differs from k_matmulRows:
//  * the eight half-waves of a workgroup take blocks t0 + P * j, j = 0 .. 7,
//    P = planMatmulTile().period: blocks P apart start at the same column of
//    their rows, so segment g of all eight halves is eight weight rows at one
//    k range, which is the B operand of an MFMA;
//  * after the join each lane writes its 8 words to row j of an LDS tile
//    Wt[8][256] (rows 528 B apart); zeros where the half has no block or the
//    segment lies past the table.  Two tiles and one workgroup barrier per
//    segment: a wave decodes segment g - 1 while a slower one multiplies g;
//  * wave t owns activation rows 16 t .. 16 t + 15 (a wave with no row only
//    decodes).  Its A operands, lane (i, kg) the 16 B at x[16 t + i][col + 32 s
//    + 8 kg], s = 0 .. 7, are loaded from global memory before the segment's
//    decode steps; after the barrier eight MFMAs, s ascending, add the
//    segment into D[16][16], columns 8 .. 15 of B being zero;
//  * a piece ends where its segment starts a row, or at the bottom of the
//    block, which now is the same segment in every half; the lanes that hold
//    column j < 8 store D[m][j] to part[m * pieces + block_j + row_j] and the
//    accumulators restart at 0.  k_matmulFinish (matmul.h) adds a row's pieces.
// A row m of x meets one wave, one accumulator and the segments in one order
// whatever M is, and a weight row's pieces and their segments follow from
// (rowWords, r): the bits are the row's own.
#pragma once

#include "matmul.h"

namespace dietgpu {

namespace mmt {

constexpr uint32_t kTileRowBytes = 2 * dec::kSegWords + 16;  // at 512 the rows of a B read share a bank group
constexpr uint32_t kTileBytes = kGatherTasksPerWG * kTileRowBytes;
constexpr uint32_t kKSteps = dec::kSegWords / 32;  // MFMAs per segment and m-tile

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// D = A * B + C, A [16 x 32] and B [32 x 16] in their lanes' 16 B
template <int FT>
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (FT == 1) {
    const f16x8 av = __builtin_bit_cast(f16x8, a), bv = __builtin_bit_cast(f16x8, b);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, c, 0, 0, 0);
  } else {
    const bf16x8 av = __builtin_bit_cast(bf16x8, a), bv = __builtin_bit_cast(bf16x8, b);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
  }
}

__host__ __device__ constexpr uint32_t ldsBytes(uint32_t decoderBytes) { return decoderBytes + 2 * kTileBytes; }

}  // namespace mmt

// grid planMatmulTile().gridX (decode_plan.h), dynamic LDS
// mmt::ldsBytes(DecCfg<FT>::ldsBytes(pb)).  period: planMatmulTile().period.
// The other arguments, the checks and what a failed check leaves are
// k_matmulRows'; mRows <= 64.
template <int FT>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_matmulTile(
    const uint8_t* __restrict__ archive, uint32_t numRows, uint32_t rowWords, const uint8_t* __restrict__ x,
    uint64_t xRowStrideBytes, uint32_t mRows, float* __restrict__ part, uint32_t pieces, uint32_t period, int pb) {
  static_assert(FT == 1 || FT == 2, "the 16-bit types of v_mfma_f32_16x16x32");
  using Cfg = DecCfg<FT>;
  using J = Join<FT, 0>;
  constexpr int S = Cfg::S, R = J::kR, D = mm::kDwords<FT>;
  static_assert(S == 1 && J::kW == D && D == 4, "one ANS stream per word, 16 B per chunk");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  lp<uint8_t> L = (lp<uint8_t>)smem;
  const uint32_t lutBytes = Cfg::lutBytes(pb);
  lp<uint16_t> ringAll = (lp<uint16_t>)(L + lutBytes);
  lp<uint16_t> segAll = (lp<uint16_t>)(L + lutBytes + Cfg::kRingBytes);
  lp<uint8_t> tiles = L + Cfg::ldsBytes(pb);

  const uint32_t tid = threadIdx.x;
  gp<const uint8_t> base = G(archive);

  // the headers, once per workgroup
  gp<const uint8_t> arch[S];
  uint32_t n;
  if (!mm::openTable<FT>(base, pb, numRows, rowWords, n, arch)) return;
  const uint32_t total = numRows * rowWords;          // the table's words: a multiple of 256
  const uint32_t nBlocks = divUp(n, kBlockSize);      // the element's blocks
  const uint32_t tBlocks = divUp(total, kBlockSize);  // ... that hold words of the table
  const uint32_t run = kGatherTasksPerWG * period;    // blocks of `period` task groups
  const uint32_t groups = divUp(tBlocks, run) * period;

  const uint32_t w = readfirst(tid >> 6), lane = tid & 63, l = lane & 31;
  const uint32_t hv = upperHalfMask(lane);
  const bool hi = lane >= 32;
  const bool vecIn = (reinterpret_cast<uintptr_t>(archive) & 15) == 0;
  gp<const uint8_t> raw = rawSectionOf(base);
  const uint32_t mask = (1u << pb) - 1;
  lp<const u32x2> lut[S];
  lut[0] = (lp<const u32x2>)L;

  buildLut64((gp<const uint16_t>)(arch[0] + kANSHeaderBytes), (lp<u32x2>)L, pb, (uint32_t*)segAll);
  __syncthreads();

  const uint32_t off = dec::kChunk * l;  // this lane's chunk in a segment
  // the multiply: this wave's m-tile, this lane's place (i, kg) in A, B and D
  const bool mine = 16 * w < mRows;  // wave-uniform
  const uint32_t li = lane & 15, kg = lane >> 4;
  gp<const uint8_t> xLane = G(x) + (16 * w + li < mRows ? uint64_t(16 * w + li) * xRowStrideBytes : 0u) + 16 * kg;
  // where this lane's chunk goes in a tile, and where its B operand comes from
  const uint32_t tileTo = (2 * w + (hi ? 1u : 0u)) * mmt::kTileRowBytes + 16 * l;
  const uint32_t tileFrom = (li & 7) * mmt::kTileRowBytes + 16 * kg;
  mmt::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  uint32_t buf = 0;  // the tile that the next segment fills

  // Persistent over the task groups, one generation of resident workgroups.
  // Everything that decides a barrier below is uniform over the workgroup.
  for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const uint32_t t0 = (grp / period) * run + grp % period;  // half 0's block, the lowest
    if (t0 >= tBlocks) continue;
    // only the element's last block is short, so half 0's is the longest
    const int32_t nSeg = int32_t(divUp(divUp(symbolsOfBlock(t0, n), 32), dec::kSegSteps));
    // the column of segment nSeg - 1 in its row, in every half
    uint32_t col = ((t0 * kBlockSize) % rowWords + uint32_t(nSeg - 1) * dec::kSegWords) % rowWords;

    // per half of this wave (wave-uniform): block and its size (0: the half idles)
    uint32_t bkH[2], uwH[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t t = t0 + period * (2 * w + hh);
      bkH[hh] = t < tBlocks ? t : 0u;
      uwH[hh] = t < tBlocks ? symbolsOfBlock(t, n) : 0u;
    }
    // this lane's half: the block's top segment inside the table (whole: total
    // is a multiple of 256 and at most n); the segments above it, and all of
    // an idle half's, are zeros in the tile
    const uint32_t bkM = hi ? bkH[1] : bkH[0], uwM = hi ? uwH[1] : uwH[0];
    const uint32_t b0 = bkM * kBlockSize;
    const int32_t gTop = uwM ? int32_t(min(kBlockSize, total - b0) / dec::kSegWords) - 1 : -1;
    // the half whose column of D this lane holds: its block, top segment and
    // that segment's row
    const uint32_t bkS = t0 + period * li;
    int32_t gTopS = -1;
    uint32_t rowS = 0;
    if (li < kGatherTasksPerWG && bkS < tBlocks) {
      gTopS = int32_t(min(kBlockSize, total - bkS * kBlockSize) / dec::kSegWords) - 1;
      rowS = (bkS * kBlockSize + uint32_t(gTopS) * dec::kSegWords) / rowWords;
    }

    // states and block-words entries
    const AnsSections arc(arch[0], nBlocks);
    const uint32_t x0 = uwM ? ((gp<const uint32_t>)(arc.states + uint64_t(kStateBytesPerBlock) * bkM))[l] : kMinState;
    uint2 bwE[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) bwE[hh] = uwH[hh] ? ld8(arc.bwords + bkH[hh]) : make_uint2(0, 0);

    // segments [0, nFull) are full for both halves' blocks: unmasked steps;
    // at and above nMine neither half has a word
    const uint32_t nFull = min(uwH[0], uwH[1]) / dec::kSegWords;
    const int32_t nMine = int32_t(divUp(max(uwH[0], uwH[1]), dec::kSegWords));

    DStream st[S];
    lp<uint16_t> segLane[S];
    DStream* chains[S];
    bindStream(st[0], segLane[0], ringAll, segAll, w, hv, l);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) openHalf(st[0], hh, arc.words, bwE[hh], uwH[hh] != 0, lane, vecIn);
    st[0].x = x0;
    chains[0] = &st[0];
    // this lane's chunk of its half's segment buffer
    lp<const uint16_t> q0 = segLane[0] - l + off;

    for (int32_t g = nSeg - 1; g >= 0; --g) {
      const bool full = uint32_t(g) < nFull;
      const bool live = g <= gTop;  // the segment holds words of the table
      const uint32_t i0 = b0 + uint32_t(g) * dec::kSegWords + off;
      // the chunk's raw float bytes and the wave's A operands, loaded ahead of
      // the segment's steps
      uint32_t rv[R];
      if (vecIn && live) J::load(rv, raw, n, i0);
      u32x4 xa[mmt::kKSteps];
      if (mine) {
        gp<const uint8_t> p = xLane + 2 * col;
#pragma unroll
        for (int s = 0; s < int(mmt::kKSteps); ++s) xa[s] = *(gp<const u32x4>)(p + 64 * s);
      }
      if (g < nMine) {
        const int32_t tBot = g * int32_t(dec::kSegSteps);
#pragma unroll
        for (int sg = int(dec::kSegSteps / dec::kUnroll) - 1; sg >= 0; --sg) {
          ringEnsure(st[0], lane, vecIn);
          // a partial segment, or a half that idles: masked steps
          if (full) decSteps<false, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), 0, l, 0u);
          else decSteps<true, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), tBot, l, uwM);
        }
      }
      __builtin_amdgcn_wave_barrier();
      // join the chunk's 8 words (dwords in memory order) into the tile
      uint32_t ww[D];
#pragma unroll
      for (int k = 0; k < D; ++k) ww[k] = 0;
      if (live) {
        if (vecIn) {
          uint32_t sv[4], sv1[4];
          loadChunkSyms<S>(q0, q0, sv, sv1);
          J::words(ww, sv, sv1, rv);
        } else {
#pragma unroll
          for (int k = 0; k < int(dec::kChunk); ++k)
            ww[k >> 1] |= uint32_t(J::one(q0[k] >> 8, 0, raw, n, i0 + k)) << (16 * (k & 1));
        }
      }
      lp<uint8_t> tile = tiles + buf * mmt::kTileBytes;
      *(lp<u32x4>)(tile + tileTo) = u32x4{ww[0], ww[1], ww[2], ww[3]};
      // The one barrier of the segment.  The tile filled two segments ago is
      // free: every wave has passed the barrier between, after its reads.
      __syncthreads();
      const bool end = col == 0 || g == 0;  // the end of a piece, in every half
      if (mine) {
#pragma unroll
        for (int s = 0; s < int(mmt::kKSteps); ++s) {
          u32x4 b = u32x4{0, 0, 0, 0};
          if (li < kGatherTasksPerWG) b = *(lp<const u32x4>)(tile + tileFrom + 64 * s);
          acc = mmt::mfma<FT>(xa[s], b, acc);
        }
        if (end) {
          if (g <= gTopS) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const uint32_t m = 16 * w + 4 * kg + uint32_t(v);
              if (m < mRows) G(part)[m * pieces + bkS + rowS] = acc[v];
            }
          }
          acc = mmt::f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      // the segment below: the same row, or the end of the row before it
      if (col == 0) {
        if (g <= gTopS) --rowS;
        col = rowWords - dec::kSegWords;
      } else {
        col -= dec::kSegWords;
      }
      buf ^= 1;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace dietgpu
