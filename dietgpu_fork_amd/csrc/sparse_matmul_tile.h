// Matmul on a sparse weight archive through the matrix pipe, for gfx950
// (DESIGN.md 5.2o): W a [R, rowWords] table, the first R * rowWords words of
// the element of one sparse fp16 / bf16 archive, x [M, rowWords], 1 <= M <= 64,
//
//   out[m * outRowStride + r] = round_out(sum_k x[m, k] * W[r, k])
//
// the products exact, the sums fp32 (v_mfma_f32_16x16x32_{f16,bf16}), one
// rounding to the output type, and ONE pass over the decoded nonzero list and
// the bitmap whatever M is (k_sparseMatmul, sparse_matmul.h, makes one per eight
// rows of x).  A clear bitmap bit is a +0.0 weight word here and IS multiplied:
// the A operand of an MFMA is shared by its 16 weight rows, so x cannot be
// masked per row, and an Inf or NaN of x over a zero of W gives NaN as in a
// dense product.  That is the one difference from k_sparseMatmul's contract.
//
// After k_sparseChunks and the dense decode of the list (sparse_matmul_tile.hip):
//  * k_sparseChunkOffsets, one thread per chunk of the table: the chunk's list
//    offset, chunkPre[c] + the totals of the counting workgroups before c's,
//    so that the tiles read one word per chunk where chunkListOffset makes a
//    wave sum per chunk (a wave here meets up to eight chunks per task);
//  * k_sparseMatmulTile, one workgroup per task = (16 weight rows) x (a slice
//    of up to 1024 columns, 1 .. 4 groups of 256).  Per group, ascending: wave
//    w expands weight rows 4 w .. 4 w + 3 at the group's columns.  Each of
//    these four runs of 256 words is 256-aligned in the word line, four bitmap
//    words of one chunk: lane 16 q + i loads bitmap word i of run q's chunk
//    (cut at R * rowWords) beside the chunk's list offset, a 16-lane DPP
//    prefix of the popcounts gives every line's list base, and the 16 gathers
//    go out back to back with one counted wait.  The bitmap words of all the
//    slice's groups are loaded before the first gather.  The wave writes its
//    four rows into an LDS tile Wt[16][256] (rows mmt::kTileRowBytes apart;
//    two tiles, one workgroup barrier per group), then wave w multiplies its
//    activation rows 16 w .. 16 w + 15 (A operands from global memory, loaded
//    before the gathers' wait) into D[16][16] with eight MFMAs, s ascending:
//    all 16 columns of B are weight rows.  After the slice's last group the
//    lanes store D[m][n] to part[(m R + r) slices + slice];
//  * k_sparseMatmulTileFinish, one thread per (m, r): the status, then the
//    row's slices added in ascending order, one rounding, one store.
// A row m of x meets one wave, one accumulator and the groups in one order
// whatever M is; a weight row r meets column r % 16 of B and the slices of
// rowWords whatever R is and whatever else the table holds: the order is a
// function of rowWords alone.  No atomics, no wait between workgroups.
#pragma once

#include "matmul_tile.h"
#include "sparse_matmul.h"

namespace dietgpu {

struct SparseMatmulTileArgs {
  SparseMatmulArgs t;        // k_sparseMatmul's (pieces: the slices of a row)
  const uint32_t* chunkOff;  // k_sparseChunkOffsets' list offset of every chunk of the table
};

namespace smt {

constexpr uint32_t kBlockRows = 16;                                  // weight rows of a task: the columns of B
constexpr uint32_t kSliceWords = 1024;                               // columns of a task
constexpr uint32_t kSliceGroups = kSliceWords / smm::kGroupWords;    // groups of a whole slice
constexpr uint32_t kWaveRows = kBlockRows / kWaves;                  // weight rows a wave expands
constexpr uint32_t kTileBytes = kBlockRows * mmt::kTileRowBytes;
static_assert(kWaveRows * smm::kGroupLines == kChunkRows && kWaveRows * 16 == 64,
              "16 lines per wave and group, a run's chunk bitmap in 16 lanes");

// inclusive sum over the lanes of a row of 16 (DPP row_shr: zeros shift in)
__device__ __forceinline__ uint32_t rowInclusiveScan(uint32_t v) {
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, true));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, true));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, true));
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, true));
  return v;
}

}  // namespace smt

// grid planSparseMatmulTile().cblocks x 256 threads, after k_sparseChunks:
// chunkOff[c] = chunkPre[c] + blockTot[0] + .. + blockTot[c / 256 - 1] for the
// `chunks` chunks of the table.
static __global__ __launch_bounds__(kThreads) void k_sparseChunkOffsets(const uint32_t* __restrict__ chunkPre,
                                                                 const uint32_t* __restrict__ blockTot,
                                                                 uint32_t chunks, uint32_t* __restrict__ chunkOff) {
  __shared__ uint32_t red[kWaves];
  const uint32_t g = blockIdx.x;
  uint32_t share = 0;
  for (uint32_t k = threadIdx.x; k < g; k += kThreads) share += G(blockTot)[k];
  const uint32_t before = blockSum<kThreads>(share, red);
  const uint32_t c = g * kThreads + threadIdx.x;
  if (c < chunks) G(chunkOff)[c] = before + G(chunkPre)[c];
}

// grid planSparseMatmulTile().tasks x 256 threads; task = blockIdx.x: row block
// task / slices, slice task % slices.  x and xRowStrideBytes are multiples of
// 16, rowWords a positive multiple of 256, numRows * rowWords < 2^32, M <= 64.
// A call that fails smm::openTable writes nothing (the finish makes the same
// checks and writes the status).  Bitmap words at or past numRows * rowWords
// are not read, and no gather's index reaches listCapacity, whatever a corrupt
// bitmap counts: such a word is a zero.
template <int FT>
__global__ __launch_bounds__(kThreads) void k_sparseMatmulTile(SparseMatmulTileArgs a, const uint8_t* __restrict__ x,
                                                               uint64_t xRowStrideBytes, uint32_t M,
                                                               float* __restrict__ part) {
  static_assert(FT == 1 || FT == 2, "the 16-bit types of v_mfma_f32_16x16x32");
  using W = WordOf<FT>;
  __shared__ __attribute__((aligned(16))) uint8_t tiles[2 * smt::kTileBytes];
  uint32_t n;
  if (!smm::openTable(a.t, n)) return;  // uniform over the grid
  const uint32_t R = a.t.numRows, K = a.t.rowWords, slices = a.t.pieces;
  const uint32_t total = R * K;  // a multiple of 256, at most n
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t rb = blockIdx.x / slices, slice = blockIdx.x - rb * slices;
  const uint32_t col0 = slice * smt::kSliceWords;
  const uint32_t groups = min(smt::kSliceGroups, (K - col0) / smm::kGroupWords);  // 1 .. 4, uniform

  gp<const uint8_t> bm = G(a.t.archive) + kSparseHeaderBytes;
  gp<const W> list = (gp<const W>)G(a.t.list);
  const bool gap = n == total && gapBit(bm, n);  // word n - 1 is a table word iff n == total

  // This lane's run: weight row 4 w + q of the block, q = lane / 16; of its
  // chunk's bitmap this lane holds word lane % 16.
  const uint32_t rowQ = rb * smt::kBlockRows + smt::kWaveRows * w + (lane >> 4);
  // the multiply: this wave's m-tile, this lane's place (i, kg) in A, B and D
  const bool mine = 16 * w < M;  // wave-uniform
  const uint32_t li = lane & 15, kg = lane >> 4;
  gp<const uint8_t> xLane =
      G(x) + (16 * w + li < M ? uint64_t(16 * w + li) * xRowStrideBytes : 0u) + 2 * col0 + 16 * kg;
  lp<uint8_t> tileAll = (lp<uint8_t>)tiles;
  const uint32_t tileTo = smt::kWaveRows * w * mmt::kTileRowBytes + 2 * lane;
  const uint32_t tileFrom = li * mmt::kTileRowBytes + 16 * kg;

  // the bitmap words and line bases of every group of the slice, in flight together
  uint64_t mv[smt::kSliceGroups];
  uint32_t off[smt::kSliceGroups];
#pragma unroll
  for (uint32_t g = 0; g < smt::kSliceGroups; ++g) {
    mv[g] = 0;
    off[g] = 0;
    if (g < groups && rowQ < R) {
      const uint32_t i0 = rowQ * K + col0 + g * smm::kGroupWords;  // below total
      const uint32_t c = i0 / kChunkWords;
      mv[g] = chunkBitmapWord(bm, c, total - c * kChunkWords, li);
      off[g] = G(a.chunkOff)[c];
    }
  }

  mmt::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (uint32_t g = 0; g < smt::kSliceGroups; ++g) {
    if (g < groups) {
      // the wave's A operands of this group
      u32x4 xa[mmt::kKSteps];
      if (mine) {
#pragma unroll
        for (int s = 0; s < int(mmt::kKSteps); ++s)
          xa[s] = *(gp<const u32x4>)(xLane + 2 * smm::kGroupWords * g + 64 * s);
      }
      // every line's list base: the chunk's offset + the set bits of its lines before
      const uint32_t cnt = uint32_t(__popcll(mv[g]));
      const uint32_t lineBase = off[g] + smt::rowInclusiveScan(cnt) - cnt;
      W v[kChunkRows];
#pragma unroll
      for (uint32_t q = 0; q < smt::kWaveRows; ++q) {
        // run q (wave-uniform): its first word and the line that holds it in
        // its chunk, 0, 4, 8 or 12 (a row at or past R has an empty bitmap:
        // its words are zeros whatever i0 wraps to)
        const uint32_t i0 = (rb * smt::kBlockRows + smt::kWaveRows * w + q) * K + col0 + g * smm::kGroupWords;
        const uint32_t l0 = 16 * q + ((i0 / 64) & 12);
#pragma unroll
        for (uint32_t t = 0; t < smm::kGroupLines; ++t) {
          const int L = int(l0 + t);
          const uint64_t m = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(mv[g] >> 32)), L))) << 32) |
                             uint32_t(__builtin_amdgcn_readlane(int(uint32_t(mv[g])), L));
          uint32_t src = uint32_t(__builtin_amdgcn_readlane(int(lineBase), L)) + mbcnt(m);
          if (gap && i0 + 64 * t + lane + 1 == n) src += 1;
          v[smm::kGroupLines * q + t] = ((m >> lane) & 1) && src < a.t.listCapacity ? list[src] : W(0);
        }
      }
      // one wait for the 16 gathers, then the wave's four rows of the tile
      lp<uint8_t> tile = tileAll + (g & 1) * smt::kTileBytes;
#pragma unroll
      for (uint32_t j = 0; j < kChunkRows; ++j) landed(v[j]);
#pragma unroll
      for (uint32_t j = 0; j < kChunkRows; ++j)
        *(lp<W>)(tile + tileTo + (j / smm::kGroupLines) * mmt::kTileRowBytes + 128 * (j % smm::kGroupLines)) = v[j];
      // The one barrier of the group.  The tile filled two groups ago is free:
      // every wave has passed the barrier between, after its reads.
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int s = 0; s < int(mmt::kKSteps); ++s)
          acc = mmt::mfma<FT>(xa[s], *(lp<const u32x4>)(tile + tileFrom + 64 * s), acc);
      }
    }
  }

  const uint32_t r = rb * smt::kBlockRows + li;
  if (mine && r < R) {
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) {
      const uint32_t m = 16 * w + 4 * kg + v;
      if (m < M) G(part)[(m * R + r) * slices + slice] = acc[v];
    }
  }
}

// grid planSparseMatmulTile().finishGrid x 256 threads, one per (m, r).  Row
// r's slices part[(m R + r) slices + s], s ascending, are added in fp32,
// rounded once and stored to out[m * outRowStride + r] (OUT32: fp32 words,
// else the archive's 16-bit type).  The checks are k_sparseMatmulTile's: on
// failure nothing but the status is written.  outSuccess (optional): one byte,
// by thread 0.
template <int FT, bool OUT32>
__global__ __launch_bounds__(kThreads) void k_sparseMatmulTileFinish(SparseMatmulTileArgs a, uint32_t M,
                                                                     const float* __restrict__ part, uint8_t* out,
                                                                     uint64_t outRowStride, uint8_t* outSuccess) {
  static_assert(FT == 1 || FT == 2, "fp16 and bf16");
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  uint32_t n;
  const bool ok = smm::openTable(a.t, n);
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0 && outSuccess) G(outSuccess)[0] = ok ? 1 : 0;
  if (!ok || i >= M * a.t.numRows) return;
  const uint32_t m = i / a.t.numRows, r = i - m * a.t.numRows;
  gp<const float> p = G(part) + uint64_t(i) * a.t.pieces;
  float sum = p[0];
  for (uint32_t s = 1; s < a.t.pieces; ++s) sum += p[s];
  gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(m) * outRowStride + r);
  if constexpr (OUT32) *o = __builtin_bit_cast(uint32_t, sum);
  else if constexpr (FT == 1) *o = __builtin_bit_cast(uint16_t, _Float16(sum));
  else *o = uint16_t(Join<FT, 0>::bf16Of(sum));
}

}  // namespace dietgpu
