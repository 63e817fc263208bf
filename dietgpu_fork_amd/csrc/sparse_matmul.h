// Matmul on a sparse weight archive for gfx950: W a
// [R, rowWords] table, the first R * rowWords words of the element of one
// sparse float archive (nonzero bitmap + a dense archive of the compacted
// nonzeros), x [M, rowWords] a few activation rows in device memory,
//
//   out[m * outRowStride + r] = round_out(sum over k with bit(r * rowWords + k) set of f(x[m, k]) * f(W[r, k]))
//
// f the exact conversion to fp32, every term one fp32 fmaf, one rounding to the
// output type.  A clear bitmap bit is skipped, not multiplied (the sparse
// codec's rule): neither the list nor x is read there, so an Inf or NaN of x
// under a clear bit does not reach out.  The expanded matrix never exists in
// memory.
//
// The nonzero list is decoded once into scratch by the dense decoder
// (sparse_matmul.hip), whatever M is.  Then
//  * k_sparseMatmul, one wave per 1024-word chunk of the table like
//    k_sparseExpand and k_sparseReduce (sparse.hip), no LDS and no barrier:
//    lanes 0-15 load the chunk's 16 bitmap words beside its list offset,
//    expandRows (sparse_expand.h) issues the 16 list gathers, and its row hook
//    the x words of the same 16 lines for MT activation rows -- lane l, line j
//    reads x[m][col + 64 j + l], one coalesced line per row, masked by the bit
//    -- so everything the chunk needs is in flight in one memory round trip.
//    rowWords is a multiple of 256, so the four lines of a 256-word group lie
//    in one table row and a chunk is 1 .. 4 *pieces*, each a run of groups of
//    one row.  Per lane and m: acc = fmaf(x, w, acc) over the piece's lines
//    ascending, a select where the bit is clear; at the piece's end one fixed
//    64-lane tree (mm::halfSum and one cross-half add, lower half first), and
//    lane m stores sum m to part[m][c + r], c the chunk and r the row: chunks
//    and rows are both consecutive intervals of the word line, so the id is
//    unique and below R + chunks (matmul.h).  Rows of x beyond MT are further
//    passes (blockIdx.y) over the same scratch list.
//  * k_sparseMatmulFinish, one thread per (m, r): the status, then row r's
//    pieces added in ascending order, one rounding, one store.
// No atomics, no arrival counter, no wait between workgroups: the order of the
// adds is a function of (rowWords, r) alone, and the call can be captured.
#pragma once

#include "matmul.h"
#include "sparse_expand.h"

namespace dietgpu {

// What both kernels read beside x, part and out.
struct SparseMatmulArgs {
  const uint8_t* archive;  // the sparse archive, 16 B-aligned
  uint32_t numRows, rowWords;
  uint32_t chunks, cblocks;  // the table's chunks and their counting workgroups (planSparseMatmul)
  const uint32_t* chunkPre;  // k_sparseChunks' prefixes and totals of this archive
  const uint32_t* blockTot;
  const uint8_t* list;       // the decoded nonzero list
  uint32_t listCapacity;     // ... its words: no gather goes past them
  const uint8_t* denseOk;    // the dense decode's verdict: valid for the config, and the list fits
  uint32_t pieces;
};

namespace smm {

// Whether the call goes on: a sparse header (sparseSizeOf) whose element holds
// the table, and a dense part that passed k_decode's checks and fits the list
// capacity.  n: the element's words.
__device__ __forceinline__ bool openTable(const SparseMatmulArgs& a, uint32_t& n) {
  bool hdrOk;
  n = sparseSizeOf(G(a.archive), hdrOk);
  return hdrOk && a.denseOk[0] != 0 && uint64_t(a.numRows) * a.rowWords <= n;
}

template <int FT>
__device__ __forceinline__ float asFloat(uint32_t w) {
  if constexpr (FT == 3) return __builtin_bit_cast(float, w);
  else return Join<FT, 0>::widen(w);
}

// The sum of v over the 64 lanes in one fixed tree: each half's 32 lanes
// (mm::halfSum), then lower half + upper half.  Wave-uniform result.
__device__ __forceinline__ float waveSum64(float v) {
  const int s = __builtin_bit_cast(int, mm::halfSum(v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 0)) +
         __builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 32));
}

constexpr uint32_t kGroupWords = 256;                       // the unit rowWords is a multiple of
constexpr uint32_t kGroupLines = kGroupWords / 64;          // lines (bitmap words) of a group
constexpr uint32_t kGroups = kChunkWords / kGroupWords;     // groups of a chunk: its most pieces

}  // namespace smm

// grid (planSparseMatmul().gridX, passes) x 256 threads.  Pass p = blockIdx.y
// serves rows m0 = p * MT .. min(m0 + MT, M) - 1 of x.  x and xRowStrideBytes
// are multiples of 16, rowWords a positive multiple of 256, numRows * rowWords
// < 2^32.  A call that fails openTable writes nothing (k_sparseMatmulFinish
// makes the same checks and writes the status).  Lines at or past numRows *
// rowWords are not read: their bitmap words are cut (chunkBitmapWord's limit).
// Every gather's index is held below listCapacity, whatever a corrupt bitmap
// counts.
template <int FT, int MT>
__global__ __launch_bounds__(kThreads) void k_sparseMatmul(SparseMatmulArgs a, const uint8_t* __restrict__ x,
                                                           uint64_t xRowStrideBytes, uint32_t M,
                                                           float* __restrict__ part) {
  static_assert(FT >= 1 && FT <= 3 && MT >= 1 && MT <= 32, "fp16, bf16 and fp32; lane m stores row m's sum");
  using W = WordOf<FT>;
  uint32_t n;
  if (!smm::openTable(a, n)) return;
  const uint32_t total = a.numRows * a.rowWords;  // a multiple of 256, at most n
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t c = blockIdx.x * kWaves + w;
  const uint32_t i0 = c * kChunkWords;
  if (c >= a.chunks || i0 >= total) return;
  const uint32_t m0 = blockIdx.y * MT;
  const uint32_t rows = min(uint32_t(MT), M - m0);

  gp<const uint8_t> bm = G(a.archive) + kSparseHeaderBytes;
  uint64_t mv = chunkBitmapWord(bm, c, total - i0, lane);
  const uint32_t base = chunkListOffset(G(a.chunkPre), G(a.blockTot), c, lane);
  // only the chunk holding word n-1 looks (it is a table word iff n == total)
  const bool gap = n - 1 - i0 < kChunkWords && gapBit(bm, n);
  // The chunk's gathers end at list word base + its set bits (+ 1 behind a
  // gap).  A bitmap that counts more than the list capacity holds (no
  // compressor writes one) gathers nothing: its sums are 0, and no read leaves
  // the scratch list.
  if (uint64_t(base) + waveSum(uint32_t(__popcll(mv))) + (gap ? 1u : 0u) > a.listCapacity) mv = 0;

  // the chunk's groups (wave-uniform): their rows, and their first columns
  const uint32_t live = min(smm::kGroups, (total - i0) / smm::kGroupWords);
  uint32_t rowG[smm::kGroups], colG[smm::kGroups];
  {
    uint32_t r = i0 / a.rowWords, col = i0 - r * a.rowWords;
#pragma unroll
    for (uint32_t g = 0; g < smm::kGroups; ++g) {
      rowG[g] = r;
      colG[g] = col;
      col += smm::kGroupWords;
      if (col == a.rowWords) col = 0, ++r;
    }
  }

  // the 16 gathers and, between them, the MT x 16 words of x: one round trip
  W v[kChunkRows];
  uint32_t xw[MT][kChunkRows];
  uint32_t taken16 = 0;  // bit j: this lane's word of line j has its bitmap bit set
  gp<const W> xRow[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
    xRow[m] = (gp<const W>)(G(x) + (uint32_t(m) < rows ? uint64_t(m0 + m) * xRowStrideBytes : 0u));
  gp<const W> list = (gp<const W>)G(a.list);
  // (mv holds no bit at or past total, so every gather of a set bit is wanted)
  expandRows(
      mv, base, i0, n, gap, list, lane, [](uint32_t) { return true; }, v,
      [&](uint32_t j, uint32_t, bool set) __attribute__((always_inline)) {
        taken16 |= (set ? 1u : 0u) << j;
        const uint32_t k = colG[j / smm::kGroupLines] + 64 * (j % smm::kGroupLines) + lane;
#pragma unroll
        for (int m = 0; m < MT; ++m) xw[m][j] = set && uint32_t(m) < rows ? uint32_t(xRow[m][k]) : 0u;
      });
  // one wait for all of them, where the wave has converged (k_sparseExpand's
  // accumulate form, DESIGN.md 5.2f "One wait")
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) {
    landed(v[j]);
#pragma unroll
    for (int m = 0; m < MT; ++m) landed(xw[m][j]);
  }

  float acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = 0.f;
#pragma unroll
  for (uint32_t g = 0; g < smm::kGroups; ++g) {
    if (g < live) {
#pragma unroll
      for (uint32_t q = 0; q < smm::kGroupLines; ++q) {
        const uint32_t j = g * smm::kGroupLines + q;
        const float wf = smm::asFloat<FT>(v[j]);
        const bool set = (taken16 >> j) & 1;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const float t = __builtin_fmaf(smm::asFloat<FT>(xw[m][j]), wf, acc[m]);
          acc[m] = set ? t : acc[m];
        }
      }
      // the end of a piece: the group is its row's last, or the chunk's last live one
      if (colG[g] + smm::kGroupWords == a.rowWords || g + 1 == live) {
        float mine = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const float s = smm::waveSum64(acc[m]);
          mine = lane == uint32_t(m) ? s : mine;
          acc[m] = 0.f;
        }
        if (lane < rows) G(part)[(m0 + lane) * a.pieces + c + rowG[g]] = mine;
      }
    }
  }
}

// grid planSparseMatmul().finishGrid x 256 threads, one per (m, r).  Row r's
// pieces part[m * pieces + r + c], c its first chunk .. its last, are added in
// ascending order in fp32, rounded once and stored to out[m * outRowStride + r]
// (OUT32: fp32 words, else the archive's 16-bit type).  The checks are
// k_sparseMatmul's: on failure nothing but the status is written.  outSuccess
// (optional): one byte, by thread 0.
template <int FT, bool OUT32>
__global__ __launch_bounds__(kThreads) void k_sparseMatmulFinish(SparseMatmulArgs a, uint32_t M,
                                                                 const float* __restrict__ part, uint8_t* out,
                                                                 uint64_t outRowStride, uint8_t* outSuccess) {
  static_assert(FT >= 1 && FT <= 3 && (OUT32 || FT != 3), "fp16, bf16 and fp32; fp32 products leave as fp32");
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  uint32_t n;
  const bool ok = smm::openTable(a, n);
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0 && outSuccess) G(outSuccess)[0] = ok ? 1 : 0;
  if (!ok || i >= M * a.numRows) return;
  const uint32_t m = i / a.numRows, r = i - m * a.numRows;
  const uint32_t s0 = r * a.rowWords;
  const uint32_t cFirst = s0 / kChunkWords, cLast = (s0 + a.rowWords - 1) / kChunkWords;
  gp<const float> p = G(part) + (m * a.pieces + r);
  float sum = p[cFirst];
  for (uint32_t c = cFirst + 1; c <= cLast; ++c) sum += p[c];
  gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(m) * outRowStride + r);
  if constexpr (OUT32) *o = __builtin_bit_cast(uint32_t, sum);
  else if constexpr (FT == 1) *o = __builtin_bit_cast(uint16_t, _Float16(sum));
  else *o = uint16_t(Join<FT, 0>::bf16Of(sum));
}

}  // namespace dietgpu
