// Matmul on a compressed weight table for gfx950: W a
// [R, rowWords] table stored as one dense float archive, x [M, rowWords] a few
// activation rows in device memory,
//
//   out[m * outRowStride + r] = round_out(sum_k f(x[m, k]) * f(W[r, k]))
//
// f the exact conversion to fp32, every product and add one fp32 fmaf, one
// rounding to the output type.  The decoded matrix never exists in memory: the
// lane that has just joined 8 words of a row multiplies them into the matching
// 8 words of each activation row and keeps the partial dot products in
// registers.
//
// A fourth outer loop around k_decode's block body (decode.h), after k_decode's
// own, k_gather's (gather.h) and k_gatherSum's (gather_sum.h): openArchive,
// buildLut64, bindStream / openHalf, ringEnsure, decSteps and the 8-word chunk
// join (loadChunkSyms, Join::words; Join::one where the archive is 4 B off
// 16 B) are theirs.  What this file holds is what differs:
//  * a task is a 4096-word block of the table, one per half-wave, eight per
//    workgroup; with rowWords a multiple of 256 every segment of a block lies in
//    one row, so a block is 1 .. 16 row *pieces*, each a run of segments;
//  * the 8 words of x[m] that go with a lane's chunk are loaded before the
//    segment's decode steps (16 B per row, two for fp32; coalesced over the
//    half, L2-resident) and are in flight while the state chain runs;
//  * at the end of a piece the half reduces each accumulator over its 32 lanes
//    in one fixed tree (four DPP steps and a swizzle) and lane m stores sum m
//    to part[m][b + r], b the block and r the row: rows and blocks are both
//    consecutive intervals of the word line, so the id is unique, below
//    R + nBlocks, and the pieces of one row have consecutive ids;
//  * k_matmulFinish adds a row's pieces in ascending order, rounds once and
//    stores.  Two launches, no atomics and no arrival counter: the order of the
//    adds is a function of (rowWords, r) alone, and the call can be captured.
// No matrix instructions: an MFMA shares one B operand across its 16 or 32
// output columns, and here a wave holds two weight rows, one per half, each at
// its own k range.  k_matmulTile (matmul_tile.h) assigns the
// blocks so that a workgroup holds eight rows at one k range, and uses them.
#pragma once

#include "decode.h"
#include "decode_plan.h"

namespace dietgpu {

namespace mm {

// The sum of v over the 32 lanes of each half-wave, in every lane of the half:
// xor 1, xor 2, mirror in 8, mirror in 16 (DPP), xor 16 (swizzle).  Partners
// add the same two values, so all lanes hold the same bits.  Whole wave.
__device__ __forceinline__ float halfSum(float v) {
  auto f = [](int x) __attribute__((always_inline)) { return __builtin_bit_cast(float, x); };
  auto i = [](float x) __attribute__((always_inline)) { return __builtin_bit_cast(int, x); };
  v += f(__builtin_amdgcn_mov_dpp(i(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v += f(__builtin_amdgcn_mov_dpp(i(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v += f(__builtin_amdgcn_mov_dpp(i(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  v += f(__builtin_amdgcn_mov_dpp(i(v), 0x140, 0xF, 0xF, true));  // row_mirror
  v += f(__builtin_amdgcn_ds_swizzle(i(v), 0x401F));              // lane ^ 16 within 32
  return v;
}

// dwords of 8 words of x / of W
template <int FT>
constexpr int kDwords = FT == 3 ? 8 : 4;

// acc += sum over the chunk's 8 words of x * w, word 0 first
template <int FT>
__device__ __forceinline__ float fma8(float acc, const uint32_t (&xw)[kDwords<FT>], const uint32_t (&ww)[kDwords<FT>]) {
  using J = Join<FT, 0>;
#pragma unroll
  for (int k = 0; k < kDwords<FT>; ++k) {
    if constexpr (FT == 3) {
      acc = __builtin_fmaf(__builtin_bit_cast(float, xw[k]), __builtin_bit_cast(float, ww[k]), acc);
    } else {
      acc = __builtin_fmaf(J::widen(xw[k]), J::widen(ww[k]), acc);
      acc = __builtin_fmaf(J::widen(xw[k] >> 16), J::widen(ww[k] >> 16), acc);
    }
  }
  return acc;
}

// whether the headers are a float archive of type FT at precision pb that
// holds numRows rows of rowWords words; n: the element's size
template <int FT>
__device__ __forceinline__ bool openTable(gp<const uint8_t> base, int pb, uint32_t numRows, uint32_t rowWords,
                                          uint32_t& n, gp<const uint8_t> (&arch)[1]) {
  bool ok;
  n = openArchive<FT>(base, pb, ok, arch);
  return ok && uint64_t(numRows) * rowWords <= n;
}

}  // namespace mm

// grid planMatmul().gridX (decode_plan.h), dynamic LDS DecCfg<FT>::ldsBytes(pb).
// One pass: rows x[0 .. mRows), mRows <= MT, against every row of the table;
// the row sums of piece (block b, row r) go to part[m * pieces + b + r].
// rowWords a positive multiple of dec::kSegWords, numRows * rowWords < 2^32, x
// and xRowStrideBytes multiples of 16.  A call whose headers fail k_decode's
// checks, or whose table does not fit the element, writes nothing
// (k_matmulFinish makes the same checks and writes the status).
// Rows m >= mRows read x row 0 and are stored nowhere.
template <int FT, int MT>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(4))) void k_matmulRows(
    const uint8_t* __restrict__ archive, uint32_t numRows, uint32_t rowWords, const uint8_t* __restrict__ x,
    uint64_t xRowStrideBytes, uint32_t mRows, float* __restrict__ part, uint32_t pieces, int pb) {
  static_assert(FT >= 1 && FT <= 3 && MT >= 1 && MT <= 32, "fp16, bf16 and fp32; lane m stores row m's sum");
  using Cfg = DecCfg<FT>;
  using WordT = typename FloatTraits<FT>::WordT;
  using J = Join<FT, 0>;
  constexpr int S = Cfg::S, R = J::kR, D = mm::kDwords<FT>;
  static_assert(S == 1 && J::kW == D, "one ANS stream per word");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  lp<uint8_t> L = (lp<uint8_t>)smem;
  const uint32_t lutBytes = Cfg::lutBytes(pb);
  lp<uint16_t> ringAll = (lp<uint16_t>)(L + lutBytes);
  lp<uint16_t> segAll = (lp<uint16_t>)(L + lutBytes + Cfg::kRingBytes);

  const uint32_t tid = threadIdx.x;
  gp<const uint8_t> base = G(archive);

  // the headers, once per workgroup
  gp<const uint8_t> arch[S];
  uint32_t n;
  if (!mm::openTable<FT>(base, pb, numRows, rowWords, n, arch)) return;
  const uint32_t total = numRows * rowWords;               // the table's words: a multiple of 256
  const uint32_t nBlocks = divUp(n, kBlockSize);           // the element's blocks
  const uint32_t tBlocks = divUp(total, kBlockSize);       // ... that hold words of the table: the tasks
  const uint32_t groups = divUp(tBlocks, kGatherTasksPerWG);

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
  // x row m (wave-uniform; a row past the pass's reads row 0)
  auto xRow = [&](int m) __attribute__((always_inline)) {
    return G(x) + (uint32_t(m) < mRows ? uint64_t(m) * xRowStrideBytes : 0u);
  };
  float acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = 0.f;

  // Persistent over the task groups, one generation of resident workgroups.
  // No workgroup barrier below: the waves run their tasks independently.
  for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    // per half (wave-uniform): block and its size (0: the half idles)
    uint32_t bkH[2], uwH[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t t = grp * kGatherTasksPerWG + 2 * w + hh;
      bkH[hh] = t < tBlocks ? t : 0u;
      uwH[hh] = t < tBlocks ? symbolsOfBlock(t, n) : 0u;
    }
    if (uwH[0] == 0 && uwH[1] == 0) continue;

    // this lane's half
    const uint32_t bkM = hi ? bkH[1] : bkH[0], uwM = hi ? uwH[1] : uwH[0];
    const uint32_t b0 = bkM * kBlockSize;
    // the block's top segment inside the table (whole: total is a multiple of
    // 256 and at most n), its row and its first column in that row.  Segments
    // above it are decoded for the state chain alone.
    int32_t gTop = -1;
    uint32_t rowM = 0, colM = 0;
    if (uwM) {
      gTop = int32_t(min(kBlockSize, total - b0) / dec::kSegWords) - 1;
      const uint32_t s = b0 + uint32_t(gTop) * dec::kSegWords;
      rowM = s / rowWords;
      colM = s - rowM * rowWords;
    }

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
    // this lane's chunk of its half's segment buffer
    lp<const uint16_t> q0 = segLane[0] - l + off;

    for (int32_t g = nSeg - 1; g >= 0; --g) {
      const bool full = uint32_t(g) < nFull;
      const bool live = g <= gTop;  // the segment holds words of the table
      const uint32_t i0 = b0 + uint32_t(g) * dec::kSegWords + off;
      // the chunk's raw float bytes and its words of every x row, loaded ahead
      // of the segment's steps (an idle lane reads the head of its x rows)
      uint32_t rv[R];
      if (vecIn && live) J::load(rv, raw, n, i0);
      uint32_t xw[MT][D];
      {
        const uint32_t cb = ((live ? colM : 0u) + off) * uint32_t(sizeof(WordT));
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          gp<const u32x4> p = (gp<const u32x4>)(xRow(m) + cb);
#pragma unroll
          for (int j = 0; j < D / 4; ++j) {
            const u32x4 v = p[j];
            xw[m][4 * j] = v.x; xw[m][4 * j + 1] = v.y; xw[m][4 * j + 2] = v.z; xw[m][4 * j + 3] = v.w;
          }
        }
      }
      const int32_t tBot = g * int32_t(dec::kSegSteps);
#pragma unroll
      for (int sg = int(dec::kSegSteps / dec::kUnroll) - 1; sg >= 0; --sg) {
        ringEnsure(st[0], lane, vecIn);
        // a partial segment, or a half that idles: masked steps
        if (full) decSteps<false, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), 0, l, 0u);
        else decSteps<true, S>(chains, lut, mask, pb, hv, segLane, sg * int(dec::kUnroll), tBot, l, uwM);
      }
      __builtin_amdgcn_wave_barrier();
      if (live) {
        // join the chunk's 8 words (dwords in memory order) and multiply
        uint32_t ww[D];
        if (vecIn) {
          uint32_t sv[4], sv1[4];
          loadChunkSyms<S>(q0, q0, sv, sv1);
          J::words(ww, sv, sv1, rv);
        } else {
#pragma unroll
          for (int k = 0; k < D; ++k) ww[k] = 0;
#pragma unroll
          for (int k = 0; k < int(dec::kChunk); ++k) {
            const uint32_t v = J::one(q0[k] >> 8, 0, raw, n, i0 + k);
            if constexpr (FT == 3) ww[k] = v;
            else ww[k >> 1] |= v << (16 * (k & 1));
          }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mm::fma8<FT>(acc[m], xw[m], ww);
      }
      // the end of a piece: the segment is its row's first, or the block's last
      const bool end = live && (colM == 0 || g == 0);
      if (ballot(end) != 0) {
        float mine = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const float s = mm::halfSum(acc[m]);
          mine = l == uint32_t(m) ? s : mine;
        }
        if (end) {
          if (l < mRows) G(part)[l * pieces + bkM + rowM] = mine;
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m] = 0.f;
        }
      }
      // the segment below: the same row, or the end of the row before it
      if (live) {
        if (colM == 0) --rowM, colM = rowWords - dec::kSegWords;
        else colM -= dec::kSegWords;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// grid divUp(mRows * numRows, 256) x 256 threads, one per (m, r).  Row r's
// pieces part[m * pieces + r + b], b its first block .. its last, are added in
// ascending order in fp32, rounded once and stored to out[m * outRowStride + r]
// (OUT32: fp32 words, else the archive's 16-bit type).  The checks are
// k_matmulRows': on failure nothing but the status is written.  outSuccess
// (optional): one byte, by thread 0.
template <int FT, bool OUT32>
__global__ __launch_bounds__(dec::kThreads) void k_matmulFinish(const uint8_t* __restrict__ archive, uint32_t numRows,
                                                               uint32_t rowWords, uint32_t mRows,
                                                               const float* __restrict__ part, uint32_t pieces,
                                                               uint8_t* out, uint64_t outRowStride, int pb,
                                                               uint8_t* outSuccess) {
  static_assert(FT >= 1 && FT <= 3 && (OUT32 || FT != 3), "fp16, bf16 and fp32; fp32 products leave as fp32");
  using J = Join<FT, 0>;
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  gp<const uint8_t> arch[1];
  uint32_t n;
  const bool ok = mm::openTable<FT>(G(archive), pb, numRows, rowWords, n, arch);
  const uint32_t i = blockIdx.x * dec::kThreads + threadIdx.x;
  if (i == 0 && outSuccess) G(outSuccess)[0] = ok ? 1 : 0;
  if (!ok || i >= mRows * numRows) return;
  const uint32_t m = i / numRows, r = i - m * numRows;
  const uint32_t s0 = r * rowWords;
  const uint32_t bFirst = s0 / kBlockSize, bLast = (s0 + rowWords - 1) / kBlockSize;
  gp<const float> p = G(part) + (m * pieces + r);
  float sum = p[bFirst];
  for (uint32_t b = bFirst + 1; b <= bLast; ++b) sum += p[b];
  gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(m) * outRowStride + r);
  if constexpr (OUT32) *o = __builtin_bit_cast(uint32_t, sum);
  else if constexpr (FT == 1) *o = __builtin_bit_cast(uint16_t, _Float16(sum));
  else *o = uint16_t(J::bf16Of(sum));
}

}  // namespace dietgpu
