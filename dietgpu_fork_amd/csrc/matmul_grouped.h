// Grouped matmul on compressed expert tables for gfx950: E
// weight tables W_e [R, rowWords], each one dense fp16 / bf16 archive of one
// shape, and activation rows x [T, rowWords] ordered by expert, expert e owning
// rows offsets[e] .. offsets[e + 1] - 1:
//
//   out[t * outRowStride + r] = round_out(sum_k x[t, k] * W_e[r, k])
//
// in one task line over the experts that have rows.  Three kernels, no host
// table, no atomics, no cross-workgroup wait:
//  * k_matmulGroupPlan, one workgroup: validates the offsets, opens every
//    archive's headers (ok[e]) and lists the entries (e, firstRow, count <= 64)
//    of the experts that are ok and have rows, an expert of more than 64 rows
//    as several.  The host knows only the bound E + T / 64 on their number;
//  * k_matmulTileGrouped<FT>: the task line is nEntries x groups, groups the
//    task groups of k_matmulTile for one table (planMatmulTile), and workgroup
//    wg takes the contiguous range [wg * total / grid, (wg + 1) * total / grid):
//    it crosses from an entry to the next at most once per entry in its range.
//    On a crossing it opens the entry's archive, rebuilds the decode table
//    between two workgroup barriers and takes its activation rows from the
//    entry.  The task body is a copy of k_matmulTile's (matmul_tile.h), kept
//    apart so that k_matmulTile's code stays as it is: with the archive, the
//    table and the rows loop-variant the compiler allocates its registers
//    anew.  A row sits at 16 * wave + i of its entry as it does in
//    matmul_tile(archive_e, x[the entry's rows]) and meets the same segments
//    and pieces in the same order: the bits are that call's;
//  * k_matmulFinishGrouped<FT, OUT32>, one thread per (t, r): finds t's expert
//    by binary search in the offsets, skips the row of a failed expert, adds
//    the row's pieces in k_matmulFinish's order and rounds once.
// Partials go to part[t * pieces + block + row], t the row of x: entries never
// collide.
#pragma once

#include "matmul_tile.h"

namespace dietgpu {

namespace mmg {

// the scratch's first words: what k_matmulGroupPlan leaves for the other two
enum : uint32_t { kHeadEntries = 0, kHeadBadOffsets = 1, kHeadWords = 4 };

// the slots of k_matmulTileGrouped's crossing context in LDS, 8 B each
enum : uint32_t { kCtxArchives, kCtxEntries, kCtxX, kCtxXStride, kCtxPart, kCtxSlots };

__host__ __device__ constexpr uint32_t ldsBytes(uint32_t decoderBytes) {
  return mmt::ldsBytes(decoderBytes) + 8 * kCtxSlots;
}

// a 64-bit value that every lane holds, as a scalar
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return uint64_t(readfirst(uint32_t(v))) | (uint64_t(readfirst(uint32_t(v >> 32))) << 32);
}

// buildLut64 (decode.h) for a table that is rebuilt inside a loop.  The same
// entries; what differs is the bound of the fill: 2^pb is a multiple of the
// workgroup's 256 threads, so whether a thread's slot lies inside the table is
// the same for the whole workgroup and is decided on the scalar side, as is
// which waves' totals come before a thread's in the scan.  The per-lane forms'
// lane masks are loop-invariant: they get hoisted out of the task loop and
// hold two scalar registers each over it, which k_matmulTileGrouped lacks.
__device__ __forceinline__ void rebuildLut64(gp<const uint16_t> pdfIn, lp<u32x2> lut, int pb, uint32_t* scratch) {
  static_assert(dec::kThreads == kNumSymbols, "one symbol per thread");
  uint32_t* cdfS = scratch;
  uint32_t* pdfS = scratch + kNumSymbols;
  uint32_t* red = scratch + 2 * kNumSymbols;
  const uint32_t tid = threadIdx.x;
  const uint32_t p = pdfIn[tid];
  // blockExclusiveScan with the wave's number and total on the scalar side too
  const uint32_t w = readfirst(tid >> 6);
  const uint32_t inc = waveInclusiveScan(p);
  __syncthreads();
  red[w] = uint32_t(__builtin_amdgcn_readlane(int(inc), 63));  // every lane the same word
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t i = 0; i < dec::kThreads / 64; ++i) before += i < w ? red[i] : 0u;
  pdfS[tid] = p;
  cdfS[tid] = before + inc - p;
  __syncthreads();
  constexpr int kG = 4;  // slots searched together
  const uint32_t total = 1u << pb;
#pragma unroll 1
  for (uint32_t u0 = 0; u0 < total; u0 += kG * dec::kThreads) {  // the round's first slot, uniform
    uint32_t s[kG], cs[kG];
#pragma unroll
    for (int j = 0; j < kG; ++j) s[j] = 0, cs[j] = 0;
#pragma unroll
    for (uint32_t bit = kNumSymbols / 2; bit; bit >>= 1) {
#pragma unroll
      for (int j = 0; j < kG; ++j) {
        const uint32_t cv = cdfS[s[j] + bit];
        const bool up = cv <= u0 + tid + j * dec::kThreads;
        s[j] = up ? s[j] + bit : s[j];
        cs[j] = up ? cv : cs[j];
      }
    }
#pragma unroll
    for (int j = 0; j < kG; ++j) {
      const uint32_t slot = u0 + tid + j * dec::kThreads;
      if (u0 + j * dec::kThreads < total) lut[slot] = u32x2{pdfS[s[j]] | (s[j] << 24), slot - cs[j]};
    }
  }
}

// entry i of an offsets list
__device__ __forceinline__ int64_t offsetAt(const void* offsets, uint32_t is64, uint32_t i) {
  return is64 ? ((gp<const int64_t>)G(offsets))[i] : int64_t(((gp<const int32_t>)G(offsets))[i]);
}

}  // namespace mmg

// One workgroup of dec::kThreads.  head, status and entries lie in the call's
// scratch (planMatmulGrouped, decode_plan.h): head[kHeadEntries] entries
// {expert, first row, rows <= 64, 0} in ascending (expert, row) order,
// head[kHeadBadOffsets] 1 iff offsets[0] < 0, some offsets[e] > offsets[e + 1]
// or offsets[E] > T (then every status is 0 and there is no entry), status[e]
// 1 iff archive e is 4 B-aligned and its headers pass mm::openTable.
// outSuccess (optional) takes a copy of the statuses.
template <int FT>
__global__ __launch_bounds__(dec::kThreads) void k_matmulGroupPlan(const uint64_t* __restrict__ archives, uint32_t E,
                                                                  const void* __restrict__ offsets, uint32_t offIs64,
                                                                  uint32_t T, uint32_t numRows, uint32_t rowWords,
                                                                  int pb, uint32_t* head, uint8_t* status, u32x4* entries,
                                                                  uint8_t* outSuccess) {
  __shared__ uint32_t red[dec::kThreads / 64];
  const uint32_t tid = threadIdx.x;
  int bad = 0;
  for (uint32_t e = tid; e < E; e += dec::kThreads) {
    const int64_t lo = mmg::offsetAt(offsets, offIs64, e), up = mmg::offsetAt(offsets, offIs64, e + 1);
    bad |= (lo > up || (e == 0 && lo < 0) || (e == E - 1 && up > int64_t(T))) ? 1 : 0;
  }
  bad = __syncthreads_or(bad);

  uint32_t base = 0;  // entries of the rounds before
  for (uint32_t e0 = 0; e0 < E; e0 += dec::kThreads) {
    const uint32_t e = e0 + tid;
    bool ok = false;
    uint32_t first = 0, rows = 0;
    if (e < E && !bad) {
      const uint64_t addr = ((gp<const uint64_t>)G(archives))[e];
      if (addr != 0 && (addr & 3) == 0) {
        gp<const uint8_t> arch[1];
        uint32_t n;
        ok = mm::openTable<FT>(G(reinterpret_cast<const uint8_t*>(addr)), pb, numRows, rowWords, n, arch);
      }
      const int64_t lo = mmg::offsetAt(offsets, offIs64, e);
      first = uint32_t(lo);
      rows = uint32_t(mmg::offsetAt(offsets, offIs64, e + 1) - lo);
    }
    if (e < E) {
      G(status)[e] = ok ? 1 : 0;
      if (outSuccess) G(outSuccess)[e] = ok ? 1 : 0;
    }
    const uint32_t chunks = ok ? divUp(rows, kMatmulMaxRows) : 0u;
    uint32_t sum;
    const uint32_t at = base + blockExclusiveScan<dec::kThreads>(chunks, red, &sum);
    base += sum;
    for (uint32_t c = 0; c < chunks; ++c) {
      const uint32_t r0 = c * kMatmulMaxRows;
      G(entries)[at + c] = u32x4{e, first + r0, min(kMatmulMaxRows, rows - r0), 0u};
    }
  }
  if (tid == 0) {
    G(head)[mmg::kHeadEntries] = base;
    G(head)[mmg::kHeadBadOffsets] = uint32_t(bad);
  }
}

// grid planMatmulGrouped().gridX (decode_plan.h) or fewer, dynamic LDS
// mmg::ldsBytes(DecCfg<FT>::ldsBytes(pb)).  period, groups: planMatmulTile's
// for one table.  x, xRowStrideBytes and rowWords as k_matmulTile's.
template <int FT>
__global__ __launch_bounds__(dec::kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_matmulTileGrouped(
    const uint64_t* __restrict__ archives, uint32_t numRows, uint32_t rowWords, const uint8_t* __restrict__ x,
    uint64_t xRowStrideBytes, const uint32_t* __restrict__ head, const u32x4* __restrict__ entries,
    float* __restrict__ part, uint32_t pieces, uint32_t period, uint32_t groups, int pb) {
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
  // what only a crossing needs, kept in LDS and not in scalar registers over the segment loop
  lp<uint64_t> ctx = (lp<uint64_t>)(tiles + 2 * mmt::kTileBytes);

  // this workgroup's part of the task line; one with none leaves before any barrier
  const uint32_t nEntries = readfirst(G(head)[mmg::kHeadEntries]);
  const uint64_t line = uint64_t(nEntries) * groups;
  const uint32_t taskLo = uint32_t(blockIdx.x * line / gridDim.x);
  const uint32_t taskHi = uint32_t((uint64_t(blockIdx.x) + 1) * line / gridDim.x);
  if (taskLo >= taskHi) return;

  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    ctx[mmg::kCtxArchives] = reinterpret_cast<uintptr_t>(archives);
    ctx[mmg::kCtxEntries] = reinterpret_cast<uintptr_t>(entries);
    ctx[mmg::kCtxX] = reinterpret_cast<uintptr_t>(x);
    ctx[mmg::kCtxXStride] = xRowStrideBytes;
    ctx[mmg::kCtxPart] = reinterpret_cast<uintptr_t>(part);
  }
  const uint32_t total = numRows * rowWords;          // a table's words: a multiple of 256
  const uint32_t tBlocks = divUp(total, kBlockSize);  // the blocks that hold words of a table
  const uint32_t run = kGatherTasksPerWG * period;    // blocks of `period` task groups

  const uint32_t w = readfirst(tid >> 6), lane = tid & 63, l = lane & 31;
  const uint32_t hv = upperHalfMask(lane);
  const bool hi = lane >= 32;
  const uint32_t mask = (1u << pb) - 1;
  lp<const u32x2> lut[S];
  lut[0] = (lp<const u32x2>)L;

  const uint32_t off = dec::kChunk * l;  // this lane's chunk in a segment
  // the multiply: this lane's place (i, kg) in A, B and D
  const uint32_t li = lane & 15, kg = lane >> 4;
  // where this lane's chunk goes in a tile, and where its B operand comes from
  const uint32_t tileTo = (2 * w + (hi ? 1u : 0u)) * mmt::kTileRowBytes + 16 * l;
  const uint32_t tileFrom = (li & 7) * mmt::kTileRowBytes + 16 * kg;
  mmt::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  uint32_t buf = 0;  // the tile that the next segment fills

  // the entry in hand: its archive, its rows of x and this wave's m-tile
  uint32_t cur = ~0u;
  bool open = false;
  gp<const uint8_t> arch[S];
  gp<const uint8_t> raw = nullptr;
  uint32_t n = 0;
  bool vecIn = false, mine = false;
  gp<const uint8_t> xLane = nullptr;  // this lane's row of A
  gp<float> partLane = nullptr;       // the partials of row 16 w + 4 kg of the entry, this lane's first of D
  int32_t mLeft = 0;                  // the entry's rows from that one on

  // Everything that decides a barrier below is uniform over the workgroup.
  for (uint32_t task = taskLo; task < taskHi; ++task) {
    const uint32_t ent = task / groups, grp = task - ent * groups;
    if (ent != cur) {
      // Crossing into an entry.  No wave may still read the old table, segment
      // buffers or tile when the new table is built.
      // (The first crossing's barrier is the one after ctx was written.)
      __syncthreads();
      cur = ent;
      const u32x4 en = ((gp<const u32x4>)mmg::uniform64(ctx[mmg::kCtxEntries]))[ent];
      const uint32_t e = readfirst(en.x), row0 = readfirst(en.y), mRows = readfirst(en.z);
      const uint64_t addr = mmg::uniform64(((gp<const uint64_t>)mmg::uniform64(ctx[mmg::kCtxArchives]))[e]);
      gp<const uint8_t> base = G(reinterpret_cast<const uint8_t*>(addr));
      open = mm::openTable<FT>(base, pb, numRows, rowWords, n, arch);  // as k_matmulGroupPlan found it
      if (open) {
        vecIn = (addr & 15) == 0;
        raw = rawSectionOf(base);
        mmg::rebuildLut64((gp<const uint16_t>)(arch[0] + kANSHeaderBytes), (lp<u32x2>)L, pb, (uint32_t*)segAll);
        __syncthreads();
        mine = 16 * w < mRows;  // wave-uniform
        // (a lane past the entry's rows reads its last row: D rows that are stored nowhere)
        xLane = (gp<const uint8_t>)ctx[mmg::kCtxX] +
                uint64_t(row0 + min(16 * w + li, mRows - 1)) * ctx[mmg::kCtxXStride] + 16 * kg;
        partLane = (gp<float>)ctx[mmg::kCtxPart] + uint64_t(row0 + 16 * w + 4 * kg) * pieces;
        mLeft = int32_t(mRows) - int32_t(16 * w + 4 * kg);
      }
    }
    if (!open) {  // the entry's other task groups
      task = min(taskHi, (ent + 1) * groups) - 1;
      continue;
    }
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
    // this lane's half: the block's top segment inside the table; the segments
    // above it, and all of an idle half's, are zeros in the tile
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
    const AnsSections arc(arch[0], divUp(n, kBlockSize));
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
              if (v < mLeft) partLane[uint32_t(v) * pieces + bkS + rowS] = acc[v];
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

// grid divUp(T * numRows, 256) x 256 threads, one per (t, r).  Nothing is
// stored when the plan found bad offsets, for a row below offsets[0] or at or
// past offsets[E] and for a row whose expert failed; else row r's pieces part[t * pieces + r + b]
// are added as k_matmulFinish adds them and rounded once.
template <int FT, bool OUT32>
__global__ __launch_bounds__(dec::kThreads) void k_matmulFinishGrouped(
    const void* __restrict__ offsets, uint32_t offIs64, uint32_t E, uint32_t T, uint32_t numRows, uint32_t rowWords,
    const uint32_t* __restrict__ head, const uint8_t* __restrict__ status, const float* __restrict__ part,
    uint32_t pieces, uint8_t* out, uint64_t outRowStride) {
  static_assert(FT == 1 || FT == 2, "fp16 and bf16");
  using J = Join<FT, 0>;
  using OutT = std::conditional_t<OUT32, uint32_t, uint16_t>;
  if (G(head)[mmg::kHeadBadOffsets] != 0) return;
  const uint32_t i = blockIdx.x * dec::kThreads + threadIdx.x;
  if (i >= T * numRows) return;
  const uint32_t t = i / numRows, r = i - t * numRows;
  // no expert owns a row below offsets[0] or at and past offsets[E]
  if (int64_t(t) < mmg::offsetAt(offsets, offIs64, 0) || int64_t(t) >= mmg::offsetAt(offsets, offIs64, E)) return;
  // the expert that owns t: offsets[e] <= t < offsets[e + 1] (the first
  // boundary above t is in 1 .. E)
  uint32_t lo = 1, up = E;
  while (lo < up) {
    const uint32_t mid = (lo + up) / 2;
    if (mmg::offsetAt(offsets, offIs64, mid) > int64_t(t)) up = mid;
    else lo = mid + 1;
  }
  if (G(status)[lo - 1] == 0) return;
  const uint32_t s0 = r * rowWords;
  const uint32_t bFirst = s0 / kBlockSize, bLast = (s0 + rowWords - 1) / kBlockSize;
  gp<const float> p = G(part) + (t * pieces + r);
  float sum = p[bFirst];
  for (uint32_t b = bFirst + 1; b <= bLast; ++b) sum += p[b];
  gp<OutT> o = (gp<OutT>)G(out) + (uint64_t(t) * outRowStride + r);
  if constexpr (OUT32) *o = __builtin_bit_cast(uint32_t, sum);
  else if constexpr (FT == 1) *o = __builtin_bit_cast(uint16_t, _Float16(sum));
  else *o = uint16_t(J::bf16Of(sum));
}

}  // namespace dietgpu
