// Sparse float codec: nonzero bitmap + per-element exclusive scan +
// compaction, wrapped around the dense float codec.
//
// Reference: float/GpuSparseFloatCompress.{cu,cuh},
// float/GpuSparseFloatDecompress.{cu,cuh}.  The reference scans with one
// thrust::exclusive_scan per batch element on the legacy default stream
// between two cudaDeviceSynchronize calls (GpuSparseFloatCompress.cuh:360-369);
// here both directions are reduce-then-scan over 4096-word tiles, fully
// stream-ordered (no host or device-wide sync): compression reads the input
// ONCE (k_sparseCount: bitmap, tile counts, nonzeros compacted within the
// tile into a staging area; k_sparseGather: each tile sums its element's
// earlier tile counts and moves its staged nonzeros to their list
// positions); decompression counts the bitmap per 1024-word chunk and scans
// the counts within each workgroup of 256 chunks (k_sparseChunks), then
// expands one chunk per wave, adding the element's earlier workgroups' totals
// (k_sparseExpand).  (A decoupled look-back across
// the tiles of one element measured slower: with thousands of tiles its
// chain dominates.)  A word range of an element is read without the rest
// (floatDecompressSparseRange, an extension): the same chunk counts give the
// rank of the range's ends, i.e. its slice of the nonzero list; the dense
// range decode reads that slice and k_sparseExpandRange expands it.  An
// element is added to an accumulator without a temporary
// (floatDecompressSparseAccumulate, an extension): k_sparseExpand<FT, ACC>
// adds the nonzero words where the full decode stores them and touches no
// other accumulator word.  K archives are summed without any accumulator in
// memory (floatReduceSparseArchives, an extension): k_sparseReduce<FT, NS>
// expands the same chunk of NS archives side by side and keeps the fp32
// running sum in registers, a clear bit a select and never an add of +0.0.
//
// Wire format: 16 B header {u32 N, 12 B zero}, bitmap
// ceil(N/8) bytes (bit 7 of byte k <-> element 8k) padded to 16, then a dense
// float archive of the compacted list.  The compacted list reproduces the
// reference's n-2 quirk (fill_comp_input :162-184): when x[N-2] == 0 one extra
// slot (written as 0 here, uninitialised in the reference) precedes x[N-1].
#include <algorithm>
#include <vector>

#include "codec_internal.h"
#include "common.h"
#include "dietgpu/GpuFloatCodec.h"
#include "decode.h"
#include "encode.h"
#include "profile.h"
#include "sparse_plan.h"
#include "sync_arena.h"

namespace dietgpu {

namespace {

constexpr uint32_t kTileWords = 4096;   // 4 waves x 16 steps x 64 lanes
// Decompression works on 1024-word chunks (16 bitmap words, one wave).
constexpr uint32_t kChunkWords = 1024;
constexpr uint32_t kChunkRows = kChunkWords / 64;  // 64-word rows, one bitmap word each
static_assert(kTileWords == splan::kTileWords && kChunkWords == splan::kChunkWords &&
                  kThreads == splan::kThreads && kWaves == splan::kWaves && kBlockSize == cplan::kBlockWords,
              "sparse_plan.h restates the kernels' constants");

template <int FT>
using WordOf = typename FloatTraits<FT>::WordT;

// flags of words [base, base + 64) as a lane mask <-> packed bitmap u64
__device__ __forceinline__ uint64_t maskToBitmap(uint64_t m) {
  return __builtin_bswap64(__builtin_bitreverse64(m));
}

template <int FT>
__device__ __forceinline__ bool isNonzero(WordOf<FT> w) {
  return w != 0;  // bitwise: -0.0 is "nonzero" (generate_bitmap :56)
}

// Load tile `tile` of an element (words past n read as 0) into LDS: 16 B
// vectors when the element is 16 B aligned (coalesced), else words.
template <typename W, bool kVec>
__device__ __forceinline__ void loadTile(gp<const W> x, uint32_t t0, uint32_t tileN, W* buf) {
  const uint32_t tid = threadIdx.x;
  if (kVec) {
    constexpr uint32_t kWPV = 16 / sizeof(W);
    constexpr uint32_t kVecs = kTileWords * sizeof(W) / 16 / kThreads;
#pragma unroll
    for (uint32_t v = 0; v < kVecs; ++v) {
      const uint32_t wi = (v * kThreads + tid) * kWPV;  // first word of the vector
      uint4 val = make_uint4(0, 0, 0, 0);
      if (wi + kWPV <= tileN) {
        val = ld16nt((gp<const uint4>)(x + t0 + wi));  // read once: stream it
      } else if (wi < tileN) {
        W tmp[kWPV];
#pragma unroll
        for (uint32_t k = 0; k < kWPV; ++k) tmp[k] = wi + k < tileN ? x[t0 + wi + k] : W(0);
        __builtin_memcpy(&val, tmp, 16);
      }
      *(lp<u32x4>)&buf[wi] = u32x4{val.x, val.y, val.z, val.w};
    }
  } else {
#pragma unroll 4
    for (uint32_t i = tid; i < kTileWords; i += kThreads) buf[i] = i < tileN ? x[t0 + i] : W(0);
  }
}

// One tile of k_sparseCount (t0 < n).
template <int FT, bool kVec, bool kHist, typename W, typename HS>
__device__ __forceinline__ void sparseCountTile(const BatchDesc& in, gp<uint8_t> o, uint32_t b, uint32_t n,
                                                uint32_t tile, uint32_t numInBatch, uint32_t tilesPerElem,
                                                uint32_t* __restrict__ tileCounts, W* __restrict__ staging,
                                                uint32_t* __restrict__ histRows, uint32_t* __restrict__ zeroNext,
                                                uint32_t nRows, W* buf, HS& hs, uint32_t* waveCnt) {
  constexpr int kSegs = FloatTraits<FT>::kSegs;
  constexpr uint32_t kSteps = kTileWords / kWaves / 64;
  constexpr uint32_t kCols = 4;  // LDS counter columns per bin (lane & 3)
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t t0 = tile * kTileWords;
  if constexpr (kHist) {
    for (int sg = 0; sg < kSegs; ++sg)
      for (uint32_t i = tid; i < kNumSymbols * kCols / 4; i += kThreads)
        *(lp<u32x4>)&hs[sg][4 * i] = u32x4{0, 0, 0, 0};
  }
  gp<const W> x = (gp<const W>)in.start(b);
  // bitwise: -0.0 is "nonzero" (generate_bitmap :56); loaded with the tile
  const W xn2 = n >= 2 ? x[n - 2] : W(1);
  loadTile<W, kVec>(x, t0, min(kTileWords, n - t0), buf);
  __syncthreads();
  const uint32_t bmBytes = (n + 7) / 8, bmPad = roundUp(bmBytes, 16);
  const bool gap = xn2 == W(0);
  // (the step ballots are taken again in the compaction below: sixteen
  // 64-bit masks held across the barrier cost registers, i.e. occupancy)
  uint32_t cnt = 0;
  uint64_t bmLane = 0;  // lane j < kSteps: the bitmap word of step j
#pragma unroll
  for (uint32_t j = 0; j < kSteps; ++j) {
    const uint32_t q = w * (kTileWords / kWaves) + 64 * j;  // step's first word in the tile
    const uint64_t mj = ballot(buf[q + lane] != W(0));
    cnt += uint32_t(__popcll(mj));
    bmLane = lane == j ? maskToBitmap(mj) : bmLane;
    const uint32_t i0 = t0 + q;
    if (gap && i0 <= n - 1 && n - 1 < i0 + 64) cnt += 1;  // the extra slot
  }
  {
    // the wave's kSteps bitmap words in one store; then zero the 16-byte
    // padding after the element's last bitmap word
    const uint32_t i0 = t0 + w * (kTileWords / kWaves) + 64 * lane;
    gp<uint64_t> dst = (gp<uint64_t>)(o + kSparseHeaderBytes + i0 / 8);
    if (lane < kSteps && i0 < n) {
      dst[0] = bmLane;
      if (i0 + 64 >= n && i0 / 8 + 8 < bmPad) dst[1] = 0;
    }
  }
  if (lane == 0) waveCnt[w] = cnt;
  __syncthreads();
  uint32_t pos = 0;
  for (uint32_t k = 0; k < w; ++k) pos += waveCnt[k];
  if (tid == 0) tileCounts[uint64_t(b) * tilesPerElem + tile] = waveCnt[0] + waveCnt[1] + waveCnt[2] + waveCnt[3];
  W* st = staging + (uint64_t(b) * tilesPerElem + tile) * (kTileWords + 1);
#pragma unroll
  for (uint32_t j = 0; j < kSteps; ++j) {
    const uint32_t q = w * (kTileWords / kWaves) + 64 * j;
    const uint32_t i = t0 + q + lane;
    const W v = buf[q + lane];
    const uint64_t mj = ballot(v != W(0));
    const uint32_t dst = pos + mbcnt(mj);
    if (i + 1 == n && gap) {
      st[dst] = W(0);
      if (v != W(0)) st[dst + 1] = v;
    } else if (v != W(0)) {
      st[dst] = v;
    }
    if constexpr (kHist) {
      auto count = [&](W y) {
#pragma unroll
        for (int sg = 0; sg < kSegs; ++sg)
          atomicAdd(&hs[sg][compOf<FT>(y, sg) * kCols + (lane & (kCols - 1))], 1u);
      };
      if (i + 1 == n && gap) count(W(0));
      if (v != W(0)) count(v);
    }
    pos += uint32_t(__popcll(mj)) + ((gap && t0 + q <= n - 1 && n - 1 < t0 + q + 64) ? 1u : 0u);
  }
  if constexpr (kHist) {
    __syncthreads();
    for (int sg = 0; sg < kSegs; ++sg) {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t k = 0; k < kCols; ++k) sum += hs[sg][tid * kCols + ((k + tid) & (kCols - 1))];
      // few adds per address: the tiles of an element spread over nRows rows
      commitHistRow(histRows, zeroNext, uint64_t(sg) * numInBatch + b, tile, nRows, sum);
    }
  }
}

// s1: bitmap + tile count + tile-local compaction.  grid (tiles, batch); a
// workgroup takes one 4096-word tile of one element into LDS, then each wave
// takes 1024 consecutive words as 16 steps of 64 lanes: the ballot of nonzero
// flags is the step's 64 bitmap bits (generate_bitmap :40-71) and its
// nonzeros' ranks (v_mbcnt).  The nonzeros go, in order, to the tile's slice
// of a staging area; the n-2 quirk (fill_comp_input :162-184) is one extra
// staged slot: when x[n-2] == 0, a 0 precedes x[n-1]'s slot.  (A persistent
// grid streaming several tiles per workgroup measured slower: its live state
// halves the occupancy, and a wave's wait for its next tile's loads also
// drains its stores.)
//
// kHist: the staged words are also counted into the dense codec's symbol
// histogram(s) (the compacted list's symbols, the n-2 slot included) and
// added into row tile % nRows of [segments][nb][nRows][256] (PartialHist),
// so the dense codec skips its histogram pass over the list.  The rows are
// the stream's sync-arena row buffer (SyncLease::rows, zero on entry); the
// first nRows tiles, empty ones included, zero the same rows of the other
// buffer for the next call (`zeroNext`; commitHistRow, encode.h), so no
// zeroing launch precedes this one (1 x 15M fp32: a
// 4.7 us k_zero of 64 KB before).  (Normalising in the element's last-arriving tile instead of the
// dense codec's k_normalize launch made every tile pay a store drain and a
// counter round trip: c4 1 x 15M fp32 compress 70 -> 95 us.)
// (at most 80 SGPRs: 86-94 admit 7 workgroups per CU instead of 8,
// MI355X_MICROARCH.md, Residency)
template <int FT, bool kVec, bool kHist>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(80))) void k_sparseCount(BatchDesc in, BatchDesc outD,
                                                          uint32_t batchOffset, uint32_t numInBatch,
                                                          uint32_t tilesPerElem,
                                                          uint32_t* __restrict__ tileCounts,
                                                          WordOf<FT>* __restrict__ staging,
                                                          uint32_t* __restrict__ histRows,
                                                          uint32_t* __restrict__ zeroNext, uint32_t nRows) {
  using W = WordOf<FT>;
  constexpr int kSegs = FloatTraits<FT>::kSegs;
  constexpr uint32_t kCols = 4;  // LDS counter columns per bin (lane & 3)
  __shared__ __attribute__((aligned(16))) W buf[kTileWords];
  __shared__ __attribute__((aligned(16))) uint32_t hs[kHist ? kSegs : 1][kHist ? kNumSymbols * kCols : 4];
  __shared__ uint32_t waveCnt[kWaves];
  const uint32_t b = batchOffset + blockIdx.y;
  const uint32_t n = in.size(b);
  const uint32_t tile = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  gp<uint8_t> o = startOf(outD, b);
  if (tile == 0 && tid == 0) writeSparseHeader(o, n);
  const uint32_t t0 = tile * kTileWords;
  if (t0 >= n) {
    if (tid == 0) tileCounts[uint64_t(b) * tilesPerElem + tile] = 0;
    // (an empty element's tile 0 among them: whoever holds a rows lease zeroes
    // its rows of the other buffer, whatever the sizes)
    if constexpr (kHist) {
      for (int sg = 0; sg < kSegs; ++sg)
        commitHistRow(histRows, zeroNext, uint64_t(sg) * numInBatch + b, tile, nRows, 0);
    }
  } else {
    sparseCountTile<FT, kVec, kHist>(in, o, b, n, tile, numInBatch, tilesPerElem, tileCounts, staging, histRows,
                                     zeroNext, nRows, buf, hs, waveCnt);
  }
}

// Sum of counts[0, k) by the whole workgroup: 16 loads in flight per thread
// (4,096 counts per memory round trip; an element of 16 M words has 4,096
// tiles).  Every workgroup of an element sums its own prefix of the tile
// counts, which stay in L2 (a 15 M-word element: 14.6 KB of counts, 27 MB of
// L2 reads over its 3,662 workgroups), instead of a separate scan launch
// (each launch of this chain costs ~5 us, however little it does).
__device__ __forceinline__ uint32_t tilePrefix(gp<const uint32_t> counts, uint32_t k, uint32_t* red) {
  constexpr uint32_t kR = 16;
  uint32_t sum = 0;
  for (uint32_t base = 0; base < k; base += kR * kThreads) {
    uint32_t v[kR];
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j) {
      const uint32_t i = base + j * kThreads + threadIdx.x;
      v[j] = i < k ? counts[i] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j) sum += v[j];
  }
  return blockSum<kThreads>(sum, red);
}

// s2: staged nonzeros -> their list positions.  grid (tiles [+ 1], batch).
// The tile's list offset is the sum of the element's earlier tile counts
// (tilePrefix); the last tile also stores the list's length.  With
// na.hist set (k_sparseCount counted the list's histogram), one extra
// workgroup per element normalises it meanwhile, into the dense codec's
// encode table and pdf: the dense codec then skips its k_normalize launch
// (c4 1 x 15M fp32 compress -6 us).
template <int FT>
__global__ __launch_bounds__(kThreads) void k_sparseGather(BatchDesc in, uint32_t batchOffset,
                                                           uint32_t numInBatch, uint32_t tilesPerElem,
                                                           const uint32_t* __restrict__ tileCounts,
                                                           uint32_t* __restrict__ listLen,
                                                           const WordOf<FT>* __restrict__ staging,
                                                           BatchDesc lists, NormArgs na) {
  using W = WordOf<FT>;
  __shared__ uint32_t red[kWaves];
  const uint32_t b = batchOffset + blockIdx.y;
  const uint32_t tile = blockIdx.x;
  if (tile == tilesPerElem) {  // (grid.x = tiles + 1 only with na.hist)
    __shared__ __attribute__((aligned(16))) uint32_t keys[kNumSymbols];
    __shared__ u32x4 red4[kThreads];
    for (int sg = 0; sg < FloatTraits<FT>::kSegs; ++sg) {
      normalizeElement(na, numInBatch, b, sg, keys, red, red4);
      __syncthreads();
    }
    return;
  }
  const uint32_t n = in.size(b);
  if (tile * kTileWords >= n) {
    // an empty element has no last tile: its (empty) list length is written here
    if (n == 0 && tile == 0 && threadIdx.x == 0) listLen[b] = 0;
    return;
  }
  const uint64_t row = uint64_t(b) * tilesPerElem + tile;
  const uint32_t cnt = tileCounts[row];
  const uint32_t off = tilePrefix(G(tileCounts) + uint64_t(b) * tilesPerElem, tile, red);
  if ((tile + 1) * kTileWords >= n && threadIdx.x == 0) listLen[b] = off + cnt;
  const W* st = staging + row * (kTileWords + 1);
  gp<W> list = (gp<W>)lists.start(b);
  // every staged word of the tile in flight at once, then the stores (a
  // load -> store loop took one memory round trip per 256 words: 5 x 15M
  // fp32 at 50 % zeros, 2,048 nonzeros a tile, 92 us for this kernel)
  constexpr uint32_t kPer = (kTileWords + 1 + kThreads - 1) / kThreads;
  W v[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t i = threadIdx.x + k * kThreads;
    if (i < cnt) v[k] = st[i];
  }
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t i = threadIdx.x + k * kThreads;
    if (i < cnt) list[off + i] = v[k];
  }
}

// The set bits of chunk c of the bitmap bm of an N-word element: the popcount
// of its 128 bitmap bytes, bits at or past N cut (the bitmap's padding is the
// reference's uninitialised bytes); 0 for a chunk at or past N.  Words are
// counted from the chunk's start, which cannot wrap (c < 2^22 + 256).  Only
// the bitmap words that start below N are read, so the reads stay inside the
// padded bitmap.
__device__ __forceinline__ uint32_t chunkPopcount(gp<const uint8_t> bm, uint32_t c, uint32_t n) {
  if (uint64_t(c) * kChunkWords >= n) return 0;
  const uint32_t left = n - c * kChunkWords;  // the element's words from the chunk's start on
  gp<const uint64_t> bw = (gp<const uint64_t>)bm + uint64_t(c) * kChunkRows;
  uint64_t v[kChunkRows];
#pragma unroll
  for (uint32_t k = 0; k < kChunkRows; ++k) v[k] = left > 64 * k ? bw[k] : 0ull;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunkRows; ++k) {
    uint64_t m = v[k];
    const uint32_t rem = left - 64 * k;  // (used only when the word was loaded)
    if (left > 64 * k && rem < 64) m = maskToBitmap(m) & ((1ull << rem) - 1);  // element order, tail cut
    cnt += uint32_t(__popcll(m));
  }
  return cnt;
}

// One thread per chunk (d1 / r1): thread t counts chunk c (0 for c >= nChunks)
// of the N-word element with bitmap bm, the workgroup scans its 256 counts,
// and the chunk's exclusive prefix goes to *pre (this thread's chunkPre entry,
// not written for c >= nChunks), the workgroup's total to *tot (its blockTot
// entry).
__device__ __forceinline__ void countAndScanChunks(gp<const uint8_t> bm, uint32_t c, uint32_t nChunks, uint32_t n,
                                                   uint32_t* red, gp<uint32_t> pre, gp<uint32_t> tot) {
  const uint32_t cnt = c < nChunks ? chunkPopcount(bm, c, n) : 0u;
  uint32_t total = 0;
  const uint32_t excl = blockExclusiveScan<kThreads>(cnt, red, &total);
  if (c < nChunks) *pre = excl;
  if (threadIdx.x == 0) *tot = total;
}

// Lane k < 16: bitmap word k of chunk c of the bitmap bm, in element order
// (bit j <-> word 1024 c + 64 k + j of the element), the bits of words at or
// past `limit` (counted from the chunk's start) cut; 0 in the other lanes and
// for a bitmap word wholly at or past the limit, which is not read.
__device__ __forceinline__ uint64_t chunkBitmapWord(gp<const uint8_t> bm, uint32_t c, uint32_t limit,
                                                    uint32_t lane) {
  uint64_t m = 0;
  if (lane < kChunkRows && 64 * lane < limit) {
    m = maskToBitmap(*(gp<const uint64_t>)(bm + uint64_t(c) * (kChunkWords / 8) + 8 * lane));
    const uint32_t rem = limit - 64 * lane;
    if (rem < 64) m &= (1ull << rem) - 1;
  }
  return m;
}

// gap: x[N-1] is read from idx[N-2] + 1 (fill_in_nonzeros :139-144), one list
// slot further than its rank, when bit N-2 of the bitmap is clear.
__device__ __forceinline__ bool gapBit(gp<const uint8_t> bm, uint32_t n) {
  return n >= 2 && ((bm[(n - 2) / 8] >> (7 - (n - 2) % 8)) & 1) == 0;
}

// This lane's share of the totals of the counting workgroups before g (tot:
// the archive's blockTot entries): one load per lane up to 64 workgroups,
// i.e. 16 M words.  waveSum of the shares is the list offset of chunk 256 g.
__device__ __forceinline__ uint32_t totalsShare(gp<const uint32_t> tot, uint32_t g, uint32_t lane) {
  uint32_t part = 0;
  for (uint32_t k0 = 0; k0 < g; k0 += 64) part += k0 + lane < g ? tot[k0 + lane] : 0u;
  return part;
}

// Chunk c's list offset (wave-uniform c): its count prefix within its counting
// workgroup (pre: the archive's chunkPre entries) plus the totals of the
// earlier workgroups.
__device__ __forceinline__ uint32_t chunkListOffset(gp<const uint32_t> pre, gp<const uint32_t> tot, uint32_t c,
                                                    uint32_t lane) {
  return readfirst(pre[c]) + waveSum(totalsShare(tot, c / kThreads, lane));
}

// A chunk's 16 rows of 64 words, one wave: mv holds the rows' bitmap words in
// lanes 0-15, base is the chunk's list offset.  For each row the mask comes
// to SGPRs (readlane), each lane's list index is the running offset + v_mbcnt
// of the mask (+ 1 for word N-1 behind a gap), and all 16 rows' list gathers
// are issued back to back (their addresses depend only on the bitmap) for the
// caller's 16 row stores.  v[j] = word i0 + 64 j + lane of the element, 0
// where its bit is clear or wanted(i) is false (that word is not read).
// row(j, i, set) follows row j's gather at once (set: the word's bitmap bit),
// so what it loads is in flight with the 16 gathers (the accumulate forms'
// accumulator words).
template <class W, class Wanted, class Row>
__device__ __forceinline__ void expandRows(uint64_t mv, uint32_t base, uint32_t i0, uint32_t n, bool gap,
                                           gp<const W> list, uint32_t lane, Wanted wanted, W (&v)[kChunkRows],
                                           Row row) {
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) {
    const uint64_t m = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(mv >> 32)), int(j)))) << 32) |
                       uint32_t(__builtin_amdgcn_readlane(int(uint32_t(mv)), int(j)));
    const uint32_t i = i0 + 64 * j + lane;
    uint32_t src = base + mbcnt(m);
    if (gap && i + 1 == n) src += 1;
    v[j] = wanted(i) && ((m >> lane) & 1) ? list[src] : W(0);
    row(j, i, ((m >> lane) & 1) != 0);
    base += uint32_t(__popcll(m));
  }
}

template <class W, class Wanted>
__device__ __forceinline__ void expandRows(uint64_t mv, uint32_t base, uint32_t i0, uint32_t n, bool gap,
                                           gp<const W> list, uint32_t lane, Wanted wanted, W (&v)[kChunkRows]) {
  expandRows(mv, base, i0, n, gap, list, lane, wanted, v, [](uint32_t, uint32_t, bool) {});
}

// x is in its register from here on: a loaded value has arrived, and nothing
// computed from it moves above this point (an empty asm the compiler cannot
// see through; no instruction is emitted).
template <class T>
__device__ __forceinline__ void landed(T& x) {
  if constexpr (sizeof(T) == 8) {
    asm volatile("" : "+v"(x));
  } else {
    uint32_t t = x;
    asm volatile("" : "+v"(t));
    x = T(t);
  }
}

// d1: one thread per chunk: the popcount of its 128 bitmap bytes (bits past
// N masked: the bitmap's padding is the reference's uninitialised bytes),
// then the workgroup's exclusive scan of its 256 chunk counts: chunkPre[c] =
// the count of the earlier chunks of c's workgroup, blockTot[g] = workgroup
// g's total; (chunk 0) the dense archive's address and N.  grid
// (ceil(chunks / 256), batch).  The expansion adds the earlier workgroups'
// totals itself (k_sparseExpand), so no scan launch or cross-workgroup
// hand-off follows (a separate one-workgroup-per-element scan launch: 1 x 15M
// fp32 decompress 5.8 us more).
__global__ __launch_bounds__(kThreads) void k_sparseChunks(BatchDesc in, uint32_t batchOffset,
                                                           uint32_t chunksPerElem, uint32_t blocksPerElem,
                                                           uint64_t* __restrict__ densePtrs,
                                                           uint32_t* __restrict__ sizes,
                                                           uint32_t* __restrict__ chunkPre,
                                                           uint32_t* __restrict__ blockTot) {
  __shared__ uint32_t red[kWaves];
  const uint32_t b = batchOffset + blockIdx.y;
  gp<const uint8_t> a = (gp<const uint8_t>)in.start(b);
  const uint32_t n = ((gp<const uint32_t>)a)[kSparseSize];
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c == 0) {
    densePtrs[b] = reinterpret_cast<uint64_t>(in.start(b) + sparsePrefixBytes(n));
    sizes[b] = n;
  }
  countAndScanChunks(a + kSparseHeaderBytes, c, chunksPerElem, n, red, G(chunkPre) + uint64_t(b) * chunksPerElem + c,
                     G(blockTot) + uint64_t(b) * blocksPerElem + blockIdx.x);
}

// d3: expand the decoded nonzero list into the output (fill_in_nonzeros
// :95-144).  One wave per 1024-word chunk (grid (ceil(chunks / 4), batch)),
// no LDS and no barrier: lanes 0-15 load the chunk's 16 bitmap words
// beside its list offset (the scanned chunk count, loaded in the bitmap's
// round trip), then expandRows and the 16 row stores.  (The
// tile-per-workgroup kernel it replaces summed every earlier tile's count per
// tile and staged through LDS: 5 x 15M fp32 at 50 % zeros 176 us, fp64
// 430 us.)
//
// ACC (Join<FT, ACC>'s, decode.h): 0 stores the expanded
// words; 1 / 2 add them to the accumulators `out`, acc[i] = sumOne(acc[i],
// x[i]) for every i < n whose bitmap bit is set.  A word whose bit is clear
// is +0.0 and its accumulator word is neither read nor written (it keeps its
// bits where IEEE a + (+0.0) would turn -0.0 into +0.0 or quiet a NaN).  The
// 16 accumulator loads, masked like the gathers, are issued between them
// (expandRows' row hook), so all 32 are in flight before the first add; the
// stores are masked by the bit and plain (the next peer's call reads the
// accumulator again).
template <int FT, int ACC = 0>
__global__ __launch_bounds__(kThreads) void k_sparseExpand(BatchDesc in, BatchDesc out, uint32_t batchOffset,
                                                           uint32_t chunksPerElem, uint32_t blocksPerElem,
                                                           const uint32_t* __restrict__ sizes,
                                                           const uint32_t* __restrict__ chunkPre,
                                                           const uint32_t* __restrict__ blockTot, BatchDesc lists,
                                                           const uint8_t* __restrict__ denseOk,
                                                           uint8_t* __restrict__ outSuccess,
                                                           uint32_t* __restrict__ outSize) {
  using W = WordOf<FT>;
  const uint32_t b = batchOffset + blockIdx.y;
  const uint32_t n = sizes[b];
  const bool ok = denseOk[b] != 0 && out.size(b) >= n;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (outSuccess) outSuccess[b] = ok ? 1 : 0;
    if (outSize) outSize[b] = n;  // fill_in_nonzeros :107-109
  }
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t c = blockIdx.x * kWaves + w;
  const uint32_t i0 = c * kChunkWords;
  if (!ok || c >= chunksPerElem || i0 >= n) return;
  gp<const uint8_t> bm = (gp<const uint8_t>)in.start(b) + kSparseHeaderBytes;
  const uint64_t mv = chunkBitmapWord(bm, c, n - i0, lane);
  const uint32_t base = chunkListOffset(G(chunkPre) + uint64_t(b) * chunksPerElem,
                                        G(blockTot) + uint64_t(b) * blocksPerElem, c, lane);
  // only the chunk holding word n-1 looks
  const bool gap = n - 1 - i0 < kChunkWords && gapBit(bm, n);
  W v[kChunkRows];
  if constexpr (ACC == 0) {
    expandRows(mv, base, i0, n, gap, (gp<const W>)lists.start(b), lane, [](uint32_t) { return true; }, v);
    gp<W> y = (gp<W>)out.start(b);
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j) {
      const uint32_t i = i0 + 64 * j + lane;
      // streaming: nothing here re-reads the output
      if (i < n) __builtin_nontemporal_store(v[j], y + i);
    }
  } else {
    using J = Join<FT, ACC>;  // (its static_assert: ACC 2 for fp16 / bf16 only)
    using A = typename J::AccT;
    gp<A> y = (gp<A>)out.start(b);
    A a[kChunkRows];
    uint32_t taken16 = 0;  // bit j: this lane's word of row j has its bitmap bit set
    // (mv holds no bit at or past n; the loads and stores test i < n all the same)
    expandRows(mv, base, i0, n, gap, (gp<const W>)lists.start(b), lane, [&](uint32_t i) { return i < n; }, v,
               [&](uint32_t j, uint32_t i, bool set) __attribute__((always_inline)) {
                 const bool taken = set && i < n;
                 a[j] = taken ? y[i] : A(0);
                 taken16 |= (taken ? 1u : 0u) << j;
               });
    // One wait for the 32 loads here, where the wave has converged.  Left to
    // the masked store blocks below, the compiler widened a bf16 word inside
    // its masked load block (a wait per row), and every store block waited
    // for vmcnt(0), i.e. for the previous row's store as well.
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j) {
      landed(v[j]);
      landed(a[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j)
      if ((taken16 >> j) & 1) y[i0 + 64 * j + lane] = J::sumOne(a[j], v[j]);
  }
}

// What a pass of the fused sparse reduce reads and writes beside its archives.
struct SparseRedArgs {
  uint32_t batchOffset;  // first member of this grid slice
  uint32_t nb;           // members: source s of member b is row s * nb + b of the pass
  uint32_t chunksPerElem, blocksPerElem;
  uint32_t initKind;  // 0: none (the sum starts as float(x_1)), 1: the archives' 16-bit type, 2: fp32
  uint32_t outF32;    // out words are fp32 (always for fp32 archives and for the partial)
  uint32_t first;     // the call's first pass: no earlier verdict, n is this pass's first source's
  uint32_t last;      // the call's last pass writes outSuccess / outSize, the others the verdict
};

// Fused sparse reduce: one pass over sources s < NS of every
// member on top of `init`,
//   a = float(init[i])  (initKind 0: the decoded word x_0[i], +0.0 under a clear bit)
//   a = bit i of source s set ? a + float(x_s[i]) : a,  sources in order
//   out[i] = round(a),
// the running sum in 16 fp32 registers per lane.  One wave per 1024-word chunk
// like k_sparseExpand, no LDS and no barrier: per source lanes 0-15 load the
// chunk's 16 bitmap words beside its list offset, then the NS x 16 list
// gathers (expandRows) and the 16 init loads (source 0's row hook) are issued
// back to back before one counted wait (landed), the sums, and 16 row stores.
// A clear bit is a select of `a`, never an add of +0.0: an init of -0.0 or a
// signalling NaN under clear bits keeps its bits.  PART: `out` is the fp32
// partial that the next pass reads (plain stores); otherwise the caller's out
// (streaming stores; a compile-time choice, as for Join::vec).
//
// A member goes on iff every source so far had a valid dense part
// (denseOk) and the same n as the call's first source, and out.size(b) >= n:
// `verdictIn` carries that from the earlier passes, `verdictOut` (another
// array) to the next one, firstN the first source's n.  A failing member
// returns before any list, bitmap, init or out word is touched; for the others
// every list index lies below the row's popcount + 1 <= n + 1 words.
template <int FT, int NS, bool PART>
__global__ __launch_bounds__(kThreads) void k_sparseReduce(BatchDesc in, BatchDesc init, BatchDesc out,
                                                           SparseRedArgs a, const uint32_t* __restrict__ sizes,
                                                           const uint32_t* __restrict__ chunkPre,
                                                           const uint32_t* __restrict__ blockTot, BatchDesc lists,
                                                           const uint8_t* __restrict__ denseOk,
                                                           const uint8_t* __restrict__ verdictIn,
                                                           uint8_t* __restrict__ verdictOut, uint32_t* firstN,
                                                           uint8_t* __restrict__ outSuccess,
                                                           uint32_t* __restrict__ outSize) {
  static_assert(FT >= 1 && FT <= 3 && NS >= 1 && NS <= int(kSparseReduceMaxNS), "fp16, bf16 and fp32; 1 .. 4 sources");
  using W = WordOf<FT>;
  using J = Join<FT>;
  const uint32_t b = a.batchOffset + blockIdx.y;
  const uint32_t n = readfirst(a.first ? sizes[b] : G(firstN)[b]);
  bool good = a.first || verdictIn[b] != 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) good = good && denseOk[s * a.nb + b] != 0 && sizes[s * a.nb + b] == n;
  const bool ok = good && out.size(b) >= n;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (a.last) {
      if (outSuccess) outSuccess[b] = ok ? 1 : 0;
      if (outSize) outSize[b] = n;  // the first source's, as the sparse decode reports it
    } else {
      verdictOut[b] = good ? 1 : 0;
      if (a.first) G(firstN)[b] = n;
    }
  }
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t c = blockIdx.x * kWaves + w;
  const uint32_t i0 = c * kChunkWords;
  if (!ok || c >= a.chunksPerElem || i0 >= n) return;

  uint64_t mv[NS];
  uint32_t base[NS];
  bool gap[NS];
  gp<const W> list[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const uint32_t row = s * a.nb + b;
    gp<const uint8_t> bm = (gp<const uint8_t>)in.start(row) + kSparseHeaderBytes;
    mv[s] = chunkBitmapWord(bm, c, n - i0, lane);
    base[s] = chunkListOffset(G(chunkPre) + uint64_t(row) * a.chunksPerElem,
                              G(blockTot) + uint64_t(row) * a.blocksPerElem, c, lane);
    // only the chunk holding word n-1 looks; per source
    gap[s] = n - 1 - i0 < kChunkWords && gapBit(bm, n);
    list[s] = (gp<const W>)lists.start(row);
  }

  const uint32_t initKind = a.initKind;
  gp<const uint8_t> initB = initKind ? (gp<const uint8_t>)init.start(b) : nullptr;
  W v[NS][kChunkRows];
  uint32_t d[kChunkRows];  // the init words' bits
  uint32_t taken[NS];      // bit j: this lane's word of row j has its bitmap bit set in source s
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) d[j] = 0;
  // (mv holds no bit at or past n, so every gather of a set bit is wanted)
  auto inside = [](uint32_t) { return true; };
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    taken[s] = 0;
    auto mark = [&](uint32_t j, bool set) __attribute__((always_inline)) {
      taken[s] |= (set ? 1u : 0u) << j;
    };
    // (the init loads test i < n: the last chunk's rows may end early)
    if (s == 0 && initKind == 2) {
      expandRows(mv[s], base[s], i0, n, gap[s], list[s], lane, inside, v[s],
                 [&](uint32_t j, uint32_t i, bool set) __attribute__((always_inline)) {
                   d[j] = i < n ? ((gp<const uint32_t>)initB)[i] : 0u;
                   mark(j, set);
                 });
    } else if (FT != 3 && s == 0 && initKind == 1) {
      expandRows(mv[s], base[s], i0, n, gap[s], list[s], lane, inside, v[s],
                 [&](uint32_t j, uint32_t i, bool set) __attribute__((always_inline)) {
                   d[j] = i < n ? uint32_t(((gp<const uint16_t>)initB)[i]) : 0u;
                   mark(j, set);
                 });
    } else {
      expandRows(mv[s], base[s], i0, n, gap[s], list[s], lane, inside, v[s],
                 [&](uint32_t j, uint32_t, bool set) __attribute__((always_inline)) { mark(j, set); });
    }
  }
  // one wait for the NS x 16 gathers and the 16 init loads, where the wave has
  // converged (k_sparseExpand's accumulate form, DESIGN.md 5.2f "One wait")
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) {
#pragma unroll
    for (int s = 0; s < NS; ++s) landed(v[s][j]);
    landed(d[j]);
  }

  auto asFloat = [](W x) __attribute__((always_inline)) {
    if constexpr (FT == 3) return __builtin_bit_cast(float, x);
    else return J::widen(x);
  };
  float acc[kChunkRows];
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) {
    const float x0 = asFloat(v[0][j]);
    float t = x0;
    if (initKind != 0) {
      float i32 = __builtin_bit_cast(float, d[j]);
      if constexpr (FT != 3) i32 = initKind == 2 ? i32 : J::widen(d[j]);
      t = (taken[0] >> j) & 1 ? i32 + x0 : i32;
    }
#pragma unroll
    for (int s = 1; s < NS; ++s) t = (taken[s] >> j) & 1 ? t + asFloat(v[s][j]) : t;
    acc[j] = t;
  }

  // each lane stores one word per row: no alignment of `out` matters
  gp<uint8_t> y = startOf(out, b);
  if constexpr (PART) {
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j) {
      const uint32_t i = i0 + 64 * j + lane;
      if (i < n) ((gp<float>)y)[i] = acc[j];  // plain: the next pass reads it
    }
  } else if (FT == 3 || a.outF32 != 0) {
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j) {
      const uint32_t i = i0 + 64 * j + lane;
      if (i < n) __builtin_nontemporal_store(acc[j], (gp<float>)y + i);
    }
  } else if constexpr (FT != 3) {
    // one rounding to nearest even
#pragma unroll
    for (uint32_t j = 0; j < kChunkRows; ++j) {
      const uint32_t i = i0 + 64 * j + lane;
      uint16_t h;
      if constexpr (FT == 1) h = __builtin_bit_cast(uint16_t, _Float16(acc[j]));
      else h = uint16_t(J::bf16Of(acc[j]));
      if (i < n) __builtin_nontemporal_store(h, (gp<uint16_t>)y + i);
    }
  }
}

// c: the sparse inputs (sizes = N, at most c.maxSize) -> the sparse archives
// c.out; denseOut: where each dense archive starts; c.sparseN: a device array
// holding each element's N (the dense archive's size writer adds the sparse
// header and bitmap to outSize, EncTail::sparseN).
template <int FT>
void sparseCompressT(const FloatCompressConfig& config, const CompressCall& c, const BatchDesc& denseOut) {
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const uint32_t nb = c.nb, maxN = c.maxSize;
  constexpr int kSegs = FloatTraits<FT>::kSegs;
  // the list's symbol histogram is counted here for a single element when the
  // three-kernel dense path follows (planSparseCompress, sparse_plan.h): the
  // dense codec then skips its histogram pass
  const SparseCompressPlan plan = planSparseCompress(
      kSegs, sizeof(WordOf<FT>), nb, maxN,
      planCompressCall(FT, nb, maxN, config.useChecksum, false, /*inAligned16=*/true).singlePass);
  const uint32_t tiles = plan.tiles, R = plan.rows;
  const bool countHist = plan.countHist;
  auto tileCounts = res.alloc<uint32_t>(s, plan.tileCounts);
  auto listLen = res.alloc<uint32_t>(s, nb);
  // per tile: its nonzeros in order, plus the n-2 quirk's slot
  auto staging = res.alloc<WordOf<FT>>(s, plan.staging);
  // the compacted lists: 16 B-aligned rows of one arena allocation, lengths
  // on the device
  auto list = res.alloc<uint8_t>(s, plan.listBytes);
  BatchDesc lists = BatchDesc::strided(list.data(), plan.listStride, 0);
  lists.sizes = listLen.data();
  auto table = res.alloc<uint4>(s, plan.tableEntries);
  auto pdf = res.alloc<uint16_t>(s, plan.tableEntries);
  PartialHist pre{nullptr, R};
  pre.table = table.data();
  pre.pdf = pdf.data();
  auto launchAll = [&](uint32_t* histRows, uint32_t* zeroNext) {
    NormArgs na{};
    na.in = c.in;
    na.hist = histRows;
    na.rows = R;
    na.pb = config.ansConfig.probBits;
    na.table = table.data();
    na.pdf = pdf.data();
    na.totalFromHist = true;  // the list length is written by this same launch
    forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) {
      prof::Scope p("sparse", s);
      auto launch = [&](auto vecTag, auto histTag) {
        k_sparseCount<FT, decltype(vecTag)::value, decltype(histTag)::value><<<dim3(tiles, ny), kThreads, 0, s>>>(
            c.in, c.out, y0, nb, tiles, tileCounts.data(), staging.data(), histRows, zeroNext, R);
      };
      if (c.inAligned16) {
        if (countHist) launch(std::true_type{}, std::true_type{});
        else launch(std::true_type{}, std::false_type{});
      } else {
        if (countHist) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
      }
      HIP_LAUNCH_CHECK();
      k_sparseGather<FT><<<dim3(tiles + (countHist ? 1 : 0), ny), kThreads, 0, s>>>(
          c.in, y0, nb, tiles, tileCounts.data(), listLen.data(), staging.data(), lists, na);
      HIP_LAUNCH_CHECK();
    });
  };
  if (countHist) {
    // histogram rows: up to 64 per element, accumulated with atomics into this
    // stream's sync-arena row buffer (zero on entry; k_sparseCount zeroes the
    // other buffer for the next call).  The lease is the arena's newest
    // allocation and ends with this scope, before the dense codec takes its
    // own (the arena's mutex is not recursive).
    SyncLease lease(res, s, kNoSyncRegions, false, plan.rowsBytes);
    pre.rows = static_cast<uint32_t*>(lease.rows[0]);
    launchAll(static_cast<uint32_t*>(lease.rows[0]), static_cast<uint32_t*>(lease.rows[1]));
  } else {
    launchAll(nullptr, nullptr);
  }
  CompressCall dense{res, s};
  dense.nb = nb;
  dense.in = lists;
  dense.maxSize = maxN;
  dense.out = denseOut;
  dense.outSize_dev = c.outSize_dev;
  dense.inAligned16 = true;
  dense.pre = countHist ? &pre : nullptr;
  dense.sparseN = c.sparseN;
  floatCompressDescs(config, dense);
}

// c.form: kFull (c.out are the outputs), or kAccumulate / kAccumulateFp32
// (c.out are the accumulators, capacities in their words; the
// nonzero list is decoded into the scratch rows as in a full call and added
// by k_sparseExpand<FT, ACC>; no checksum is verified, so nothing here waits
// for the stream).
template <int FT>
FloatDecompressStatus sparseDecompressT(const FloatDecompressConfig& config, const DecodeCall& c) {
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const bool full = c.form == DecodeForm::kFull;
  const char* family = full ? "sparse" : "sparse_accumulate";
  const uint32_t nb = c.nb;
  const SparseDecodePlan plan = planSparseDecode(sizeof(WordOf<FT>), nb, c.maxCapacity);
  const uint32_t chunks = plan.chunks, cblocks = plan.cblocks;
  auto densePtrs = res.alloc<uint64_t>(s, nb);
  auto sizes = res.alloc<uint32_t>(s, nb);
  auto denseOk = res.alloc<uint8_t>(s, nb);
  auto list = res.alloc<uint8_t>(s, plan.listBytes);
  auto chunkPre = res.alloc<uint32_t>(s, plan.chunkPre);
  auto blockTot = res.alloc<uint32_t>(s, plan.blockTot);
  forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) {
    prof::Scope p(family, s);
    k_sparseChunks<<<dim3(cblocks, ny), kThreads, 0, s>>>(c.in, y0, chunks, cblocks, densePtrs.data(), sizes.data(),
                                                          chunkPre.data(), blockTot.data());
    HIP_LAUNCH_CHECK();
  });
  // dense decode of the nonzero list (capacity: the largest output)
  DecodeCall dense{res, s};
  dense.nb = nb;
  dense.in = BatchDesc::pointers(densePtrs.data(), nullptr);
  dense.out = BatchDesc::strided(list.data(), plan.listStride, plan.denseCapacity);
  dense.maxCapacity = plan.denseCapacity;
  dense.outSuccess_dev = denseOk.data();
  dense.streamOut = false;  // the expansion reads it
  dense.capacityOnly = true;
  const BatchDesc lists = dense.out;
  auto cfg = config;
  cfg.useChecksum = false;
  floatDecompressDescs(cfg, dense);
  FloatDecompressStatus status;
  if (full && config.useChecksum) {
    // verify the dense archive's checksum over the bytes it was computed on
    // (the first listLen bytes of the nonzero list)
    auto denseLen = res.alloc<uint32_t>(s, nb);
    k_info<<<divUp(nb, 128), 128, 0, s>>>(dense.in, nb, true, denseLen.data(), nullptr, nullptr);
    HIP_LAUNCH_CHECK();
    dense.out.sizes = denseLen.data();
    status = verifiedStatus<FloatDecompressStatus>(dense, true);
  }
  auto expand = [&](auto acc) {
    forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) {
      prof::Scope p(family, s);
      k_sparseExpand<FT, decltype(acc)::value><<<dim3(plan.gridX, ny), kThreads, 0, s>>>(
          c.in, c.out, y0, chunks, cblocks, sizes.data(), chunkPre.data(), blockTot.data(), lists, denseOk.data(),
          c.outSuccess_dev, c.outSize_dev);
      HIP_LAUNCH_CHECK();
    });
  };
  if (full) {
    expand(std::integral_constant<int, 0>{});
  } else if (c.form == DecodeForm::kAccumulate) {
    expand(std::integral_constant<int, 1>{});
  } else {
    DG_CHECK(c.form == DecodeForm::kAccumulateFp32 && (FT == 1 || FT == 2),
             "sparse decode: an fp32 accumulator goes with fp16 / bf16 archives only");
    if constexpr (FT == 1 || FT == 2) expand(std::integral_constant<int, 2>{});
  }
  return status;
}

// One fused reduce call: `in` holds the K * nb archives
// source-major, `partial` the fp32 rows between the passes.
struct SparseReduceCall {
  StackDeviceMemory& res;
  hipStream_t s;
  uint32_t nb;
  const SparseReducePlan& plan;
  const uint64_t* inPtrs;  // device column of the K * nb archive addresses
  BatchDesc init, out, partial;
  uint32_t initKind;
  bool outF32;
  uint8_t* outSuccess_dev;
  uint32_t* outSize_dev;
};

template <int FT, int NS>
void launchSparseReduce(const SparseReduceCall& c, const ReducePass& ps, const BatchDesc& in, const BatchDesc& lists,
                        SparseRedArgs a, const uint32_t* sizes, const uint32_t* chunkPre, const uint32_t* blockTot,
                        const uint8_t* denseOk, const uint8_t* verdictIn, uint8_t* verdictOut, uint32_t* firstN) {
  forGridYSlices(c.nb, [&](uint32_t y0, uint32_t ny) {
    prof::Scope p("sparse_reduce", c.s);
    a.batchOffset = y0;
    const BatchDesc& init = ps.initIsPartial ? c.partial : c.init;
    const dim3 grid(c.plan.d.gridX, ny);
    if (ps.outIsPartial) {
      k_sparseReduce<FT, NS, true><<<grid, kThreads, 0, c.s>>>(in, init, c.partial, a, sizes, chunkPre, blockTot,
                                                               lists, denseOk, verdictIn, verdictOut, firstN,
                                                               c.outSuccess_dev, c.outSize_dev);
    } else {
      k_sparseReduce<FT, NS, false><<<grid, kThreads, 0, c.s>>>(in, init, c.out, a, sizes, chunkPre, blockTot, lists,
                                                                denseOk, verdictIn, verdictOut, firstN,
                                                                c.outSuccess_dev, c.outSize_dev);
    }
    HIP_LAUNCH_CHECK();
  });
}

// The passes of planReduce, each: the chunk counts of the pass's NS * nb
// archives, one dense full decode of their nonzero lists into the scratch
// rows, one k_sparseReduce launch.  Rows, counts and totals are sized for the
// widest pass and reused by the next one (everything is stream-ordered), so
// the scratch is bounded by the sources per launch, not by K.
template <int FT>
void sparseReduceT(const FloatDecompressConfig& config, const SparseReduceCall& c) {
  static_assert(kSparseReduceMaxNS == 4, "one case per instance");
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const SparseReducePlan& plan = c.plan;
  const uint32_t nb = c.nb, chunks = plan.d.chunks, cblocks = plan.d.cblocks;
  auto densePtrs = res.alloc<uint64_t>(s, plan.densePtrs);
  auto sizes = res.alloc<uint32_t>(s, plan.sizes);
  auto denseOk = res.alloc<uint8_t>(s, plan.denseOk);
  auto list = res.alloc<uint8_t>(s, plan.d.listBytes);
  auto chunkPre = res.alloc<uint32_t>(s, plan.d.chunkPre);
  auto blockTot = res.alloc<uint32_t>(s, plan.d.blockTot);
  auto verdict = res.alloc<uint8_t>(s, plan.verdict);
  auto firstN = res.alloc<uint32_t>(s, plan.firstN);
  auto cfg = config;
  cfg.useChecksum = false;
  for (uint32_t i = 0; i < plan.passes.numPasses; ++i) {
    const ReducePass& ps = plan.passes.passes[i];
    const uint32_t rows = ps.count * nb;
    const BatchDesc in = BatchDesc::pointers(c.inPtrs + uint64_t(ps.first) * nb, nullptr);
    forGridYSlices(rows, [&](uint32_t y0, uint32_t ny) {
      prof::Scope p("sparse_reduce", s);
      k_sparseChunks<<<dim3(cblocks, ny), kThreads, 0, s>>>(in, y0, chunks, cblocks, densePtrs.data(), sizes.data(),
                                                            chunkPre.data(), blockTot.data());
      HIP_LAUNCH_CHECK();
    });
    DecodeCall dense{res, s};
    dense.nb = rows;
    dense.in = BatchDesc::pointers(densePtrs.data(), nullptr);
    dense.out = BatchDesc::strided(list.data(), plan.d.listStride, plan.d.denseCapacity);
    dense.maxCapacity = plan.d.denseCapacity;
    dense.outSuccess_dev = denseOk.data();
    dense.streamOut = false;  // the reduce reads it
    dense.capacityOnly = true;
    floatDecompressDescs(cfg, dense);
    SparseRedArgs a{};
    a.nb = nb;
    a.chunksPerElem = chunks;
    a.blocksPerElem = cblocks;
    a.initKind = ps.initIsPartial ? 2u : c.initKind;
    a.outF32 = ps.outIsPartial || c.outF32 ? 1u : 0u;
    a.first = i == 0 ? 1u : 0u;
    a.last = ps.outIsPartial ? 0u : 1u;
    const uint8_t* verdictIn = verdict.data() + size_t((i + 1) & 1) * nb;
    uint8_t* verdictOut = verdict.data() + size_t(i & 1) * nb;
    auto launch = [&](auto ns) {
      launchSparseReduce<FT, decltype(ns)::value>(c, ps, in, dense.out, a, sizes.data(), chunkPre.data(),
                                                  blockTot.data(), denseOk.data(), verdictIn, verdictOut,
                                                  firstN.data());
    };
    switch (ps.count) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      case 4: launch(std::integral_constant<int, 4>{}); break;
      default: DG_CHECK(false, "no k_sparseReduce instance of " << ps.count << " sources");
    }
  }
}

// ---------------------------------------------------------------------------
// Range decode: words [first, first + count) of the element a
// sparse archive encodes.  rank(i) = the set bitmap bits among words [0, i);
// gap = N >= 2 && bit(N-2) == 0.  Word i < N-1 lives at list index rank(i),
// word N-1 at rank(N-1) + gap, so the range needs the list slice
// [rank(first), rank(end) + (gap && end == N)): at most count + 1 words.
// Four stream-ordered launches: the chunk counts of each DISTINCT archive
// (k_sparseRangeChunks), the ranks of each member's range
// (k_sparseRangePlan), the dense range decode of the list slices into scratch
// rows (k_decode<RNG>), the expansion (k_sparseExpandRange).
// ---------------------------------------------------------------------------
// The device columns of one call: per distinct archive its address and where
// its counts live, per member its archive's slot, `first` and `count`.
struct SparseRangeTabs {
  const uint64_t* archPtr;    // [archives]
  const uint64_t* archInfo;   // [archives] first k_sparseRangeChunks workgroup | chunks counted << 32
  const uint64_t* slotFirst;  // [members] archive slot | first << 32
  const uint32_t* count;      // [members]
};

// N of the sparse archive at a: word 0 of its header.  The 12 bytes after it
// are don't-care (the reference leaves them uninitialised) and
// are not looked at.  A word 0 equal to the float or the ANS magic is a dense
// float or byte archive passed in by mistake, not an N: no sparse archive
// holds 3.5e9 words or more (its dense part's raw bytes alone pass the
// archives' 32-bit sizes in every float type), and a dense archive located
// sparsePrefixBytes(magic) bytes further would be read far outside the
// caller's buffer.  Then ok = false, N = 0.
__device__ __forceinline__ uint32_t sparseSizeOf(gp<const uint8_t> a, bool& ok) {
  const uint32_t n = readfirst(((gp<const uint32_t>)a)[kSparseSize]);
  ok = n != kFloatMagicVersion && n != kANSMagicVersion;
  return ok ? n : 0u;
}

// r1: k_sparseChunks' counting, once per distinct archive and only for the
// chunks some member's range needs.  grid (workgroups of the archive with
// the most chunks, archives): archive a's workgroup g owns chunks [256 g,
// 256 g + 256) and entries 256 (g0 + g) + t of chunkPre, g0 + g of blockTot.
// Workgroups wholly past the archive's N or its counted chunks write nothing
// (no rank reads them).
__global__ __launch_bounds__(kThreads) void k_sparseRangeChunks(SparseRangeTabs t, uint32_t archOffset,
                                                                uint32_t* __restrict__ chunkPre,
                                                                uint32_t* __restrict__ blockTot) {
  __shared__ uint32_t red[kWaves];
  const uint32_t slot = archOffset + blockIdx.y;
  const uint64_t info = BatchDesc::tableAt(t.archInfo, slot);
  const uint32_t g0 = uint32_t(info), nChunks = uint32_t(info >> 32);
  if (blockIdx.x * kThreads >= nChunks) return;
  gp<const uint8_t> a = (gp<const uint8_t>)reinterpret_cast<const uint8_t*>(BatchDesc::tableAt(t.archPtr, slot));
  bool hdrOk;
  const uint32_t n = sparseSizeOf(a, hdrOk);
  if (uint64_t(blockIdx.x) * kThreads * kChunkWords >= n) return;
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  const uint64_t g = uint64_t(g0) + blockIdx.x;
  countAndScanChunks(a + kSparseHeaderBytes, c, nChunks, n, red, G(chunkPre) + g * kThreads + threadIdx.x,
                     G(blockTot) + g);
}

// This lane's share of rank(i) of archive `bm` (its bitmap), 1 <= i <= N:
// chunk c = (i - 1) / 1024 holds the boundary (so i == N needs no chunk past
// the counted ones); lanes stride over the totals of c's earlier workgroups,
// lanes 0-15 count the chunk's bitmap words below the boundary, lane 16 adds
// the chunk's prefix.  waveSum of the shares is the rank.
__device__ __forceinline__ uint32_t rankShare(gp<const uint8_t> bm, gp<const uint32_t> chunkPre,
                                              gp<const uint32_t> blockTot, uint32_t i, uint32_t lane) {
  const uint32_t c = (i - 1) / kChunkWords;
  const uint32_t within = i - c * kChunkWords;  // 1 .. 1024 words of chunk c lie below i
  uint32_t part = totalsShare(blockTot, c / kThreads, lane);
  if (lane == 16) part += chunkPre[c];
  return part + uint32_t(__popcll(chunkBitmapWord(bm, c, within, lane)));
}

// r2: one wave per member: N, the range check, rank(first) and rank(end) ->
// the dense archive's address, the list slice [listFirst, + listCount) (0, 0
// for a failing or empty range) and flags (bit 0: the range is valid, bit 1:
// gap).  A member that is a dense archive (sparseSizeOf) gets `dummy` (64
// zero words, written here) as its dense archive, so that the dense decoder's
// header reads -- the first 64 bytes of an element of size 0, see k_decode --
// stay inside this call's memory and fail its magic check.
// (at most 80 SGPRs, as its siblings: MI355X_MICROARCH.md, Residency)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(80))) void k_sparseRangePlan(
    SparseRangeTabs t, uint32_t numInBatch, const uint32_t* __restrict__ chunkPre,
    const uint32_t* __restrict__ blockTot, uint64_t* __restrict__ densePtrs, uint32_t* __restrict__ listFirst,
    uint32_t* __restrict__ listCount, uint8_t* __restrict__ flags, uint32_t* __restrict__ dummy) {
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t b = blockIdx.x * kWaves + w;
  if (b >= numInBatch) return;
  const uint64_t sf = BatchDesc::tableAt(t.slotFirst, b);
  const uint32_t slot = uint32_t(sf), first = uint32_t(sf >> 32);
  const uint32_t count = BatchDesc::tableAt(t.count, b);
  const uint64_t info = BatchDesc::tableAt(t.archInfo, slot);
  const uint64_t addr = BatchDesc::tableAt(t.archPtr, slot);
  gp<const uint8_t> a = (gp<const uint8_t>)reinterpret_cast<const uint8_t*>(addr);
  bool hdrOk;
  const uint32_t n = sparseSizeOf(a, hdrOk);
  const bool ok = hdrOk && first <= n && count <= n - first;
  uint32_t lf = 0, lc = 0;
  bool gap = false;
  if (ok && count != 0) {
    const uint32_t end = first + count;  // <= n: no wrap
    gp<const uint8_t> bm = a + kSparseHeaderBytes;
    gp<const uint32_t> pre = G(chunkPre) + uint64_t(uint32_t(info)) * kThreads;
    gp<const uint32_t> tot = G(blockTot) + uint32_t(info);
    gap = gapBit(bm, n);
    const uint32_t s0 = first ? rankShare(bm, pre, tot, first, lane) : 0u;
    const uint32_t s1 = rankShare(bm, pre, tot, end, lane);
    lf = waveSum(s0);
    lc = waveSum(s1) - lf + (gap && end == n ? 1u : 0u);
  }
  if (!hdrOk) G(dummy)[lane] = 0;
  if (lane == 0) {
    G(densePtrs)[b] = hdrOk ? addr + sparsePrefixBytes(n) : reinterpret_cast<uint64_t>(dummy);
    G(listFirst)[b] = lf;
    G(listCount)[b] = lc;
    G(flags)[b] = uint8_t((ok ? 1u : 0u) | (gap ? 2u : 0u));
  }
}

// r4: expand the decoded list slices into the outputs, k_sparseExpand's body
// (expandRows): one wave per 1024-word chunk the range touches (grid
// (ceil((ceil(maxCount / 1024) + 1) / 4), members): a range's start inside a
// chunk is arbitrary), 16 bitmap words in lanes 0-15, list offset = the
// chunk's rank - listFirst (modulo 2^32: the first chunk's rank lies at or
// below listFirst); no LDS, no barrier.  Rows are masked to [first, end);
// word i goes to out[i - first] with plain stores (the destination is not
// row-aligned and is read right after).  Members that failed return before
// any index is formed: for the others every index lies in [0, listCount) by
// construction (listCount counts the same bitmap bits), whatever a corrupt
// bitmap holds.  Writes outSuccess / outSize of every member.
// (at most 80 SGPRs, as its siblings: MI355X_MICROARCH.md, Residency)
template <int FT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(80))) void k_sparseExpandRange(
    SparseRangeTabs t, BatchDesc out, uint32_t batchOffset, const uint32_t* __restrict__ chunkPre,
    const uint32_t* __restrict__ blockTot, const uint32_t* __restrict__ listFirst,
    const uint8_t* __restrict__ flags, BatchDesc lists, const uint8_t* __restrict__ denseOk,
    uint8_t* __restrict__ outSuccess, uint32_t* __restrict__ outSize) {
  using W = WordOf<FT>;
  const uint32_t b = batchOffset + blockIdx.y;
  const uint32_t count = BatchDesc::tableAt(t.count, b);
  const uint32_t fl = flags[b];
  const bool ok = (fl & 1) != 0 && denseOk[b] != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (outSuccess) G(outSuccess)[b] = ok ? 1 : 0;
    if (outSize) G(outSize)[b] = ok ? count : 0u;
  }
  if (!ok || count == 0) return;
  const uint64_t sf = BatchDesc::tableAt(t.slotFirst, b);
  const uint32_t slot = uint32_t(sf), first = uint32_t(sf >> 32);
  const uint32_t end = first + count;  // <= N (k_sparseRangePlan)
  const uint32_t lane = threadIdx.x & 63, w = readfirst(threadIdx.x >> 6);
  const uint32_t c = first / kChunkWords + blockIdx.x * kWaves + w;
  if (c > (end - 1) / kChunkWords) return;
  const uint32_t i0 = c * kChunkWords;
  const uint64_t info = BatchDesc::tableAt(t.archInfo, slot);
  gp<const uint8_t> a = (gp<const uint8_t>)reinterpret_cast<const uint8_t*>(BatchDesc::tableAt(t.archPtr, slot));
  gp<const uint8_t> bm = a + kSparseHeaderBytes;
  // (the bits at or past `end` are cut: no wanted word's list index counts them)
  const uint64_t mv = chunkBitmapWord(bm, c, end - i0, lane);
  // the chunk's rank less the slice's start
  const uint32_t base = chunkListOffset(G(chunkPre) + uint64_t(uint32_t(info)) * kThreads,
                                        G(blockTot) + uint32_t(info), c, lane) -
                        BatchDesc::tableAt(listFirst, b);
  // x[N-1] is read one slot further when x[N-2] == 0: only a range that ends
  // at N reaches it
  const uint32_t n = ((gp<const uint32_t>)a)[kSparseSize];
  const bool gap = (fl & 2) != 0;
  // rows are masked to [first, end).  (i0 + 1023 may wrap past 2^32 - 1 in
  // the last chunk of a 2^32-word element: compare offsets from i0, which do
  // not)
  auto inRange = [&](uint32_t i) __attribute__((always_inline)) { return i - i0 < end - i0 && i >= first; };
  W v[kChunkRows];
  expandRows(mv, base, i0, n, gap, (gp<const W>)lists.start(b), lane, inRange, v);
  gp<W> y = (gp<W>)out.start(b);
#pragma unroll
  for (uint32_t j = 0; j < kChunkRows; ++j) {
    const uint32_t i = i0 + 64 * j + lane;
    if (inRange(i)) y[i - first] = v[j];
  }
}

// One range call: the members `in` (archives), first / count / out as host
// columns, already validated.
struct SparseRangeCall {
  StackDeviceMemory& res;
  hipStream_t s;
  uint32_t nb;
  const std::vector<uint64_t>& in;
  const std::vector<uint64_t>& out;
  const uint32_t* first;
  const uint32_t* count;
  uint8_t* outSuccess_dev;
  uint32_t* outSize_dev;
};

template <int FT>
void sparseRangeT(const FloatDecompressConfig& config, const SparseRangeCall& c) {
  using W = WordOf<FT>;
  StackDeviceMemory& res = c.res;
  const hipStream_t s = c.s;
  const uint32_t nb = c.nb;
  // the distinct archives, each counted once up to the largest range end
  // among its members, and the sizes of everything below (sparse_plan.h)
  const SparseRangePlan plan = planSparseRange(c.in.data(), c.first, c.count, nb);
  DG_CHECK(!plan.tooLarge, "range ends too large for one call");
  const std::vector<uint32_t> counts(c.count, c.count + nb);
  const auto t = uploadTables(res, s, {&plan.archPtr, &plan.archInfo, &c.out, &plan.slotFirst}, counts);
  const SparseRangeTabs tabs{t.u64[0], t.u64[1], t.u64[3], t.u32};
  auto chunkPre = res.alloc<uint32_t>(s, plan.chunkPre);
  auto blockTot = res.alloc<uint32_t>(s, plan.blockTot);
  auto densePtrs = res.alloc<uint64_t>(s, nb);
  auto listFirst = res.alloc<uint32_t>(s, nb);
  auto listCount = res.alloc<uint32_t>(s, nb);
  auto flags = res.alloc<uint8_t>(s, nb);
  auto denseOk = res.alloc<uint8_t>(s, nb);
  auto dummy = res.alloc<uint32_t>(s, 64);
  // the list slices: 16 B-aligned rows of count + 1 words at most, sized by
  // the call's largest count; a call whose rows do not fit the arena throws
  // (GpuFloatCodec.h)
  auto slices = res.alloc<uint8_t>(s, size_t(nb) * plan.rowWords * sizeof(W));
  if (plan.totalBlocks != 0) {
    forGridYSlices(plan.nArch, [&](uint32_t y0, uint32_t ny) {
      prof::Scope p("sparse", s);
      k_sparseRangeChunks<<<dim3(plan.maxCblocks, ny), kThreads, 0, s>>>(tabs, y0, chunkPre.data(), blockTot.data());
      HIP_LAUNCH_CHECK();
    });
  }
  {
    prof::Scope p("sparse", s);
    k_sparseRangePlan<<<divUp(nb, kWaves), kThreads, 0, s>>>(tabs, nb, chunkPre.data(), blockTot.data(),
                                                             densePtrs.data(), listFirst.data(), listCount.data(),
                                                             flags.data(), dummy.data());
    HIP_LAUNCH_CHECK();
  }
  // dense range decode of the slices
  DecodeCall dense{res, s};
  dense.nb = nb;
  dense.in = BatchDesc::pointers(densePtrs.data(), listFirst.data());
  dense.out = BatchDesc::strided(slices.data(), plan.rowWords * sizeof(W), 0);
  dense.out.sizes = listCount.data();
  dense.outSuccess_dev = denseOk.data();
  dense.form = DecodeForm::kRange;
  dense.maxRangeBlocks = plan.maxRangeBlocks;
  floatDecompressDescs(config, dense);
  const BatchDesc outs = BatchDesc::pointers(t.u64[2], nullptr);
  forGridYSlices(nb, [&](uint32_t y0, uint32_t ny) {
    prof::Scope p("sparse", s);
    k_sparseExpandRange<FT><<<dim3(plan.expandGridX, ny), kThreads, 0, s>>>(
        tabs, outs, y0, chunkPre.data(), blockTot.data(), listFirst.data(), flags.data(), dense.out, denseOk.data(),
        c.outSuccess_dev, c.outSize_dev);
    HIP_LAUNCH_CHECK();
  });
}

}  // namespace

uint32_t getMaxSparseFloatCompressedSize(FloatType ft, uint32_t size) {
  const uint64_t v = sparsePrefixBytes(size) + getMaxFloatCompressedSize(ft, size);
  DG_CHECK(v <= uint64_t(UINT32_MAX), "input too large: " << size << " float words");
  return uint32_t(v);
}

// The sparse kernels take no InlineTable: DeviceDescs turns the tables of a
// batch (pointerBatch, batch_tables.h) into one device upload, or for one
// element (the reference's SparseFloatBenchmark shape) into stride descriptors
// without any upload.
void floatCompressSparse(StackDeviceMemory& res, const FloatCompressConfig& config,
                         uint32_t numInBatch, const void** in, const uint32_t* inSize, void** out,
                         uint32_t* outSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return;
  checkFloatConfig(config);
  // third column: the dense archives, after header and bitmap
  const auto b = pointerBatch(res, stream, numInBatch, in, out, inSize, true, floatWordBytes(int(config.floatType)),
                              [](uint32_t n) { return sparsePrefixBytes(n); });
  const DeviceDescs dd(res, stream, &b.t, numInBatch);
  CompressCall c = compressCall(res, stream, numInBatch, b, outSize_dev);
  c.in = dd.map(b.in);
  c.out = dd.map(b.out);
  c.tabs = nullptr;
  // one element: the dense archive's size writer reads N from the sparse
  // header k_sparseCount writes first (word 0 of the archive)
  c.sparseN = numInBatch == 1 ? reinterpret_cast<const uint32_t*>(out[0]) : c.in.sizes;
  const BatchDesc denseOut = dd.map(b.out2);
  dispatchFloatType(config.floatType, [&](auto f) { sparseCompressT<decltype(f)::value>(config, c, denseOut); });
}

// c's descriptors mapped for the sparse kernels (DeviceDescs in the caller's scope)
static DecodeCall mapped(DecodeCall c, const DeviceDescs& dd) {
  c.in = dd.map(c.in);
  c.out = dd.map(c.out);
  c.tabs = nullptr;
  return c;
}

FloatDecompressStatus floatDecompressSparse(StackDeviceMemory& res,
                                            const FloatDecompressConfig& config,
                                            uint32_t numInBatch, const void** in, void** out,
                                            const uint32_t* outCapacity, uint8_t* outSuccess_dev,
                                            uint32_t* outSize_dev, hipStream_t stream) {
  if (numInBatch == 0) return FloatDecompressStatus();
  checkFloatConfig(config);
  // unit 1: this entry point has never checked its outputs' alignment
  const auto b = pointerBatch(res, stream, numInBatch, in, out, outCapacity, false, 1);
  const DeviceDescs dd(res, stream, &b.t, numInBatch);
  const DecodeCall c = mapped(decodeCall(res, stream, numInBatch, b, outSuccess_dev, outSize_dev), dd);
  return dispatchFloatType(config.floatType,
                           [&](auto f) { return sparseDecompressT<decltype(f)::value>(config, c); });
}

// Sparse decode-and-accumulate: the dense entry point's
// checks, with 16-byte aligned archives.
void floatDecompressSparseAccumulate(StackDeviceMemory& res, const FloatDecompressConfig& config,
                                     uint32_t numInBatch, const void** in, void** acc,
                                     const uint32_t* accCapacity, FloatType accType, uint8_t* outSuccess_dev,
                                     uint32_t* outSize_dev, hipStream_t stream) {
  accumulateEntry(res, config, numInBatch, in, acc, accCapacity, accType, outSuccess_dev, outSize_dev, stream, 16,
                  [&](const DecodeCall& call) {
                    const DeviceDescs dd(res, stream, call.tabs, numInBatch);
                    const DecodeCall c = mapped(call, dd);
                    dispatchFloatType(config.floatType,
                                      [&](auto f) { sparseDecompressT<decltype(f)::value>(config, c); });
                  });
}

// The most sources one k_sparseReduce launch takes: the tuning hook of the
// dense reduce (dietgpu_set_reduce_max_sources), capped at the largest instance.
static uint32_t sparseReduceNsMax() {
  const uint32_t hook = reduceMaxSources();
  return hook >= 1 && hook < kSparseReduceMaxNS ? hook : kSparseReduceMaxNS;
}

uint64_t floatReduceSparseScratchBytes(FloatType floatType, uint32_t numInBatch, uint32_t numSources,
                                       uint32_t maxCapacity) {
  const int ft = int(floatType);
  checkReduceShape(ft, numSources, false, ft, ft);
  return planSparseReduce(floatWordBytes(ft), numInBatch, numSources, sparseReduceNsMax(), maxCapacity, true)
      .scratchBytes;
}

// Fused sparse reduce: floatReduceArchives' checks, with
// 16-byte aligned archives; every host check before the first allocation,
// upload or launch.
void floatReduceSparseArchives(StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch,
                               uint32_t numSources, const void** in, const void** init, FloatType initType,
                               void** out, const uint32_t* outCapacity, FloatType outType, uint8_t* outSuccess_dev,
                               uint32_t* outSize_dev, hipStream_t stream) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kReduce);
  const int ft = int(config.floatType);
  checkReduceShape(ft, numSources, init != nullptr, int(initType), int(outType));
  checkProbBits(config.ansConfig.probBits);
  const uint32_t nb = numInBatch, K = numSources;
  if (nb == 0) return;
  DG_CHECK(uint64_t(nb) * K < (1ull << 32), "numInBatch x numSources must be below 2^32");
  DG_CHECK(in && out && outCapacity, "in, out and outCapacity must not be null");
  const bool outF32 = outType == FloatType::kFloat32;
  const uint32_t initKind = !init ? 0u : (initType == FloatType::kFloat32 ? 2u : 1u);
  const auto ip = addressColumn(in, nb * K), op = addressColumn(out, nb);
  const auto np = init ? addressColumn(init, nb) : std::vector<uint64_t>();
  for (uint32_t i = 0; i < nb * K; ++i) checkArchiveAligned(ip[i], i, 16);
  for (uint32_t i = 0; i < nb; ++i) {
    DG_CHECK(op[i] % (outF32 ? 4 : 2) == 0, "float output " << i << " not aligned to its word size");
    DG_CHECK(!init || np[i] % (initKind == 2 ? 4 : 2) == 0, "init " << i << " not aligned to its word size");
  }
  const SizeColumn cap(outCapacity, nb);
  const SparseReducePlan plan =
      planSparseReduce(floatWordBytes(ft), nb, K, sparseReduceNsMax(), cap.maxSize, init != nullptr);
  DG_CHECK(plan.valid, "numSources (" << K << ") must be in 1 .. " << kReduceMaxSources);

  // device columns (the sparse kernels take no InlineTable), then the fp32
  // partial of a chained call: nb rows of the largest capacity
  const DeviceTables t = uploadTables(res, stream, {&ip, &op, &np}, cap.sizes);
  auto partial = res.alloc<float>(stream, size_t(plan.partialWords));
  BatchDesc partD = BatchDesc::strided(partial.data(), plan.partialWords / nb * sizeof(float), 0);
  partD.sizes = t.u32;
  const SparseReduceCall c{res,
                           stream,
                           nb,
                           plan,
                           t.u64[0],
                           BatchDesc::pointers(t.u64[2], nullptr),
                           BatchDesc::pointers(t.u64[1], t.u32),
                           partD,
                           initKind,
                           outF32,
                           outSuccess_dev,
                           outSize_dev};
  dispatchFloatType(config.floatType, [&](auto f) {
    constexpr int FT = decltype(f)::value;
    if constexpr (FT <= 3) sparseReduceT<FT>(config, c);
  });
}

// Every host check precedes the first allocation, upload or launch.
void floatDecompressSparseRange(StackDeviceMemory& res, const FloatDecompressConfig& config,
                                uint32_t numInBatch, const void** in, const uint32_t* first,
                                const uint32_t* count, void** out, uint8_t* outSuccess_dev,
                                uint32_t* outSize_dev, hipStream_t stream) {
  checkFloatConfig(config);
  checkProbBits(config.ansConfig.probBits);
  checkNoChecksum(config.useChecksum, PartialDecode::kRange);
  if (numInBatch == 0) return;
  const uint32_t ws = floatWordBytes(int(config.floatType));
  const auto ip = addressColumn(in, numInBatch), op = addressColumn(out, numInBatch);
  for (uint32_t i = 0; i < numInBatch; ++i) {
    DG_CHECK(op[i] % ws == 0, "float output " << i << " not aligned to its word size");
    checkArchiveAligned(ip[i], i, 16);
  }
  const SparseRangeCall c{res, stream, numInBatch, ip, op, first, count, outSuccess_dev, outSize_dev};
  dispatchFloatType(config.floatType, [&](auto f) { sparseRangeT<decltype(f)::value>(config, c); });
}

}  // namespace dietgpu
