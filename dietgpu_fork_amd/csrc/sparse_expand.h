// What the kernels that read a sparse float archive share (sparse.hip: the
// full decode, the accumulate and range forms, the fused reduce;
// sparse_matmul.h: the matmul): the bitmap of a 1024-word chunk, the chunk
// counts and their scan (k_sparseChunks), a chunk's list offset, and the one
// expander, expandRows.  Moved here from sparse.hip word for word, so that a
// second translation unit can hold kernels built on them; every definition
// keeps internal linkage (each translation unit compiles its own copy, as
// before).  The wire format is described at the top of sparse.hip.
#pragma once

#include "decode.h"
#include "encode.h"  // kThreads, kWaves: the sparse kernels' workgroup

namespace dietgpu {

namespace {

// Decompression works on 1024-word chunks (16 bitmap words, one wave).
constexpr uint32_t kChunkWords = 1024;
constexpr uint32_t kChunkRows = kChunkWords / 64;  // 64-word rows, one bitmap word each

template <int FT>
using WordOf = typename FloatTraits<FT>::WordT;

// flags of words [base, base + 64) as a lane mask <-> packed bitmap u64
__device__ __forceinline__ uint64_t maskToBitmap(uint64_t m) {
  return __builtin_bswap64(__builtin_bitreverse64(m));
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

}  // namespace

}  // namespace dietgpu
