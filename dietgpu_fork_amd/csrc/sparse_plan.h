// The host arithmetic of the four sparse drivers (sparse.hip sparseCompressT,
// sparseDecompressT, sparseReduceT, sparseRangeT): tiles, chunks, rows, strides,
// grids and the element counts of every allocation, for a reduce call its
// passes and total scratch, and for a range call the member sort and the
// packed host columns.  Host only and free of HIP headers, as
// compress_plan.h and decode_plan.h are, so that it is stated once and swept
// without a GPU (tests/test_sparse_plan.py, tests/test_sparse_reduce_plan.py).
// The drivers allocate what a plan names and launch; they compute nothing else.
//
// Sizes and capacities are combined in 32 bits where the drivers always did
// (div32 / round32 below): a size within 4,095 words of 2^32 wraps.  No
// archive holds such an element (its raw bytes alone pass the archives' 32-bit
// sizes in every float type, getMaxSparseFloatCompressedSize refuses it), and
// a decode capacity that large makes the dense stage's capacity 0, so the
// member fails.  Products of counts are formed in 64 bits.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "compress_plan.h"
#include "decode_plan.h"

namespace dietgpu {

namespace splan {
// (sparse.hip static_asserts them against the kernels' constants)
constexpr uint32_t kTileWords = 4096;   // words of a k_sparseCount workgroup
constexpr uint32_t kChunkWords = 1024;  // words a wave expands: 16 bitmap words
constexpr uint32_t kThreads = 256;      // chunks a counting workgroup scans
constexpr uint32_t kWaves = kThreads / 64;

constexpr uint32_t div32(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
constexpr uint32_t round32(uint32_t a, uint32_t b) { return div32(a, b) * b; }

// Bytes between the rows of the compacted nonzero lists (compress: the dense
// codec's input; decode: its output): 16 B-aligned rows with room for the n-2
// quirk's slot and a whole last vector.
constexpr uint64_t listStride(uint32_t maxWords, uint32_t wordBytes) {
  return uint64_t(round32(maxWords, 16) + 16) * wordBytes;
}
}  // namespace splan

// ---------------------------------------------------------------------------
// compress: nb elements of at most maxN words
// ---------------------------------------------------------------------------
struct SparseCompressPlan {
  uint32_t tiles = 1;      // k_sparseCount workgroups per element
  uint32_t rows = 1;       // histogram rows per element and segment (PartialHist::nRows)
  bool countHist = false;  // k_sparseCount counts the list's histogram, k_sparseGather normalises it
  uint64_t rowsBytes = 0;  // ... into a rows lease of this size (SyncLease); 0: no lease
  // element counts of the allocations
  uint64_t tileCounts = 0;  // u32
  uint64_t staging = 0;     // words: per tile its nonzeros in order, plus the n-2 quirk's slot
  uint64_t listBytes = 0;   // the compacted lists
  uint64_t tableEntries = 0;  // encode-table entries (uint4) and pdfs (u16), each; 1 when unused
  uint64_t listStride = 0;  // bytes between the lists' rows
};

// denseSinglePass: the dense codec would take the compacted lists single-pass
// (planCompress), counting as it loads.  Otherwise a single element's
// histogram is counted here (c4 1 x 15M fp32: compress 85 -> 75 us); it
// lengthens every tile's workgroup, so with more elements the separate k_hist
// over the compacted lists is faster (5 x 15M: 155 us against 170).
inline SparseCompressPlan planSparseCompress(int segs, uint32_t wordBytes, uint32_t nb, uint32_t maxN,
                                             bool denseSinglePass) {
  SparseCompressPlan p;
  p.tiles = std::max(1u, splan::div32(maxN, splan::kTileWords));
  p.rows = std::min(p.tiles, kReduceRows);
  p.countHist = nb == 1 && !denseSinglePass;
  p.rowsBytes = p.countHist ? uint64_t(segs) * nb * p.rows * cplan::kSymbols * 4 : 0;
  p.tileCounts = uint64_t(nb) * p.tiles;
  p.staging = uint64_t(nb) * p.tiles * (splan::kTileWords + 1);
  p.listStride = splan::listStride(maxN, wordBytes);
  p.listBytes = uint64_t(nb) * p.listStride;
  p.tableEntries = p.countHist ? uint64_t(segs) * nb * cplan::kSymbols : 1;
  return p;
}

// ---------------------------------------------------------------------------
// full decode and decode-and-accumulate: nb archives, capacities at most maxCap
// ---------------------------------------------------------------------------
struct SparseDecodePlan {
  uint32_t chunks = 1;   // 1024-word chunks per element
  uint32_t cblocks = 1;  // k_sparseChunks workgroups per element
  uint32_t gridX = 1;    // k_sparseExpand workgroups per element: a chunk per wave
  uint32_t denseCapacity = 0;  // the dense call's capacity: the n-2 quirk's slot more
  uint64_t listStride = 0;     // bytes between the decoded lists' rows
  // element counts of the allocations
  uint64_t listBytes = 0;
  uint64_t chunkPre = 0, blockTot = 0;  // u32
};

inline SparseDecodePlan planSparseDecode(uint32_t wordBytes, uint32_t nb, uint32_t maxCap) {
  SparseDecodePlan p;
  p.chunks = std::max(1u, splan::div32(maxCap, splan::kChunkWords));
  p.cblocks = splan::div32(p.chunks, splan::kThreads);
  p.gridX = splan::div32(p.chunks, splan::kWaves);
  p.denseCapacity = maxCap + 1;
  p.listStride = splan::listStride(maxCap, wordBytes);
  p.listBytes = uint64_t(nb) * p.listStride;
  p.chunkPre = uint64_t(nb) * p.chunks;
  p.blockTot = uint64_t(nb) * p.cblocks;
  return p;
}

// ---------------------------------------------------------------------------
// fused reduce: nb members of K sparse archives each,
// capacities at most maxCap, at most nsMax sources per k_sparseReduce launch
// ---------------------------------------------------------------------------
// The largest k_sparseReduce instance (sparse.hip static_asserts it).
constexpr uint32_t kSparseReduceMaxNS = 4;

struct SparseReducePlan {
  bool valid = false;  // planReduce's: 1 <= K <= 64, nsMax >= 1
  ReducePlan passes{};  // which sources go in which pass, which passes touch the fp32 partial
  uint32_t ns = 0;      // sources of the widest pass (the first)
  uint32_t rows = 0;    // ns * nb: the archives one pass counts, decodes and expands
  // per pass: k_sparseChunks grid (d.cblocks, rows) in grid-y slices, one dense
  // decode of `rows` lists (capacity d.denseCapacity), k_sparseReduce grid
  // (d.gridX, nb) in grid-y slices
  SparseDecodePlan d;
  // element counts of the allocations; the per-pass ones are sized for the
  // widest pass and reused by every pass (d.listBytes, d.chunkPre and
  // d.blockTot count `rows` archives)
  uint64_t tableBytes = 0;    // u8: the address columns in (K nb), out (nb), init (nb, if any), then the capacities
  uint64_t partialWords = 0;  // fp32: nb rows of maxCap rounded up to 4 words; 0 for one pass
  uint64_t densePtrs = 0;     // u64 [rows]
  uint64_t sizes = 0;         // u32 [rows]
  uint64_t denseOk = 0;       // u8 [rows]
  uint64_t verdict = 0;       // u8 [2][nb]: the members still good after the even / odd passes
  uint64_t firstN = 0;        // u32 [nb]: n of each member's first source
  // the arena bytes of the whole call: every allocation above rounded up to
  // the arena's 256-byte granule (an empty one takes a granule too)
  uint64_t scratchBytes = 0;
};

inline SparseReducePlan planSparseReduce(uint32_t wordBytes, uint32_t nb, uint32_t K, uint32_t nsMax,
                                         uint32_t maxCap, bool hasInit) {
  SparseReducePlan p;
  const uint64_t rowWords = uint64_t(splan::round32(maxCap, 4));
  p.passes = planReduce(K, std::min(nsMax, kSparseReduceMaxNS), uint64_t(nb) * rowWords);
  p.valid = p.passes.valid;
  if (!p.valid) return p;
  p.ns = p.passes.passes[0].count;
  p.rows = p.ns * nb;
  p.d = planSparseDecode(wordBytes, p.rows, maxCap);
  p.tableBytes = (uint64_t(K) * nb + nb + (hasInit ? nb : 0)) * 8 + uint64_t(nb) * 4;
  p.partialWords = p.passes.partialBytes / 4;
  p.densePtrs = p.sizes = p.denseOk = p.rows;
  p.verdict = 2 * uint64_t(nb);
  p.firstN = nb;
  auto granules = [](uint64_t bytes) { return std::max<uint64_t>((bytes + 255) / 256, 1) * 256; };
  p.scratchBytes = granules(p.tableBytes) + granules(4 * p.partialWords) + granules(8 * p.densePtrs) +
                   granules(4 * p.sizes) + granules(p.denseOk) + granules(p.d.listBytes) +
                   granules(4 * p.d.chunkPre) + granules(4 * p.d.blockTot) + granules(p.verdict) +
                   granules(4 * p.firstN);
  return p;
}

// ---------------------------------------------------------------------------
// range decode: words [first[i], first[i] + count[i]) of the archive at in[i]
// ---------------------------------------------------------------------------
struct SparseRangePlan {
  // the host columns (SparseRangeTabs): per distinct archive its address and
  // where its counts live, per member its archive's slot and `first`
  std::vector<uint64_t> archPtr;    // [nArch], ascending
  std::vector<uint64_t> archInfo;   // [nArch] g0 | chunks << 32: its first counting workgroup, its chunks counted
  std::vector<uint64_t> slotFirst;  // [nb] slot | first << 32
  uint32_t nArch = 0;
  uint64_t totalBlocks = 0;  // counting workgroups of all archives: blockTot entries, chunkPre / 256
  uint32_t maxCblocks = 1;   // ... of the archive with the most
  uint32_t maxCount = 0;     // the largest count among the members that size anything
  uint64_t rowWords = 0;     // words of a scratch row (a list slice: count + 1 words at most)
  uint32_t maxRangeBlocks = 0;  // DecodeCall::maxRangeBlocks of the dense range decode
  uint32_t chunkWaves = 1;   // chunks a range touches at most
  uint32_t expandGridX = 1;  // k_sparseExpandRange workgroups per member
  // element counts of the allocations (at least 1)
  uint64_t chunkPre = 1, blockTot = 1;
  bool tooLarge = false;  // totalBlocks * 256 passes 32 bits: the call is refused
};

// The distinct archives are counted once each, up to the largest range end
// among their members (64 bits: first + count may pass 2^32).  A range that
// ends past 2^32 - 1 words fails whatever N is (the plan kernel refuses it;
// nothing is counted, decoded or expanded for it), so it sizes neither the
// counts nor the scratch rows.  The rows are sized by the call's largest count
// before any N is known: a member whose count cannot be valid but still ends
// below 2^32 makes every row that long.
inline SparseRangePlan planSparseRange(const uint64_t* in, const uint32_t* first, const uint32_t* count,
                                       uint32_t nb) {
  SparseRangePlan p;
  std::vector<uint32_t> order(nb);
  for (uint32_t i = 0; i < nb; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return in[x] < in[y]; });
  std::vector<uint64_t> maxEnd;
  p.slotFirst.resize(nb);
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t i = order[k];
    if (k == 0 || in[i] != p.archPtr.back()) {
      p.archPtr.push_back(in[i]);
      maxEnd.push_back(0);
    }
    p.slotFirst[i] = uint64_t(p.archPtr.size() - 1) | (uint64_t(first[i]) << 32);
    const uint64_t end = uint64_t(first[i]) + count[i];
    if (end > uint64_t(UINT32_MAX)) continue;
    maxEnd.back() = std::max(maxEnd.back(), end);
    p.maxCount = std::max(p.maxCount, count[i]);
  }
  p.nArch = uint32_t(p.archPtr.size());
  p.archInfo.resize(p.nArch);
  for (uint32_t a = 0; a < p.nArch; ++a) {
    const uint64_t chunks = (maxEnd[a] + splan::kChunkWords - 1) / splan::kChunkWords;  // <= 2^22
    const uint32_t cblocks = uint32_t((chunks + splan::kThreads - 1) / splan::kThreads);
    p.archInfo[a] = p.totalBlocks | (chunks << 32);
    p.totalBlocks += cblocks;
    p.maxCblocks = std::max(p.maxCblocks, cblocks);
  }
  // (g0 rides in 32 bits, and the kernels index chunkPre with 256 g0 + t)
  p.tooLarge = p.totalBlocks * splan::kThreads > uint64_t(UINT32_MAX);
  p.chunkPre = std::max<uint64_t>(p.totalBlocks * splan::kThreads, 1);
  p.blockTot = std::max<uint64_t>(p.totalBlocks, 1);
  const uint64_t slice = uint64_t(p.maxCount) + 1;
  p.rowWords = (slice + 15) / 16 * 16 + 16;
  // the slice's start inside a block is not known here, hence one block more
  // (workgroups past a slice's last block return at once); a range's start
  // inside a chunk is arbitrary too
  p.maxRangeBlocks = uint32_t((slice + cplan::kBlockWords - 1) / cplan::kBlockWords) + 1;
  p.chunkWaves = uint32_t((uint64_t(p.maxCount) + splan::kChunkWords - 1) / splan::kChunkWords) + 1;
  p.expandGridX = splan::div32(p.chunkWaves, splan::kWaves);
  return p;
}

}  // namespace dietgpu
