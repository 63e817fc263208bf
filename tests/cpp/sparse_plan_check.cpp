// Host-only check of the sparse drivers' arithmetic (csrc/sparse_plan.h):
//   g++ -std=c++17 -Wall -Werror -I dietgpu_fork_amd/csrc tests/cpp/sparse_plan_check.cpp
// The formulas of sparseCompressT, sparseDecompressT and sparseRangeT as they
// stood inline in sparse.hip before the plans (32-bit divUp / roundUp of
// common.h included) are restated here and swept against planSparseCompress,
// planSparseDecode and planSparseRange; a range plan is also checked by brute
// force, member by member and archive by archive.  No HIP, no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "sparse_plan.h"

using namespace dietgpu;

static long gCases = 0, gFailures = 0;

#define EXPECT(c)                                                                        \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      if (++gFailures <= 20) std::printf("%s:%d: %s: %s\n", __FILE__, __LINE__, gWhat, #c); \
    }                                                                                    \
  } while (0)
static char gWhat[160];

// common.h's helpers, 32-bit
static uint32_t divUp(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
static uint32_t roundUp(uint32_t a, uint32_t b) { return divUp(a, b) * b; }

constexpr uint32_t kTileWords = 4096, kChunkWords = 1024, kThreads = 256, kWaves = 4, kBlockSize = 4096;
constexpr uint32_t kNumSymbols = 256, kRows = 64;  // kReduceRows

static const uint32_t kSizes[] = {0,          1,           1023,        1024, 1025, 4095, 4096, 4097, 64 * 4096,
                                  64 * 4096 + 1, (1u << 22) * 1024 - 1, UINT32_MAX};
static const uint32_t kBatches[] = {1, 2, 5, 65536};

static void compressCase(int ft, uint32_t nb, uint32_t maxN, bool denseSinglePass) {
  ++gCases;
  const uint32_t ws = ft <= 2 ? 2 : ft == 3 ? 4 : 8;
  const int kSegs = ft == 4 ? 2 : 1;
  std::snprintf(gWhat, sizeof gWhat, "compress ft=%d nb=%u maxN=%u single=%d", ft, nb, maxN, int(denseSinglePass));
  const SparseCompressPlan p = planSparseCompress(kSegs, ws, nb, maxN, denseSinglePass);
  // sparseCompressT
  const uint32_t tiles = std::max(1u, divUp(maxN, kTileWords));
  const uint64_t listStride = uint64_t(roundUp(maxN, 16) + 16) * ws;
  const bool countHist = nb == 1 && !denseSinglePass;
  const uint32_t R = std::min(tiles, kRows);
  const uint64_t rowsBytes = countHist ? uint64_t(kSegs) * nb * R * kNumSymbols * 4 : 0;
  EXPECT(p.tiles == tiles && p.rows == R && p.countHist == countHist && p.rowsBytes == rowsBytes);
  EXPECT(p.tileCounts == uint64_t(nb) * tiles);
  EXPECT(p.staging == uint64_t(nb) * tiles * (kTileWords + 1));
  EXPECT(p.listStride == listStride && p.listBytes == uint64_t(nb) * listStride);
  EXPECT(p.tableEntries == (countHist ? uint64_t(kSegs) * nb * kNumSymbols : 1));
  // sizing: a row holds every word plus the quirk's slot, in whole 16 B
  // vectors (where the size does not wrap 32 bits)
  if (maxN <= UINT32_MAX - 32) EXPECT(p.listStride % 16 == 0 && p.listStride >= (uint64_t(maxN) + 1) * ws);
  if (maxN <= UINT32_MAX - kTileWords) EXPECT(uint64_t(p.tiles) * kTileWords >= maxN && p.rows >= 1 && p.rows <= 64);
}

static void decodeCase(int ft, uint32_t nb, uint32_t maxCap) {
  ++gCases;
  const uint32_t ws = ft <= 2 ? 2 : ft == 3 ? 4 : 8;
  std::snprintf(gWhat, sizeof gWhat, "decode ft=%d nb=%u maxCap=%u", ft, nb, maxCap);
  const SparseDecodePlan p = planSparseDecode(ws, nb, maxCap);
  // sparseDecompressT
  const uint32_t chunks = std::max(1u, divUp(maxCap, kChunkWords));
  const uint32_t cblocks = divUp(chunks, kThreads);
  const uint64_t listStride = uint64_t(roundUp(maxCap, 16) + 16) * ws;
  EXPECT(p.chunks == chunks && p.cblocks == cblocks && p.gridX == divUp(chunks, kWaves));
  EXPECT(p.denseCapacity == uint32_t(maxCap + 1));
  EXPECT(p.listStride == listStride && p.listBytes == uint64_t(nb) * listStride);
  EXPECT(p.chunkPre == uint64_t(nb) * chunks && p.blockTot == uint64_t(nb) * cblocks);
  if (maxCap <= UINT32_MAX - kChunkWords) {
    EXPECT(uint64_t(p.chunks) * kChunkWords >= maxCap && uint64_t(p.cblocks) * kThreads >= p.chunks);
    EXPECT(uint64_t(p.gridX) * kWaves >= p.chunks && p.listStride >= uint64_t(p.denseCapacity) * ws);
  }
}

struct Members {
  std::vector<uint64_t> in;
  std::vector<uint32_t> first, count;
};

static void rangeCase(const char* what, const Members& m, int expectTooLarge = -1) {
  ++gCases;
  const uint32_t nb = uint32_t(m.in.size());
  std::snprintf(gWhat, sizeof gWhat, "range %s nb=%u", what, nb);
  const SparseRangePlan p = planSparseRange(m.in.data(), m.first.data(), m.count.data(), nb);

  // sparseRangeT, as it stood
  std::vector<uint32_t> order(nb);
  for (uint32_t i = 0; i < nb; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return m.in[x] < m.in[y]; });
  std::vector<uint64_t> archPtr, maxEnd, slotFirst(nb);
  uint32_t maxCount = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t i = order[k];
    if (k == 0 || m.in[i] != archPtr.back()) {
      archPtr.push_back(m.in[i]);
      maxEnd.push_back(0);
    }
    slotFirst[i] = uint64_t(archPtr.size() - 1) | (uint64_t(m.first[i]) << 32);
    const uint64_t end = uint64_t(m.first[i]) + m.count[i];
    if (end > uint64_t(UINT32_MAX)) continue;
    maxEnd.back() = std::max(maxEnd.back(), end);
    maxCount = std::max(maxCount, m.count[i]);
  }
  const uint32_t nArch = uint32_t(archPtr.size());
  std::vector<uint64_t> archInfo(nArch);
  uint64_t totalBlocks = 0;
  uint32_t maxCblocks = 1;
  for (uint32_t a = 0; a < nArch; ++a) {
    const uint64_t chunks = (maxEnd[a] + kChunkWords - 1) / kChunkWords;
    const uint32_t cblocks = uint32_t((chunks + kThreads - 1) / kThreads);
    archInfo[a] = totalBlocks | (chunks << 32);
    totalBlocks += cblocks;
    maxCblocks = std::max(maxCblocks, cblocks);
  }
  const bool tooLarge = !(totalBlocks * kThreads <= uint64_t(UINT32_MAX));
  const uint64_t rowWords = (uint64_t(maxCount) + 1 + 15) / 16 * 16 + 16;
  const uint32_t maxRangeBlocks = uint32_t((uint64_t(maxCount) + 1 + kBlockSize - 1) / kBlockSize) + 1;
  const uint32_t chunkWaves = uint32_t((uint64_t(maxCount) + kChunkWords - 1) / kChunkWords) + 1;
  EXPECT(p.archPtr == archPtr && p.archInfo == archInfo && p.slotFirst == slotFirst);
  EXPECT(p.nArch == nArch && p.totalBlocks == totalBlocks && p.maxCblocks == maxCblocks && p.maxCount == maxCount);
  EXPECT(p.rowWords == rowWords && p.maxRangeBlocks == maxRangeBlocks && p.chunkWaves == chunkWaves);
  EXPECT(p.expandGridX == divUp(chunkWaves, kWaves));
  EXPECT(p.chunkPre == std::max<uint64_t>(totalBlocks * kThreads, 1) && p.blockTot == std::max<uint64_t>(totalBlocks, 1));
  EXPECT(p.tooLarge == tooLarge);
  if (expectTooLarge >= 0) EXPECT(p.tooLarge == (expectTooLarge != 0));

  // brute force: the archives are the distinct addresses, ascending
  const std::set<uint64_t> distinct(m.in.begin(), m.in.end());
  EXPECT(p.archPtr.size() == distinct.size() && p.archInfo.size() == distinct.size() && p.slotFirst.size() == nb);
  EXPECT(std::equal(p.archPtr.begin(), p.archPtr.end(), distinct.begin(), distinct.end()));
  // each member's slot names its archive, and carries its `first`
  uint32_t bruteMaxCount = 0;
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t slot = uint32_t(p.slotFirst[i]);
    EXPECT(slot < p.archPtr.size() && p.archPtr[slot] == m.in[i]);
    EXPECT(uint32_t(p.slotFirst[i] >> 32) == m.first[i]);
    if (uint64_t(m.first[i]) + m.count[i] <= UINT32_MAX) bruteMaxCount = std::max(bruteMaxCount, m.count[i]);
  }
  EXPECT(p.maxCount == bruteMaxCount);
  // g0 is the running sum of the earlier archives' workgroups; the chunks
  // counted follow the largest valid end among the archive's members
  uint64_t run = 0;
  uint32_t most = 1;
  for (size_t a = 0; a < p.archPtr.size(); ++a) {
    uint64_t end = 0;
    for (uint32_t i = 0; i < nb; ++i) {
      const uint64_t e = uint64_t(m.first[i]) + m.count[i];
      if (m.in[i] == p.archPtr[a] && e <= UINT32_MAX) end = std::max(end, e);
    }
    const uint64_t chunks = p.archInfo[a] >> 32;
    EXPECT(uint32_t(p.archInfo[a]) == run);
    EXPECT(chunks * kChunkWords >= end && (chunks == 0 || (chunks - 1) * kChunkWords < end));
    const uint64_t cblocks = (chunks + kThreads - 1) / kThreads;
    run += cblocks;
    most = std::max<uint64_t>(most, cblocks);
  }
  EXPECT(p.totalBlocks == run && p.maxCblocks == most);
  EXPECT(p.tooLarge == (run * kThreads > uint64_t(UINT32_MAX)));
  // sizing: a scratch row holds count + 1 words in whole vectors; the dense
  // range decode and the expander cover a slice / range that starts anywhere
  // inside a block / chunk
  EXPECT(p.rowWords % 16 == 0 && p.rowWords >= uint64_t(bruteMaxCount) + 1 + 16);
  EXPECT(uint64_t(p.maxRangeBlocks - 1) * kBlockSize >= uint64_t(bruteMaxCount) + 1);
  EXPECT(uint64_t(p.chunkWaves - 1) * kChunkWords >= bruteMaxCount);
  EXPECT(uint64_t(p.expandGridX) * kWaves >= p.chunkWaves);
  EXPECT(p.chunkPre >= 1 && p.blockTot >= 1 && p.chunkPre >= p.totalBlocks * kThreads && p.blockTot >= p.totalBlocks);
}

static uint32_t gRng = 12345;
static uint32_t rnd() {
  gRng = gRng * 1664525u + 1013904223u;
  return gRng >> 8;
}

int main() {
  for (int ft = 1; ft <= 4; ++ft)
    for (uint32_t nb : kBatches)
      for (uint32_t n : kSizes) {
        compressCase(ft, nb, n, false);
        compressCase(ft, nb, n, true);
        decodeCase(ft, nb, n);
      }

  // member lists of 1 .. 300: a few archives, repeated, in no order; mixed
  // firsts and counts, count == 0 among them
  for (uint32_t nb = 1; nb <= 300; ++nb) {
    Members m;
    const uint32_t pool = 1 + nb % 7 + (nb > 100 ? nb / 3 : 0);
    for (uint32_t i = 0; i < nb; ++i) {
      m.in.push_back(0x7f0000000000ull + 16ull * ((rnd() % pool) * 2654435761u % 1000003u));
      const uint32_t kind = rnd() % 8;
      const uint32_t first = kind == 0 ? 0 : kind == 1 ? rnd() % 5000 : kind == 2 ? (rnd() << 8) : rnd() % 3000000;
      const uint32_t count = kind == 3 ? 0 : kind == 4 ? 1 : kind == 5 ? rnd() % 300000 : rnd() % 5000;
      m.first.push_back(first);
      m.count.push_back(count);
    }
    rangeCase("mixed", m);
  }
  // the ends around 2^32, alone and beside valid members of the same and of
  // another archive
  const uint64_t A = 0x7f1000000000ull, B = 0x7f1000100000ull;
  const uint32_t M = UINT32_MAX;
  const uint32_t ends[][2] = {{M - 10, 10}, {0, M}, {M, 0},     {M - 10, 11}, {1, M},
                              {M, 1},       {M, M}, {M - 1, M - 1}, {0, 0},       {5, 0}};
  for (const auto& e : ends) {
    rangeCase("end alone", Members{{A}, {e[0]}, {e[1]}});
    rangeCase("end with same archive", Members{{A, A, A}, {100, e[0], 7}, {3000, e[1], 0}});
    rangeCase("end with other archive", Members{{B, A, B}, {100, e[0], 2000}, {3000, e[1], 70000}});
    rangeCase("end with other archive, reversed", Members{{A, B}, {e[0], 0}, {e[1], 1025}});
  }
  // the too-large flag: 1,024 archives read to word 2^32 - 1 take 2^24
  // counting workgroups, i.e. 2^32 chunkPre entries; one workgroup fewer fits
  {
    Members m;
    for (uint32_t i = 0; i < 1024; ++i) {
      m.in.push_back(A + 4096ull * ((i * 7u) % 1024));  // distinct, unsorted
      m.first.push_back(0);
      m.count.push_back(M);
    }
    rangeCase("too large", m, 1);
    m.count[5] = ((1u << 14) - 1) * kThreads * kChunkWords;  // 2^14 - 1 workgroups
    rangeCase("one workgroup short of too large", m, 0);
    m.in.push_back(A + 16);  // one more archive, one more workgroup
    m.first.push_back(0);
    m.count.push_back(1);
    rangeCase("too large again", m, 1);
  }
  std::printf("%ld sparse plan cases, %ld failures\n", gCases, gFailures);
  return gFailures == 0 ? 0 : 1;
}
