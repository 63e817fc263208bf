// The grid rule of k_decode (decode.h): how many workgroups a decode call
// launches per element, how many chunks each of them decodes, and whether
// their waves run with remaining-work priorities.  Host only and free of HIP
// headers, so that the rule -- performance policy, DESIGN.md 5.2 -- is stated
// once and tested without a GPU (tests/test_decode_plan.py).  Below it the
// grid rule of k_gather (gather.h; tests/test_gather_plan.py), that of
// k_gatherSum (gather_sum.h; tests/test_gather_sum_plan.py), the pass and grid
// rule of k_matmulRows (matmul.h) and the pass and grid rules of k_reduce
// (reduce.h; tests/test_reduce_plan.py).
#pragma once

#include <algorithm>
#include <cstdint>

namespace dietgpu {

// What a decode call does with the words it decodes.
enum class DecodeForm : uint8_t {
  kFull,            // every word of the element, stored
  kRange,           // words [first, first + count), stored
  kAccumulate,      // every word, added to the destination in the archive's type (5.2d)
  kAccumulateFp32,  // ... of an fp16 / bf16 archive, added to an fp32 destination
};

struct DecodePlan {
  uint32_t gridX;        // workgroups per element
  uint32_t chunksPerWG;  // P: chunks (of blocksPerWG blocks) a workgroup decodes
  bool balance;          // remaining-work wave priorities (k_decode's BAL)
};

// P is capped: large batches then run several generations of workgroups,
// which measured faster than long persistent loops (c3: 3.02 ms at P = 64,
// 2.31 ms at P = 8, 2.60 ms at P = 1; c2's P = 2 is unaffected).
constexpr uint32_t kMaxDecodeChunks = 8;

// The plan of one grid slice of ny elements.  maxBlocks: the most 4096-word
// blocks a member decodes (for a range: that its range touches).  slots: the
// workgroups of the launched kernel resident on the device at once (unused
// for a range).
inline DecodePlan planDecode(DecodeForm form, bool capacityOnly, uint32_t maxBlocks, uint32_t blocksPerWG,
                             uint32_t ny, uint32_t slots) {
  const uint32_t chunks = std::max(1u, (maxBlocks + blocksPerWG - 1) / blocksPerWG);
  // A range is short: one chunk per workgroup, so that its chunks run side by
  // side.  So is a capacityOnly call, where the capacity is all the host
  // knows and may far exceed the archives' sizes (the sparse codec's nonzero
  // lists): the chunks that exist run side by side instead of P passes of a
  // workgroup while the grid's upper part exits at once (5 x 15M fp32 at 50 %
  // zeros: the list decode 77 -> see DESIGN).  An accumulate call knows its
  // sizes and ignores the flag.  Otherwise about one generation of resident
  // workgroups, each decoding P chunks (one table build per P chunks).
  const bool full = form == DecodeForm::kFull;
  uint32_t P = 1;
  if (form != DecodeForm::kRange && !(full && capacityOnly))
    P = std::min(kMaxDecodeChunks, std::max(1u, uint32_t((uint64_t(chunks) * ny + slots / 2) / slots)));
  const uint32_t gridX = (chunks + P - 1) / P;
  // remaining-work wave priorities balance the finish of a single generation
  // (c2 decode -2 %); across several generations they cost (c3 decode 2.02 ms
  // without, 2.32 ms with, same-box A/B).  Full decodes only.
  return {gridX, P, full && uint64_t(gridX) * ny <= slots};
}

// The grid rule of k_gather (gather.h): rows of rowWords words
// of one element, each named by an index in device memory.
struct GatherPlan {
  bool valid;       // rowWords >= 1 and numIdx * K < 2^32
  uint32_t K;       // tasks per index: the most 4096-word blocks a row touches
  uint32_t groups;  // task groups (of kGatherTasksPerWG tasks)
  uint32_t gridX;   // persistent workgroups; 0: nothing to launch
};

// a workgroup's 4 waves take a task per half-wave
constexpr uint32_t kGatherTasksPerWG = 8;

// A row that starts at word s touches divUp(s % 4096 + rowWords, 4096) blocks;
// every start is a multiple of g = gcd(rowWords, 4096), so s % 4096 is at
// most 4096 - g and some row attains K = divUp(4096 - g + rowWords, 4096).
inline uint32_t gatherBlocksPerRow(uint32_t rowWords) {
  uint64_t a = rowWords, b = 4096;
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return uint32_t((4096 - a + rowWords + 4095) / 4096);
}

// slots: the workgroups of the launched instance resident on the device at
// once.  One generation of them strides over the task groups, so that each
// builds the decode table once.
inline GatherPlan planGather(uint32_t numIdx, uint32_t rowWords, uint32_t slots) {
  if (rowWords == 0) return {false, 0, 0, 0};
  const uint32_t K = gatherBlocksPerRow(rowWords);
  const uint64_t tasks = uint64_t(numIdx) * K;
  if (tasks >= (1ull << 32)) return {false, K, 0, 0};
  const uint32_t groups = uint32_t((tasks + kGatherTasksPerWG - 1) / kGatherTasksPerWG);
  return {true, K, groups, std::min(std::max(1u, slots), groups)};
}

// The grid rule of k_gatherSum (gather_sum.h, DESIGN.md 5.2i;
// tests/test_gather_sum_plan.py): numBags bags of rows of rowWords words, each
// summed into one output row.  A task is a (bag, column tile) pair; a
// half-wave keeps a tile's running sum in registers, a column per lane and
// register, so the tile is 32 lanes x 4 registers wide and a wider row becomes
// several tasks (each decodes the row's blocks again).  4 registers, not 8:
// at 256 columns the kernel took 78 VGPRs, 6 workgroups per CU; at 128 it
// takes 60 and keeps k_decode's 8.
constexpr uint32_t kGatherSumTile = 128;

struct GatherSumPlan {
  bool valid;          // rowWords >= 1 and numBags * tiles < 2^32
  uint32_t tileWords;  // kGatherSumTile
  uint32_t tiles;      // column tiles (tasks) per bag
  uint64_t tasks;      // numBags * tiles
  uint32_t groups;     // task groups (of kGatherTasksPerWG tasks)
  uint32_t gridX;      // persistent workgroups; 0: nothing to launch
};

// slots: as planGather's.
inline GatherSumPlan planGatherSum(uint32_t numBags, uint32_t rowWords, uint32_t slots) {
  if (rowWords == 0) return {false, kGatherSumTile, 0, 0, 0, 0};
  const uint32_t tiles = uint32_t((uint64_t(rowWords) + kGatherSumTile - 1) / kGatherSumTile);
  const uint64_t tasks = uint64_t(numBags) * tiles;
  if (tasks >= (1ull << 32)) return {false, kGatherSumTile, tiles, tasks, 0, 0};
  const uint32_t groups = uint32_t((tasks + kGatherTasksPerWG - 1) / kGatherTasksPerWG);
  return {true, kGatherSumTile, tiles, tasks, groups, std::min(std::max(1u, slots), groups)};
}

// The pass and grid rule of the matmul on a compressed table (k_matmulRows,
// matmul.h): M activation rows against the R rows of rowWords
// words that one archive holds.  A task is a 4096-word block of the table; a
// pass takes at most rowsPerPass activation rows through all of them.  The rows
// go to the passes in order, evenly, as planReduce deals its sources.  Every
// (block, row) piece of a pass leaves one fp32 partial per activation row at
// id block + row, so a pass needs pieces = R + nBlocks words per row; the next
// pass reuses them.
constexpr uint32_t kMatmulSegWords = 256;   // dec::kSegWords: rowWords is a multiple of it
constexpr uint32_t kMatmulMaxRows = 64;     // more activation rows than this is a GEMM
constexpr uint32_t kMatmulRowsPerPass = 4;  // the largest k_matmulRows instance kept

struct MatmulPass {
  uint32_t first, count;  // activation rows [first, first + count)
};

struct MatmulPlan {
  bool valid;  // rowWords a positive multiple of 256, 1 <= M <= 64, R >= 1, R * rowWords < 2^32, rowsPerPass >= 1
  uint32_t numPasses;
  MatmulPass passes[kMatmulMaxRows];
  uint32_t nBlocks;       // 4096-word blocks that hold words of the table: the tasks
  uint32_t pieces;        // R + nBlocks: partial words per activation row
  uint64_t partialBytes;  // of one pass (the largest, which is the first)
  uint32_t groups;        // task groups (of kGatherTasksPerWG tasks)
  uint32_t gridX;         // persistent workgroups
};

// slots: as planGather's.
inline MatmulPlan planMatmul(uint32_t numRows, uint32_t rowWords, uint32_t M, uint32_t rowsPerPass, uint32_t slots) {
  MatmulPlan p{};
  const uint64_t words = uint64_t(numRows) * rowWords;
  p.valid = rowWords >= 1 && rowWords % kMatmulSegWords == 0 && M >= 1 && M <= kMatmulMaxRows && numRows >= 1 &&
            words < (1ull << 32) && rowsPerPass >= 1;
  if (!p.valid) return p;
  p.numPasses = (M + rowsPerPass - 1) / rowsPerPass;
  uint32_t first = 0;
  for (uint32_t i = 0; i < p.numPasses; ++i) {
    const uint32_t count = M / p.numPasses + (i < M % p.numPasses ? 1 : 0);
    p.passes[i] = {first, count};
    first += count;
  }
  p.nBlocks = uint32_t((words + 4095) / 4096);
  p.pieces = numRows + p.nBlocks;
  p.partialBytes = 4ull * p.passes[0].count * p.pieces;
  p.groups = (p.nBlocks + kGatherTasksPerWG - 1) / kGatherTasksPerWG;
  p.gridX = std::min(std::max(1u, slots), p.groups);
  return p;
}

// The task and grid rule of the matmul through the matrix pipe (k_matmulTile,
// matmul_tile.h): all M <= 64 activation rows in one pass.  A
// workgroup's eight half-waves take blocks `period` apart, period the least
// count of 4096-word blocks that is a whole number of rows: such blocks start
// at the same column of their rows.  The block line is tiled in runs of
// 8 * period blocks, each run `period` task groups; a group whose first block
// lies past the table is skipped.  The pieces are planMatmul's, one set per
// activation row.
struct MatmulTilePlan {
  bool valid;             // planMatmul's rule
  uint32_t period;        // (rowWords / 256) / gcd(rowWords / 256, 16)
  uint32_t nBlocks;       // 4096-word blocks that hold words of the table
  uint32_t pieces;        // R + nBlocks: partial words per activation row
  uint64_t partialBytes;  // 4 * M * pieces
  uint32_t groups;        // task groups: ceil(nBlocks / (8 * period)) * period
  uint32_t gridX;         // persistent workgroups
};

// slots: as planGather's.
inline MatmulTilePlan planMatmulTile(uint32_t numRows, uint32_t rowWords, uint32_t M, uint32_t slots) {
  MatmulTilePlan p{};
  const uint64_t words = uint64_t(numRows) * rowWords;
  p.valid = rowWords >= 1 && rowWords % kMatmulSegWords == 0 && M >= 1 && M <= kMatmulMaxRows && numRows >= 1 &&
            words < (1ull << 32);
  if (!p.valid) return p;
  const uint32_t segs = rowWords / kMatmulSegWords;
  uint32_t a = segs, b = 4096 / kMatmulSegWords;
  while (b) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  p.period = segs / a;
  p.nBlocks = uint32_t((words + 4095) / 4096);
  p.pieces = numRows + p.nBlocks;
  p.partialBytes = 4ull * M * p.pieces;
  const uint64_t run = uint64_t(kGatherTasksPerWG) * p.period;
  p.groups = uint32_t((p.nBlocks + run - 1) / run * p.period);
  p.gridX = std::min(std::max(1u, slots), p.groups);
  return p;
}

// The scratch and grid rule of the grouped matmul (matmul_grouped.h; DESIGN.md
// 5.2l): E tables of numRows x rowWords words, T activation rows dealt to them
// by offsets that only the device knows.  An entry is an expert's next <= 64
// rows, so there are at most E + T / 64 of them; the task line is entries x
// groups, groups and period planMatmulTile's for one table, and the grid is
// sized by the bound.  The scratch holds, each 16 B-aligned: the head words,
// one status byte per expert, the entry list (16 B each) and 4 * T * pieces
// bytes of partials.
constexpr uint32_t kMatmulGroupMaxExperts = 1024;  // four thread rounds of k_matmulGroupPlan's one workgroup

struct MatmulGroupedPlan {
  bool valid;  // planMatmulTile's rule for one table, 1 <= E <= 1024, T >= 1, T * pieces and the task bound < 2^32
  uint32_t period, groups, pieces;  // planMatmulTile's
  uint32_t entryBound;              // E + T / 64
  uint64_t statusOffset, entriesOffset, partOffset;  // bytes into the scratch; the head is at 0
  uint64_t partialBytes;            // the whole scratch
  uint32_t gridX;                   // persistent workgroups of k_matmulTileGrouped
};

// slots: as planGather's.  gridCap: dietgpu_set_matmul_grouped_grid (0: none).
inline MatmulGroupedPlan planMatmulGrouped(uint32_t E, uint32_t numRows, uint32_t rowWords, uint32_t T, uint32_t slots,
                                           uint32_t gridCap) {
  MatmulGroupedPlan p{};
  const MatmulTilePlan one = planMatmulTile(numRows, rowWords, 1, 1);
  if (!one.valid || E < 1 || E > kMatmulGroupMaxExperts || T < 1) return p;
  p.period = one.period;
  p.groups = one.groups;
  p.pieces = one.pieces;
  p.entryBound = E + T / kMatmulMaxRows;
  const uint64_t tasks = uint64_t(p.entryBound) * p.groups;
  if (uint64_t(T) * p.pieces >= (1ull << 32) || tasks >= (1ull << 32)) return p;
  p.valid = true;
  auto up16 = [](uint64_t v) { return (v + 15) / 16 * 16; };
  p.statusOffset = 16;
  p.entriesOffset = p.statusOffset + up16(E);
  p.partOffset = p.entriesOffset + 16ull * p.entryBound;
  p.partialBytes = p.partOffset + 4ull * T * p.pieces;
  p.gridX = uint32_t(std::min<uint64_t>(std::max(1u, slots), tasks));
  if (gridCap) p.gridX = std::min(p.gridX, gridCap);
  return p;
}

// The pass rule of the fused reduce (k_reduce, reduce.h; DESIGN.md 5.2g;
// tests/test_reduce_plan.py): K sources, at most nsMax per launch.  The
// sources go to the passes in order, evenly (the larger passes first: fewer
// sources per launch leave more workgroups resident); every pass but the last
// writes an fp32 partial that the next one reads as its init, so the order of
// the adds, and with it every bit, is that of one pass over all K.
constexpr uint32_t kReduceMaxSources = 64;

struct ReducePass {
  uint32_t first, count;  // sources [first, first + count)
  bool initIsPartial;     // reads the partial (else the caller's init, if any)
  bool outIsPartial;      // writes the partial (else the caller's out)
};

struct ReducePlan {
  bool valid;  // 1 <= K <= kReduceMaxSources, nsMax >= 1
  uint32_t numPasses;
  ReducePass passes[kReduceMaxSources];
  uint64_t partialBytes;  // fp32 words of every member's capacity, each padded to 4; 0 for one pass
};

// partialWords: the sum over the members of their capacity rounded up to 4
// words (a member's partial starts 16 B-aligned).
inline ReducePlan planReduce(uint32_t K, uint32_t nsMax, uint64_t partialWords) {
  ReducePlan p{};
  p.valid = K >= 1 && K <= kReduceMaxSources && nsMax >= 1;
  if (!p.valid) return p;
  p.numPasses = (K + nsMax - 1) / nsMax;
  uint32_t first = 0;
  for (uint32_t i = 0; i < p.numPasses; ++i) {
    const uint32_t count = K / p.numPasses + (i < K % p.numPasses ? 1 : 0);
    p.passes[i] = {first, count, i > 0, i + 1 < p.numPasses};
    first += count;
  }
  p.partialBytes = p.numPasses > 1 ? 4 * partialWords : 0;
  return p;
}

// The grid of one pass over a slice of ny members: k_decode's accumulate rule
// on the resident workgroups of the k_reduce instance launched.
inline DecodePlan planReduceGrid(uint32_t maxBlocks, uint32_t blocksPerWG, uint32_t ny, uint32_t slots) {
  return planDecode(DecodeForm::kAccumulate, false, maxBlocks, blocksPerWG, ny, std::max(1u, slots));
}

}  // namespace dietgpu
