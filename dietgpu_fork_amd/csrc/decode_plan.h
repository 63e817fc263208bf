// The grid rule of k_decode (decode.h): how many workgroups a decode call
// launches per element, how many chunks each of them decodes, and whether
// their waves run with remaining-work priorities.  Host only and free of HIP
// headers, so that the rule -- performance policy, DESIGN.md 5.2 -- is stated
// once and tested without a GPU (tests/test_decode_plan.py).  Below it the
// grid rule of k_gather (gather.h; tests/test_gather_plan.py), that of
// k_gatherSum (gather_sum.h; tests/test_gather_sum_plan.py) and the pass and
// grid rules of k_reduce (reduce.h; tests/test_reduce_plan.py).
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
