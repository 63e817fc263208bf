// The grid rule of k_decode (decode.h): how many workgroups a decode call
// launches per element, how many chunks each of them decodes, and whether
// their waves run with remaining-work priorities.  Host only and free of HIP
// headers, so that the rule -- performance policy, DESIGN.md 5.2 -- is stated
// once and tested without a GPU (tests/test_decode_plan.py).  Below it the
// grid rule of k_gather (gather.h; tests/test_gather_plan.py).
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

}  // namespace dietgpu
