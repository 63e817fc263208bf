// Host check of k_decode's grid rule (dietgpu_fork_amd/csrc/decode_plan.h),
// built by tests/test_decode_plan.py with a plain C++ compiler: literal
// anchors from DESIGN.md, then a sweep against the three formulas the decode
// launchers used before the rule had a function of its own.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "decode_plan.h"

using dietgpu::DecodeForm;
using dietgpu::DecodePlan;
using dietgpu::planDecode;

static uint32_t divUp(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// the full decode's launcher
static DecodePlan refFull(bool capacityOnly, uint32_t maxBlocks, uint32_t bpw, uint32_t ny, uint32_t slots) {
  const uint32_t chunks = std::max(1u, divUp(maxBlocks, bpw));
  const uint32_t P =
      capacityOnly ? 1u : std::min(8u, std::max(1u, uint32_t((uint64_t(chunks) * ny + slots / 2) / slots)));
  const uint32_t gx = divUp(chunks, P);
  return {gx, P, uint64_t(gx) * ny <= slots};
}

// the range decode's launcher
static DecodePlan refRange(uint32_t maxRangeBlocks, uint32_t bpw) {
  return {std::max(1u, divUp(maxRangeBlocks, bpw)), 1u, false};
}

// the accumulate launcher (either accumulator type)
static DecodePlan refAccumulate(uint32_t maxBlocks, uint32_t bpw, uint32_t ny, uint32_t slots) {
  const uint32_t chunks = std::max(1u, divUp(maxBlocks, bpw));
  const uint32_t P = std::min(8u, std::max(1u, uint32_t((uint64_t(chunks) * ny + slots / 2) / slots)));
  return {divUp(chunks, P), P, false};
}

static int failures = 0;

static void expect(const char* what, DecodePlan got, DecodePlan want) {
  if (got.gridX == want.gridX && got.chunksPerWG == want.chunksPerWG && got.balance == want.balance) return;
  ++failures;
  std::printf("FAIL %s: got {%u, %u, %d}, expected {%u, %u, %d}\n", what, got.gridX, got.chunksPerWG,
              int(got.balance), want.gridX, want.chunksPerWG, int(want.balance));
}

int main() {
  const uint32_t S = 2048, W = 8;  // resident slots, blocks per workgroup
  expect("c2 full", planDecode(DecodeForm::kFull, false, 128, W, 256, S), {8, 2, true});
  expect("c3 full", planDecode(DecodeForm::kFull, false, 1024, W, 1024, S), {16, 8, false});
  expect("one block full", planDecode(DecodeForm::kFull, false, 1, W, 1, S), {1, 1, true});
  expect("c2 capacityOnly", planDecode(DecodeForm::kFull, true, 128, W, 256, S), {16, 1, false});
  expect("range 9 blocks", planDecode(DecodeForm::kRange, false, 9, W, 256, S), {2, 1, false});
  expect("range 0 blocks", planDecode(DecodeForm::kRange, false, 0, W, 256, S), {1, 1, false});
  expect("c2 accumulate", planDecode(DecodeForm::kAccumulate, false, 128, W, 256, S), {8, 2, false});
  // 2^17 chunks x 2^15 elements = 2^32 exactly: 32-bit products would wrap to
  // 0 and give P = 1, or a balanced capacityOnly grid
  expect("2^32 chunks full", planDecode(DecodeForm::kFull, false, 1u << 20, W, 32768, S), {16384, 8, false});
  expect("2^32 chunks capacityOnly", planDecode(DecodeForm::kFull, true, 1u << 20, W, 32768, S),
         {131072, 1, false});

  const uint32_t blocks[] = {0, 1, 7, 8, 9, 63, 64, 65, 1024, 16384, 1u << 20};
  const uint32_t nys[] = {1, 3, 255, 256, 257, 1024, 65535};
  const uint32_t slotCounts[] = {1, 1024, 1792, 2048};
  const DecodeForm forms[] = {DecodeForm::kFull, DecodeForm::kRange, DecodeForm::kAccumulate,
                              DecodeForm::kAccumulateFp32};
  unsigned cases = 0;
  for (uint32_t mb : blocks)
    for (uint32_t ny : nys)
      for (uint32_t slots : slotCounts)
        for (int co = 0; co < 2; ++co)
          for (DecodeForm f : forms) {
            const DecodePlan want = f == DecodeForm::kFull    ? refFull(co != 0, mb, W, ny, slots)
                                    : f == DecodeForm::kRange ? refRange(mb, W)
                                                              : refAccumulate(mb, W, ny, slots);
            char what[96];
            std::snprintf(what, sizeof what, "form %d capacityOnly %d maxBlocks %u ny %u slots %u", int(f), co, mb,
                          ny, slots);
            expect(what, planDecode(f, co != 0, mb, W, ny, slots), want);
            ++cases;
          }
  std::printf("%u sweep cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
