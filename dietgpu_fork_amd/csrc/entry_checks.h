// The argument checks that more than one entry point makes: the C++ API of
// the dense codecs (codec.hip) and of the sparse codec (sparse.hip), and the C
// ABI (capi.cpp), which repeats the ones that must refuse a call before the
// stack or any pointer is looked at.  Host only.
#pragma once

#include <cstdint>

#include "common.h"
#include "decode_plan.h"
#include "dietgpu/GpuFloatCodec.h"

namespace dietgpu {

inline void checkProbBits(int pb) {
  DG_CHECK(pb >= 9 && pb <= 11, "unhandled pdf precision " << pb << " (must be 9, 10 or 11)");
}

inline void checkFloatConfig(const FloatCodecConfig& c) {
  DG_CHECK(!c.ansConfig.useChecksum,
           "ANS-level checksumming is not allowed in float mode (use FloatCodecConfig.useChecksum)");
  DG_CHECK(c.floatType != FloatType::kUndefined && uint32_t(c.floatType) <= 4, "bad float type");
}

// The forms that decode part of an element, or add it to something: none can
// verify the archive's checksum, and a config that asks for it is refused.
enum class PartialDecode { kRange, kGather, kAccumulate, kReduce, kGatherSum };

inline void checkNoChecksum(bool useChecksum, PartialDecode what) {
  switch (what) {
    case PartialDecode::kRange:
      DG_CHECK(!useChecksum, "a range decode cannot verify a checksum (it covers the whole element)");
      break;
    case PartialDecode::kGather:
      DG_CHECK(!useChecksum, "a row gather cannot verify a checksum (it covers the whole element)");
      break;
    case PartialDecode::kAccumulate:
      DG_CHECK(!useChecksum,
               "a decode-and-accumulate cannot verify a checksum (the accumulator no longer holds the decoded "
               "words)");
      break;
    case PartialDecode::kReduce:
      DG_CHECK(!useChecksum, "a fused reduce cannot verify a checksum (the decoded words are never stored)");
      break;
    case PartialDecode::kGatherSum:
      DG_CHECK(!useChecksum, "a pooled row gather cannot verify a checksum (the decoded words are never stored)");
      break;
  }
}

// The fused reduce (floatReduceArchives; float types as FloatType's values):
// fp16, bf16 and fp32 archives, 1 .. 64 sources, an init (if any) and an out
// of the archives' type or fp32.  The C ABI makes the same checks before it
// looks at the stack or any pointer.
inline void checkReduceShape(int floatType, uint32_t numSources, bool hasInit, int initType, int outType) {
  DG_CHECK(floatType >= 1 && floatType <= 3, "a fused reduce takes fp16, bf16 or fp32 archives (float type 1..3), not "
                                                 << floatType);
  DG_CHECK(numSources >= 1 && numSources <= kReduceMaxSources,
           "numSources (" << numSources << ") must be in 1 .. " << kReduceMaxSources);
  DG_CHECK(outType == floatType || outType == 3,
           "out type " << outType << " does not go with float type " << floatType << " (the archives' type, or fp32)");
  DG_CHECK(!hasInit || initType == floatType || initType == 3,
           "init type " << initType << " does not go with float type " << floatType
                        << " (the archives' type, or fp32)");
}

// An accumulator has the archive's own float type, or is fp32 for an fp16 /
// bf16 archive (types as FloatType's values; anything else pairs with nothing).
inline bool accumulatorPairs(int floatType, int accType) {
  return floatType >= 1 && floatType <= 4 && (accType == floatType || (floatType <= 2 && accType == 3));
}

// ... as the C++ API refuses a bad pair, and the form of a good one
inline DecodeForm accumulateForm(FloatType floatType, FloatType accType) {
  DG_CHECK(accumulatorPairs(int(floatType), int(accType)),
           "accumulator type " << int(accType) << " does not go with float type " << int(floatType)
                               << " (the archive's own type, or fp32 for fp16 / bf16 archives)");
  return accType == floatType ? DecodeForm::kAccumulate : DecodeForm::kAccumulateFp32;
}

// ... and as the C ABI does, in its parameters' names
inline void checkAccTypeC(int float_type, int acc_type) {
  DG_CHECK(accumulatorPairs(float_type, acc_type),
           "acc_type " << acc_type << " does not go with float_type " << float_type
                       << " (float_type itself, or 3 for float_type 1 / 2)");
}

// The row shape of a gather: rows of rowWords words, outRowStrideWords apart.
inline void checkGatherRows(uint32_t rowWords, uint64_t outRowStrideWords) {
  DG_CHECK(rowWords >= 1, "rowWords must be at least 1");
  DG_CHECK(outRowStrideWords >= rowWords,
           "outRowStrideWords (" << outRowStrideWords << ") must be at least rowWords (" << rowWords << ")");
}

// The pooled row gather (floatGatherRowsSum; float types as FloatType's
// values): fp16, bf16 and fp32 archives, an out of the archive's type or fp32.
// The C ABI makes the same checks before it looks at the stack or any pointer.
inline void checkGatherSumShape(int floatType, bool outIsFp32, uint32_t rowWords, uint64_t outRowStrideWords) {
  DG_CHECK(floatType >= 1 && floatType <= 3,
           "a pooled row gather takes fp16, bf16 or fp32 archives (float type 1..3), not " << floatType);
  DG_CHECK(outIsFp32 || floatType != 3, "the pooled rows of an fp32 archive are fp32 (outIsFp32 must be set)");
  checkGatherRows(rowWords, outRowStrideWords);
}

}  // namespace dietgpu
