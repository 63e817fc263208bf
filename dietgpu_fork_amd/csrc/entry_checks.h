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
enum class PartialDecode { kRange, kGather, kAccumulate, kReduce, kGatherSum, kMatmul };

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
    case PartialDecode::kMatmul:
      DG_CHECK(!useChecksum, "a compressed matmul cannot verify a checksum (the decoded words are never stored)");
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

// The pooling mode and the per-sample weights of floatGatherRowsPool (mode as
// PoolMode's values; weightType 0 for none, else as FloatType's values); its
// archive and row shape are checkGatherSumShape's.  The C ABI makes the same
// checks before it looks at the stack or any pointer.
inline void checkGatherPoolMode(int floatType, int mode, int weightType) {
  DG_CHECK(mode >= 0 && mode <= 2, "unknown pooling mode " << mode << " (0 sum, 1 mean, 2 max)");
  DG_CHECK(weightType == 0 || mode == 0,
           "per-sample weights go with mode sum alone, not with " << (mode == 1 ? "mean" : "max"));
  DG_CHECK(weightType == 0 || weightType == 3 || (weightType == floatType && floatType <= 2),
           "weight type " << weightType << " does not go with float type " << floatType
                          << " (fp32, or the archive's type)");
}

// The matmul on a compressed table (floatMatmulRows; float types as
// FloatType's values): fp16, bf16 and fp32 archives, an out of the archive's
// type or fp32, rows of a multiple of 256 words, 1 .. 64 activation rows at a
// stride of whole 16 B.  The C ABI makes the same checks before it looks at the
// stack or any pointer.
inline void checkMatmulShape(int floatType, bool outIsFp32, uint32_t rowWords, uint32_t numRows, uint32_t M,
                             uint64_t xRowStrideWords, uint64_t outRowStrideWords) {
  DG_CHECK(floatType >= 1 && floatType <= 3,
           "a compressed matmul takes fp16, bf16 or fp32 archives (float type 1..3), not " << floatType);
  DG_CHECK(outIsFp32 || floatType != 3, "the products of an fp32 archive are fp32 (outIsFp32 must be set)");
  DG_CHECK(rowWords >= 1 && rowWords % kMatmulSegWords == 0,
           "rowWords (" << rowWords << ") must be a positive multiple of " << kMatmulSegWords
                        << " (pad the rows with zeros)");
  DG_CHECK(M >= 1 && M <= kMatmulMaxRows, "M (" << M << ") must be in 1 .. " << kMatmulMaxRows
                                                << " (for more activation rows, decompress and call a GEMM)");
  DG_CHECK(numRows >= 1, "numRows must be at least 1");
  DG_CHECK(uint64_t(numRows) * rowWords < (1ull << 32),
           "numRows (" << numRows << ") times rowWords (" << rowWords << ") must be below 2^32");
  DG_CHECK(xRowStrideWords >= rowWords,
           "xRowStrideWords (" << xRowStrideWords << ") must be at least rowWords (" << rowWords << ")");
  DG_CHECK(xRowStrideWords * (floatType == 3 ? 4 : 2) % 16 == 0,
           "xRowStrideWords (" << xRowStrideWords << ") must be a whole number of 16 B");
  DG_CHECK(outRowStrideWords >= numRows,
           "outRowStrideWords (" << outRowStrideWords << ") must be at least numRows (" << numRows << ")");
}

// The matmul on a sparse archive (floatMatmulSparseRows) takes checkMatmulShape
// and a capacity for the decoded nonzero list, which sizes its scratch.  The C
// ABI makes the same checks before it looks at the stack or any pointer.
inline void checkSparseListCapacity(uint32_t listCapacityWords) {
  DG_CHECK(listCapacityWords >= 1 && listCapacityWords < UINT32_MAX - 32,
           "listCapacityWords (" << listCapacityWords << ") must be in 1 .. 2^32 - 34 (the words of the archive's "
                                 "nonzero list, or a bound on them)");
}

// The matmul through the matrix pipe (floatMatmulTile): fp16 and bf16 archives
// alone, each other type with its own message; everything else is
// checkMatmulShape's.  The C ABI makes the same checks before it looks at the
// stack or any pointer.
inline void checkMatmulTileShape(int floatType, bool outIsFp32, uint32_t rowWords, uint32_t numRows, uint32_t M,
                                 uint64_t xRowStrideWords, uint64_t outRowStrideWords) {
  DG_CHECK(floatType != 3, "a tiled matmul multiplies 16-bit words (float type 1 or 2); matmul_rows is the path of "
                           "an fp32 archive");
  DG_CHECK(floatType != 4, "a tiled matmul takes fp16 or bf16 archives (float type 1 or 2), not fp64");
  DG_CHECK(floatType == 1 || floatType == 2,
           "a tiled matmul takes fp16 or bf16 archives (float type 1 or 2), not " << floatType);
  checkMatmulShape(floatType, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords);
}

// The matmul on a sparse archive through the matrix pipe
// (floatMatmulSparseTile): fp16 and bf16 archives alone, each other type with
// its own message; then checkMatmulShape and checkSparseListCapacity.  The C
// ABI makes the same checks before it looks at the stack or any pointer.
inline void checkMatmulSparseTileShape(int floatType, bool outIsFp32, uint32_t rowWords, uint32_t numRows, uint32_t M,
                                       uint64_t xRowStrideWords, uint64_t outRowStrideWords,
                                       uint32_t listCapacityWords) {
  DG_CHECK(floatType != 3, "a tiled sparse matmul multiplies 16-bit words (float type 1 or 2); matmul_sparse is the "
                           "path of an fp32 archive");
  DG_CHECK(floatType != 4, "a tiled sparse matmul takes fp16 or bf16 archives (float type 1 or 2), not fp64");
  DG_CHECK(floatType == 1 || floatType == 2,
           "a tiled sparse matmul takes fp16 or bf16 archives (float type 1 or 2), not " << floatType);
  checkMatmulShape(floatType, outIsFp32, rowWords, numRows, M, xRowStrideWords, outRowStrideWords);
  checkSparseListCapacity(listCapacityWords);
}

// The grouped matmul (floatMatmulGrouped): checkMatmulTileShape's refusals for
// one table first (any number of rows T: an expert's rows go 64 at a time),
// then 1 .. 1024 experts, T >= 1 and partials that 32-bit indices reach.  The C
// ABI makes the same checks before it looks at the stack or any pointer.
inline void checkMatmulGroupedShape(int floatType, bool outIsFp32, uint32_t rowWords, uint32_t numRows,
                                    uint32_t numExperts, uint32_t T, uint64_t xRowStrideWords,
                                    uint64_t outRowStrideWords) {
  checkMatmulTileShape(floatType, outIsFp32, rowWords, numRows, 1, xRowStrideWords, outRowStrideWords);
  DG_CHECK(numExperts >= 1 && numExperts <= kMatmulGroupMaxExperts,
           "numExperts (" << numExperts << ") must be in 1 .. " << kMatmulGroupMaxExperts);
  DG_CHECK(T >= 1, "T must be at least 1 (x holds no row)");
  DG_CHECK(planMatmulGrouped(numExperts, numRows, rowWords, T, 1, 0).valid,
           "T (" << T << ") rows of numRows + blocks partial sums each must stay below 2^32 words");
}

}  // namespace dietgpu
