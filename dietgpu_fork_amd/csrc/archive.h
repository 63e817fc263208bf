// The archive wire format: the one place that knows the byte layout of byte
// (ANS), float and sparse archives.  It restates the reference's format
// (ans/GpuANSUtils.cuh:33-86, float/GpuFloatUtils.cuh:15-19 and 200-391,
// float/GpuSparseFloatCompress.cuh) so that archives are
// interchangeable; every kernel and host function that reads or writes an
// archive goes through the names, layout functions and writers below.
//
//   byte archive    ANS header (32 B) | pdf table | states | block words |
//                   compressed words
//   float archive   float header (32 B) | raw section (one or two planes,
//                   each padded) | ANS archive (fp64: a second one, at float
//                   header word kFloatSecondAns from the first)
//   sparse archive  sparse header (16 B: N, zeros) | bitmap padded to 16 |
//                   float archive of the nonzero list
#pragma once

#include "device.h"

namespace dietgpu {

// ---------------------------------------------------------------------------
// headers: sizes, word indices, flags
// ---------------------------------------------------------------------------
constexpr uint32_t kANSMagicVersion = 0xd00d0001u;
constexpr uint32_t kFloatMagicVersion = 0xf00f0001u;
constexpr uint32_t kANSHeaderBytes = 32;
constexpr uint32_t kFloatHeaderBytes = 32;
constexpr uint32_t kSparseHeaderBytes = 16;
constexpr uint32_t kPdfBytes = 2 * kNumSymbols;
constexpr uint32_t kStateBytesPerBlock = 4 * kLanesPerBlock;

// u32 words of the ANS header
constexpr uint32_t kAnsMagic = 0;
constexpr uint32_t kAnsBlocks = 1;
constexpr uint32_t kAnsSize = 2;        // uncompressed symbols
constexpr uint32_t kAnsTotalWords = 3;  // compressed u16 words, each block's padded to 8
constexpr uint32_t kAnsPrecision = 4;   // probability bits | kChecksumFlag
constexpr uint32_t kAnsChecksum = 5;
constexpr uint32_t kAnsZeros = 6;  // and every word after it
// u32 words of the float header
constexpr uint32_t kFloatMagic = 0;
constexpr uint32_t kFloatSize = 1;       // words
constexpr uint32_t kFloatType = 2;       // float type | kChecksumFlag
constexpr uint32_t kFloatChecksum = 3;
constexpr uint32_t kFloatSecondAns = 4;  // bytes from the first ANS archive to fp64's second
constexpr uint32_t kFloatZeros = 5;      // and every word after it
// u32 words of the sparse header (the rest is zero)
constexpr uint32_t kSparseSize = 0;  // words, zeros included
// words kAnsPrecision and kFloatType
constexpr uint32_t kChecksumFlag = 0x10u;
constexpr uint32_t kTypeMask = 0xfu;  // the float type / the probability bits

// ---------------------------------------------------------------------------
// layout: pure functions of the element's size
// ---------------------------------------------------------------------------
// Symbols of block bk (below the element's block count) of an n-symbol element
__host__ __device__ constexpr uint32_t symbolsOfBlock(uint32_t bk, uint32_t n) {
  const uint32_t left = n - bk * kBlockSize;
  return left < kBlockSize ? left : kBlockSize;
}
// ... or 0 for a block at or past `end` (the element's block count, or the
// end of the blocks a caller works on)
__host__ __device__ constexpr uint32_t blockSymbols(uint32_t bk, uint32_t end, uint32_t n) {
  const uint32_t s = symbolsOfBlock(bk, n);
  return bk < end ? s : 0u;
}

// ANSCoalescedHeader::getCompressedOverhead (ans/GpuANSUtils.cuh:68-86): the
// sections AnsSections lays out, up to the compressed words
__host__ __device__ constexpr uint64_t ansOverhead(uint32_t numBlocks) {
  return kANSHeaderBytes + kPdfBytes + uint64_t(kStateBytesPerBlock) * numBlocks +
      8ull * roundUp(numBlocks, 2);
}
__host__ __device__ constexpr uint64_t ansArchiveBytes(uint32_t numBlocks, uint32_t totalWords) {
  return ansOverhead(numBlocks) + 2ull * totalWords;
}
// float header word kFloatSecondAns (GpuFloatHeader2)
__host__ __device__ constexpr uint64_t secondAnsOffset(uint32_t numBlocks, uint32_t totalWords0) {
  return roundUp64(ansArchiveBytes(numBlocks, totalWords0), 16);
}

// Float raw section, FloatTypeInfo<FT>::getUncompDataSize
// (float/GpuFloatUtils.cuh:200-391).  ft: 1 fp16, 2 bf16, 3 fp32, 4 fp64.
// The first plane holds every word's low 1 / 1 / 2 / 4 bytes, the second
// (fp32, fp64) its next 1 / 2; each plane is padded.  U: uint32_t in the
// kernels; the host sizes capacities in 64 bits.
template <typename U>
__host__ __device__ constexpr U floatPlane2Offset(int ft, U n) {
  const U n4 = (n + 3) / 4 * 4, n8 = (n + 7) / 8 * 8, n16 = (n + 15) / 16 * 16;
  return ft == 3 ? 2 * n8 : (ft == 4 ? 4 * n4 : n16);
}
template <typename U>
__host__ __device__ constexpr U floatRawBytes(int ft, U n) {
  const U n8 = (n + 7) / 8 * 8, n16 = (n + 15) / 16 * 16;
  return floatPlane2Offset(ft, n) + (ft == 3 ? n16 : (ft == 4 ? 2 * n8 : U(0)));
}
__host__ __device__ constexpr uint32_t floatWordBytes(int ft) {
  return ft <= 2 ? 2 : (ft == 3 ? 4 : 8);
}

// Bytes of a sparse archive before its dense part: header and the bitmap
// (a bit per word) padded to 16 (float/GpuSparseFloatCompress.cuh, SURVEY
// Appendix A.3)
__host__ __device__ constexpr uint64_t sparsePrefixBytes(uint32_t n) {
  return kSparseHeaderBytes + roundUp64((uint64_t(n) + 7) / 8, 16);
}

// Bytes of a finished element archive: float type ft (0: a byte archive) of n
// words in nBlocks blocks, whose one or two ANS archives hold words0 / words1
// compressed words; sparseN >= 0: the dense part of a sparse archive of
// sparseN words, counted with its prefix.
__host__ __device__ constexpr uint64_t archiveBytes(int ft, uint32_t n, uint32_t nBlocks, uint32_t words0,
                                                    uint32_t words1 = 0, int64_t sparseN = -1) {
  uint64_t sz = ansArchiveBytes(nBlocks, words0);
  if (ft != 0) sz += uint64_t(kFloatHeaderBytes) + floatRawBytes(ft, n);
  if (ft == 4) sz += ansArchiveBytes(nBlocks, words1);
  if (sparseN >= 0) sz += sparsePrefixBytes(uint32_t(sparseN));
  return sz;
}

// Pins against the reference: archive sizes of constant inputs (no compressed
// words, so pure layout) of 1, 4105 and 8199 words as the CPU oracle writes
// them (oracle.ans_encode, float_compress, sparse_compress).
static_assert(archiveBytes(0, 1, 1, 0) == 688 && archiveBytes(0, 4105, 2, 0) == 816 &&
                  archiveBytes(0, 8199, 3, 0) == 960, "byte archive layout");
static_assert(archiveBytes(1, 1, 1, 0) == 736 && archiveBytes(2, 4105, 2, 0) == 4960 &&
                  archiveBytes(2, 8199, 3, 0) == 9200, "fp16 / bf16 archive layout");
static_assert(archiveBytes(3, 1, 1, 0) == 752 && archiveBytes(3, 4105, 2, 0) == 13184 &&
                  archiveBytes(3, 8199, 3, 0) == 25600, "fp32 archive layout");
static_assert(archiveBytes(4, 1, 1, 0, 0) == 1440 && archiveBytes(4, 4105, 2, 0, 0) == 26320 &&
                  archiveBytes(4, 8199, 3, 0, 0) == 51152, "fp64 archive layout");
static_assert(secondAnsOffset(1, 0) == 688 && secondAnsOffset(2, 0) == 816 && secondAnsOffset(3, 0) == 960,
              "float header word 4");
static_assert(sparsePrefixBytes(1) == 32 && sparsePrefixBytes(4105) == 544 && sparsePrefixBytes(8199) == 1056,
              "sparse prefix");
static_assert(archiveBytes(2, 1, 1, 0, 0, 4105) == 544 + 736, "sparse archive = prefix + dense archive");

// ---------------------------------------------------------------------------
// device: addresses
// ---------------------------------------------------------------------------
// The raw section of float element `base`
template <typename B>
__device__ __forceinline__ gp<B> rawSectionOf(gp<B> base) {
  return base + kFloatHeaderBytes;
}

// The ANS archive inside element `base` of n words: the element itself for
// raw bytes; for floats it follows the float header and the raw section
// (fp64's second archive follows the first, float header word 4).
template <int FT, typename B>
__device__ __forceinline__ gp<B> ansArchiveOf(gp<B> base, uint32_t n) {
  return base + (FT == 0 ? 0u : kFloatHeaderBytes + floatRawBytes(FT, n));
}

// The sections of the ANS archive at o that follow its header and pdf table
// (ANSCoalescedHeader, ans/GpuANSUtils.cuh:68-86; ansOverhead is their size
// up to `words`).  Every kernel that writes an archive and the decoder take
// their addresses from here.  (The decoder only reads through them.)
struct AnsSections {
  gp<uint8_t> states;  // [nBlocks][32] u32: the blocks' final states
  gp<uint2> bwords;    // [roundUp(nBlocks, 2)] blockWordsEntry
  gp<uint16_t> words;  // the blocks' compressed words, each padded to 8
  __device__ __forceinline__ AnsSections(gp<const uint8_t> o, uint32_t nBlocks)
      : states((gp<uint8_t>)o + kANSHeaderBytes + kPdfBytes),
        bwords((gp<uint2>)(states + uint64_t(kStateBytesPerBlock) * nBlocks)),
        words((gp<uint16_t>)(bwords + roundUp(nBlocks, 2))) {}
};

// Block k's entry of the block-words section: its symbols and compressed
// words, and the word offset of its first compressed word
__device__ __forceinline__ uint2 blockWordsEntry(uint32_t n, uint32_t k, uint32_t words, uint32_t offset) {
  return make_uint2((symbolsOfBlock(k, n) << 16) | words, offset);
}

// ---------------------------------------------------------------------------
// device: writers.  The headers and closeElement are called by one lane.
// ---------------------------------------------------------------------------
// Every word of the ANS header at o but kAnsTotalWords (closeElement)
__device__ __forceinline__ void writeAnsHeader(gp<uint8_t> o, uint32_t nBlocks, uint32_t n, int pb,
                                               bool useChecksum, uint32_t checksum) {
  gp<uint32_t> h = (gp<uint32_t>)o;
  h[kAnsMagic] = kANSMagicVersion;
  h[kAnsBlocks] = nBlocks;
  h[kAnsSize] = n;
  h[kAnsPrecision] = uint32_t(pb) | (useChecksum ? kChecksumFlag : 0u);
  h[kAnsChecksum] = useChecksum ? checksum : 0u;
#pragma unroll
  for (uint32_t w = kAnsZeros; w < kANSHeaderBytes / 4; ++w) h[w] = 0;
}

// Every word of the float header at base but kFloatSecondAns (closeElement)
__device__ __forceinline__ void writeFloatHeader(gp<uint8_t> base, int ft, uint32_t n, bool useChecksum,
                                                 uint32_t checksum) {
  gp<uint32_t> h = (gp<uint32_t>)base;
  h[kFloatMagic] = kFloatMagicVersion;
  h[kFloatSize] = n;
  h[kFloatType] = uint32_t(ft) | (useChecksum ? kChecksumFlag : 0u);
  h[kFloatChecksum] = useChecksum ? checksum : 0u;
#pragma unroll
  for (uint32_t w = kFloatZeros; w < kFloatHeaderBytes / 4; ++w) h[w] = 0;
}

// The header of the sparse archive at o, of n words
__device__ __forceinline__ void writeSparseHeader(gp<uint8_t> o, uint32_t n) {
  static_assert(kSparseHeaderBytes == 16, "one 16 B store");
  st16(o, make_uint4(n, 0, 0, 0));
}

// The header(s) of element `base`, whose (first) ANS archive is o: a byte
// archive carries the element's checksum in its ANS header, a float archive
// in its float header.  (k_pcompress spells the same stores out with the
// names above: called from there this function changes the kernel's spills.)
template <int FT>
__device__ __forceinline__ void writeHeaders(gp<uint8_t> base, gp<uint8_t> o, uint32_t n, uint32_t nBlocks,
                                             int pb, bool useChecksum, uint32_t checksum) {
  writeAnsHeader(o, nBlocks, n, pb, FT == 0 && useChecksum, checksum);
  if constexpr (FT != 0) writeFloatHeader(base, FT, n, useChecksum, checksum);
}

// Zero the rounding tail of each plane of float element base's raw section
// (reference: uninitialised).  Called with lane = 0..15 at least.
template <int FT>
__device__ __forceinline__ void zeroRawTails(gp<uint8_t> base, uint32_t n, uint32_t lane) {
  if constexpr (FT != 0) {
    if (lane < 16) {
      gp<uint8_t> raw = rawSectionOf(base), raw2 = raw + floatPlane2Offset(FT, n);
      const uint32_t i = n + lane;
      if constexpr (FT == 1 || FT == 2) {
        if (i < roundUp(n, 16)) raw[i] = 0;
      } else if constexpr (FT == 3) {
        if (i < roundUp(n, 8)) ((gp<uint16_t>)raw)[i] = 0;
        if (i < roundUp(n, 16)) raw2[i] = 0;
      } else {
        if (i < roundUp(n, 4)) ((gp<uint32_t>)raw)[i] = 0;
        if (i < roundUp(n, 8)) ((gp<uint16_t>)raw2)[i] = 0;
      }
    }
  }
}

// Close element b (`base`, n words in nBlocks blocks) once its one or two ANS
// archives' word totals are known.  Poisoned (a look-back gave up): the
// element is abandoned, size 0, and counted on the device error word.
// Otherwise: each ANS header's total, the pad entry that evens an odd block
// count's block-words section, float header word kFloatSecondAns and the
// element's size (sparseN: the sizes of the sparse elements whose prefix
// precedes this dense archive; null otherwise).
template <int FT>
__device__ __forceinline__ void closeElement(gp<uint8_t> base, uint32_t n, uint32_t nBlocks, bool poisoned,
                                             uint32_t words0, uint32_t words1, uint32_t* outSize,
                                             const uint32_t* sparseN, uint32_t b, uint32_t* err) {
  if (poisoned) {
    if (outSize) G(outSize)[b] = 0u;
    __hip_atomic_fetch_add(G(err), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  gp<uint8_t> o = ansArchiveOf<FT>(base, n);
  const uint32_t words[2] = {words0, words1};
#pragma unroll
  for (int s = 0; s < FloatTraits<FT>::kSegs; ++s) {
    ((gp<uint32_t>)o)[kAnsTotalWords] = words[s];
    if (nBlocks & 1) st8(AnsSections(o, nBlocks).bwords + nBlocks, make_uint2(0, 0));
    if (FT != 0 && s == 0) ((gp<uint32_t>)base)[kFloatSecondAns] = uint32_t(secondAnsOffset(nBlocks, words0));
    o += secondAnsOffset(nBlocks, words0);
  }
  if (outSize)
    G(outSize)[b] = uint32_t(archiveBytes(FT, n, nBlocks, words0, words1, sparseN ? int64_t(sparseN[b]) : -1));
}

}  // namespace dietgpu
