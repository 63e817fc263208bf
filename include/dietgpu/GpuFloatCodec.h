// Public C++ API of the MI355X-native exponent-split float codec and the
// sparse-float codec.
//
// Drop-in for dietgpu/float/GpuFloatCodec.h:32-322 of NSagan271/dietgpu_fork:
// same names, argument order, units (float sizes/capacities in *words*,
// compressed sizes in bytes) and semantics; hipStream_t streams.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "dietgpu/GpuANSCodec.h"

namespace dietgpu {

class StackDeviceMemory;

enum class FloatType : uint32_t {
  kUndefined = 0,
  kFloat16 = 1,
  kBFloat16 = 2,
  kFloat32 = 3,
  kFloat64 = 4,
};

uint32_t getMaxFloatCompressedSize(FloatType floatType, uint32_t size);
uint32_t getMaxSparseFloatCompressedSize(FloatType floatType, uint32_t size);

struct FloatCodecConfig {
  inline FloatCodecConfig()
      : floatType(FloatType::kFloat16), useChecksum(false), is16ByteAligned(false) {}
  inline FloatCodecConfig(FloatType ft, const ANSCodecConfig& ansConf, bool align,
                          bool checksum = false)
      : floatType(ft), useChecksum(checksum), ansConfig(ansConf),
        is16ByteAligned(align) {}
  FloatType floatType;
  bool useChecksum;
  ANSCodecConfig ansConfig;  // ansConfig.useChecksum must be false
  // Kept for API compatibility.  The MI355X decoder is always the fused
  // single-pass kernel (fp64 included), so alignment only picks load widths.
  bool is16ByteAligned;
};

using FloatCompressConfig = FloatCodecConfig;
using FloatDecompressConfig = FloatCodecConfig;

enum class FloatDecompressError : uint32_t {
  None = 0,
  ChecksumMismatch = 1,
};

struct FloatDecompressStatus {
  inline FloatDecompressStatus() : error(FloatDecompressError::None) {}
  FloatDecompressError error;
  std::vector<std::pair<int, std::string>> errorInfo;
};

// GpuFloatCodec.h:118-158
void floatCompress(StackDeviceMemory& res, const FloatCompressConfig& config,
                   uint32_t numInBatch, const void** in, const uint32_t* inSize,
                   void** out, uint32_t* outSize_dev, hipStream_t stream);

// GpuFloatCodec.h:160-187
void floatCompressSplitSize(StackDeviceMemory& res,
                            const FloatCompressConfig& config,
                            uint32_t numInBatch, const void* in_dev,
                            const uint32_t* inSplitSizes, void* out_dev,
                            uint32_t outStride, uint32_t* outSize_dev,
                            hipStream_t stream);

// GpuFloatCodec.h:189-203
void floatCompressSparse(StackDeviceMemory& res, const FloatCompressConfig& config,
                         uint32_t numInBatch, const void** in,
                         const uint32_t* inSize, void** out,
                         uint32_t* outSize_dev, hipStream_t stream);

// GpuFloatCodec.h:209-242
FloatDecompressStatus floatDecompress(StackDeviceMemory& res,
                                      const FloatDecompressConfig& config,
                                      uint32_t numInBatch, const void** in,
                                      void** out, const uint32_t* outCapacity,
                                      uint8_t* outSuccess_dev,
                                      uint32_t* outSize_dev, hipStream_t stream);

// GpuFloatCodec.h:244-280
FloatDecompressStatus floatDecompressSplitSize(
    StackDeviceMemory& res, const FloatDecompressConfig& config,
    uint32_t numInBatch, const void** in, void* out_dev,
    const uint32_t* outSplitSizes, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream);

// GpuFloatCodec.h:282-293
FloatDecompressStatus floatDecompressSparse(StackDeviceMemory& res,
                                            const FloatDecompressConfig& config,
                                            uint32_t numInBatch, const void** in,
                                            void** out,
                                            const uint32_t* outCapacity,
                                            uint8_t* outSuccess_dev,
                                            uint32_t* outSize_dev,
                                            hipStream_t stream);

// GpuFloatCodec.h:299-322
void floatGetCompressedInfo(StackDeviceMemory& res, const void** in,
                            uint32_t numInBatch, uint32_t* outSizes_dev,
                            uint32_t* outTypes_dev, uint32_t* outChecksum_dev,
                            hipStream_t stream);
void floatGetCompressedInfoDevice(StackDeviceMemory& res, const void** in_dev,
                                  uint32_t numInBatch, uint32_t* outSizes_dev,
                                  uint32_t* outTypes_dev,
                                  uint32_t* outChecksum_dev, hipStream_t stream);

// ---- MI355X extensions (not in the reference API) ----
// Stride-addressed float batch: no host->device parameter copies at all.
void floatCompressBatchStride(StackDeviceMemory& res,
                              const FloatCompressConfig& config,
                              uint32_t numInBatch, const void* in_dev,
                              uint32_t inPerBatchWords, uint64_t inPerBatchStrideBytes,
                              void* out_dev, uint64_t outPerBatchStrideBytes,
                              uint32_t* outSize_dev, hipStream_t stream);
FloatDecompressStatus floatDecompressBatchStride(
    StackDeviceMemory& res, const FloatDecompressConfig& config,
    uint32_t numInBatch, const void* in_dev, uint64_t inPerBatchStrideBytes,
    void* out_dev, uint64_t outPerBatchStrideBytes, uint32_t outPerBatchCapacityWords,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream);

// Range decode of dense float archives (see ansDecodeBatchRange): first /
// count in float words, out[b] word-aligned.  For sparse archives:
// floatDecompressSparseRange.
void floatDecompressRange(StackDeviceMemory& res,
                          const FloatDecompressConfig& config,
                          uint32_t numInBatch, const void** in,
                          const uint32_t* first, const uint32_t* count,
                          void** out, uint8_t* outSuccess_dev,
                          uint32_t* outSize_dev, hipStream_t stream);

// Range decode of sparse float archives: out[b][j] = word first[b] + j of the
// element that sparse archive in[b] encodes, 0 <= j < count[b], bitwise what
// floatDecompressSparse puts there; nothing else is written.  A bitmap rank
// locates the range's slice of the nonzero list, a dense range decode reads
// that slice only.  in[b] 16-byte aligned, out[b] word-aligned; an archive may
// appear in any number of members (its bitmap is counted once per call).
// outSuccess_dev[b] = 1 iff the range lies inside in[b]'s element
// (first <= N && count <= N - first), the dense archive is valid for this
// config and holds the list slice; outSize_dev[b] = count[b] then, else 0
// (and out[b] is untouched).  An empty range succeeds.  Header bytes 4..15
// are ignored, as by floatDecompressSparse; a dense float or byte archive
// passed in (word 0 is its magic) fails without being read further.
// Temporary memory is sized before any N is known: numInBatch rows of the
// largest count[b] + 32 words (members with first + count >= 2^32, which
// always fail, aside), and 4 bytes per 1024 words up to each archive's
// largest range end.  A call whose rows do not fit `res` throws as a whole,
// so one absurd count turns per-member status into a call-level error.
// config.useChecksum must be false (archives written with a checksum decode
// normally).  No host synchronisation.
void floatDecompressSparseRange(StackDeviceMemory& res,
                                const FloatDecompressConfig& config,
                                uint32_t numInBatch, const void** in,
                                const uint32_t* first, const uint32_t* count,
                                void** out, uint8_t* outSuccess_dev,
                                uint32_t* outSize_dev, hipStream_t stream);

// Decode-and-accumulate: acc[b][i] = acc[b][i] + x[i], 0 <= i < n, where x is
// the element (n words) that dense float archive in[b] encodes: one kernel,
// no temporary.  accType is the accumulators' type: config.floatType (the
// sum is formed in the archive's own type), or kFloat32 when config.floatType
// is kFloat16 / kBFloat16 (acc + float(x), x widened exactly); anything else
// throws.  Every sum is the correctly rounded IEEE sum in the accumulator's
// type (nearest even, denormals kept, x + (-x) = +0, overflow to +-inf); a
// NaN result is some NaN.  in[b] 4-byte aligned; acc[b] aligned to the
// accumulator's word, accCapacity[b] in accumulator words.  Status as
// floatDecompress: outSuccess_dev[b] = 1 iff the archive is valid for this
// config and accCapacity[b] >= n; outSize_dev[b] = n for a valid archive,
// else 0.  A failing member's accumulator is neither read nor written, and
// nothing outside acc[b][0 .. n) ever is.  Two members whose accumulators
// overlap are the caller's error: the result is undefined and not checked
// for.  config.useChecksum must be false: the decoder verifies a checksum on
// the decoded words, which an accumulated destination no longer holds
// (archives written with a checksum decode normally).  No host
// synchronisation, no allocation outside `res`.
void floatDecompressAccumulate(StackDeviceMemory& res,
                               const FloatDecompressConfig& config,
                               uint32_t numInBatch, const void** in, void** acc,
                               const uint32_t* accCapacity, FloatType accType,
                               uint8_t* outSuccess_dev, uint32_t* outSize_dev,
                               hipStream_t stream);

// Fused multi-archive reduce: for member b, the numSources dense float
// archives x_1 .. x_K = in[k * numInBatch + b] (source-major), each of n words:
//   out[b][i] = round((...((init[b][i] + x_1[i]) + x_2[i]) + ...) + x_K[i])
// for 0 <= i < n, in one kernel pass over all K archives with the running sum
// in registers (K above the kernel's source limit: chained passes through an
// fp32 partial taken from `res`; the split never changes the order or the
// bits).  config.floatType is kFloat16, kBFloat16 or kFloat32; every add is
// one correctly rounded fp32 add (archive words widened exactly).  init may be
// null (the sum then starts as float(x_1), not +0.0: K = 1 returns the decoded
// element, -0.0 included), else initType is config.floatType or kFloat32.
// outType is config.floatType (the sum rounded once, to nearest even) or
// kFloat32 (not rounded).  numSources in 1 .. 64; anything else throws.
// out[b] may be init[b] itself when the types agree; any other overlap is
// undefined and not checked.  in[.] 4-byte aligned, init[b] / out[b] aligned
// to their words, outCapacity[b] in out words.  outSuccess_dev[b] = 1 iff all
// K archives are valid for this config, hold the same n, and
// outCapacity[b] >= n; outSize_dev[b] = n when all K are valid and agree, else
// 0.  A member fails as a whole: its out and init are neither read nor
// written, and nothing outside out[b][0 .. n) ever is.  config.useChecksum
// must be false, for floatDecompressAccumulate's reason (archives written with
// a checksum reduce normally).  No host synchronisation, no allocation outside
// `res`: the call can be captured in a graph and replayed on new archive bytes.
void floatReduceArchives(StackDeviceMemory& res,
                         const FloatDecompressConfig& config,
                         uint32_t numInBatch, uint32_t numSources,
                         const void** in, const void** init, FloatType initType,
                         void** out, const uint32_t* outCapacity,
                         FloatType outType, uint8_t* outSuccess_dev,
                         uint32_t* outSize_dev, hipStream_t stream);

// Sparse decode-and-accumulate: acc[b][i] = acc[b][i] + x[i] for every i < n
// whose bit is set in the bitmap of sparse float archive in[b] (x: the n-word
// element it encodes; a word is "set" iff it is not +0.0 bitwise, so -0.0 is
// added).  Every other accumulator word is neither read nor written: the
// expansion adds where floatDecompressSparse stores, with no temporary and no
// traffic for the zeros.  accType and the sums follow floatDecompressAccumulate
// (config.floatType, or kFloat32 for kFloat16 / kBFloat16; anything else
// throws; each sum correctly rounded in the accumulator's type).
// Deviation from the dense form: a clear bit stands for +0.0, and IEEE
// a + (+0.0) differs from a for a = -0.0 (the sum is +0.0) and for a
// signalling NaN (it is quieted); here such accumulator words keep their
// bits.  in[b] 16-byte aligned, acc[b] aligned to the accumulator's word,
// accCapacity[b] in accumulator words.  Status as floatDecompressSparse:
// outSuccess_dev[b] = 1 iff the dense part is valid for this config and
// accCapacity[b] >= n; outSize_dev[b] = n always (it comes from the sparse
// header).  A failing member's accumulator is neither read nor written, and
// nothing outside the set positions of acc[b][0 .. n) ever is.  Overlapping
// accumulators are the caller's error.  config.useChecksum must be false, for
// floatDecompressAccumulate's reason (archives written with a checksum decode
// normally).  No host synchronisation, no allocation outside `res`.
void floatDecompressSparseAccumulate(StackDeviceMemory& res,
                                     const FloatDecompressConfig& config,
                                     uint32_t numInBatch, const void** in,
                                     void** acc, const uint32_t* accCapacity,
                                     FloatType accType, uint8_t* outSuccess_dev,
                                     uint32_t* outSize_dev, hipStream_t stream);

// Fused sparse reduce: floatReduceArchives for sparse float archives.  For
// member b, the numSources sparse archives x_1 .. x_K = in[k * numInBatch + b]
// (source-major), each of n words, and 0 <= i < n:
//   a = float(init[b][i]);
//   for k = 1 .. K in source order: if bit i of x_k's bitmap is set (the word
//     is not +0.0 bitwise, so -0.0 is added), a = a + float(x_k[i]), one
//     correctly rounded fp32 add with denormals kept; if it is clear, a keeps
//     its bits;
//   out[b][i] = a rounded to nearest even to outType (not rounded for kFloat32).
// A clear bit is skipped, never added as +0.0 (floatDecompressSparseAccumulate's
// rule): an init word of -0.0 or a signalling NaN under clear bits comes out
// with its bits.  init may be null: the sum then starts as a = float(x_1[i]),
// the decoded word (+0.0 where its bit is clear, the element's -0.0 where it
// holds one), and runs over x_2 .. x_K; K = 1 returns the decoded element.
// The result equals, bit for bit, own.to(fp32), one
// floatDecompressSparseAccumulate per archive in order, and one rounding; a
// NaN result is some NaN.  One kernel pass over all K archives with the
// running sum in registers (K above the kernel's source limit: chained passes
// through an fp32 partial taken from `res`; the split never changes the order
// or the bits).  config.floatType is kFloat16, kBFloat16 or kFloat32; initType
// and outType are config.floatType or kFloat32; numSources in 1 .. 64;
// anything else throws.  out[b] may be init[b] itself when the types agree;
// any other overlap is undefined and not checked.  in[.] 16-byte aligned,
// init[b] / out[b] aligned to their words, outCapacity[b] in out words.
// outSuccess_dev[b] = 1 iff the dense parts of all K archives are valid for
// this config, all K sparse headers hold the same n, and outCapacity[b] >= n;
// outSize_dev[b] = n of the first source always (it comes from the sparse
// header).  A member fails as a whole: its out and init are not written and,
// in a call of one pass, not read (a chained call learns of a bad later source
// only in that source's pass; the earlier passes have read init into the
// partial), and nothing outside out[b][0 .. n) ever is written.
// config.useChecksum must be false, for
// floatDecompressAccumulate's reason (archives written with a checksum reduce
// normally).  No host synchronisation, no allocation outside `res`: the call
// can be captured in a graph and replayed on new archive bytes.
void floatReduceSparseArchives(StackDeviceMemory& res,
                               const FloatDecompressConfig& config,
                               uint32_t numInBatch, uint32_t numSources,
                               const void** in, const void** init,
                               FloatType initType, void** out,
                               const uint32_t* outCapacity, FloatType outType,
                               uint8_t* outSuccess_dev, uint32_t* outSize_dev,
                               hipStream_t stream);

// The bytes of `res` that a floatReduceSparseArchives call of numInBatch
// members, numSources sources and capacities of at most maxCapacity words
// takes at most (with an init; the scratch is bounded by the sources of one
// kernel launch, not by numSources).  Host only: no device is touched.
uint64_t floatReduceSparseScratchBytes(FloatType floatType, uint32_t numInBatch,
                                       uint32_t numSources, uint32_t maxCapacity);

// Row gather with device-resident indices from a dense float archive that
// holds a table [R, rowWords] (see ansGatherRows, GpuANSCodec.h: the same
// rules, in float words; out_dev word-aligned).  Sparse archives are not
// gathered from here.
void floatGatherRows(StackDeviceMemory& res,
                     const FloatDecompressConfig& config,
                     const void* archive_dev, uint32_t rowWords, uint32_t numIdx,
                     const void* idx_dev, bool idxIs64, void* out_dev,
                     uint64_t outRowStrideWords, uint8_t* outSuccess_dev,
                     hipStream_t stream);

// Pooled row gather (embedding_bag(mode="sum") on a compressed table): the
// dense fp16 / bf16 / fp32 archive holds a table [R, rowWords]; idx_dev holds
// numIdx row indices and offsets_dev numBags + 1 bag boundaries in device
// memory, both int32 or (idxIs64) both int64.  Bag b is
// idx[offsets[b] .. offsets[b + 1]), and for 0 <= j < rowWords
//   out[b * outRowStrideWords + j] =
//       round_out((..(f(x_1[j]) + f(x_2[j])) + ..) + f(x_m[j]))
// with x_t the row named by the bag's t-th index, f the exact conversion to
// fp32, every add a correctly rounded fp32 add in list order, the running sum
// started as f(x_1) (a one-row bag returns the row, -0.0 included) and one
// rounding to the output type: fp32 when outIsFp32 (always for fp32
// archives), else the archive's 16-bit type.  An empty bag gives a row of
// +0.0.  outSuccess_dev[b] (optional) = 1 iff the archive is valid for this
// config, 0 <= offsets[b] <= offsets[b + 1] <= numIdx and every index of the
// bag lies in [0, n / rowWords); a failing bag's row is untouched, and nothing
// but the rowWords words of succeeding bags is written.  One launch, no host
// synchronisation, no allocation, no atomics: the call can be captured in a
// graph, and its result is the same bits on every run.  Refused before any
// launch: fp64 archives, a config with useChecksum, rowWords == 0, a stride
// below rowWords, and numBags * ceil(rowWords / 128) >= 2^32.  Not offered:
// mean / max pooling, per-sample weights, sparse archives, a backward pass.
void floatGatherRowsSum(StackDeviceMemory& res,
                        const FloatDecompressConfig& config,
                        const void* archive_dev, uint32_t rowWords,
                        uint32_t numBags, uint32_t numIdx, const void* idx_dev,
                        const void* offsets_dev, bool idxIs64, void* out_dev,
                        bool outIsFp32, uint64_t outRowStrideWords,
                        uint8_t* outSuccess_dev, hipStream_t stream);

} // namespace dietgpu
