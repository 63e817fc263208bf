// Internal entry points shared by the dense and sparse float drivers.
#pragma once

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "archive.h"
#include "batch.h"
#include "batch_tables.h"
#include "compress_plan.h"
#include "decode_plan.h"
#include "entry_checks.h"
#include "dietgpu/GpuFloatCodec.h"

namespace dietgpu {

// Partial symbol histograms of the float words counted by the caller (the
// sparse compressor counts its nonzeros as it compacts them, so the dense
// codec's histogram pass is skipped): u32 rows [segments][nb][nRows][256],
// summed per element.  Ignored when the single-pass compressor takes the call.
// table / pdf non-null: the caller has normalised the rows too
// ([segments][nb][256] encode-table entries and u16 pdfs, NormArgs layout),
// so the dense codec goes straight to k_encode.
struct PartialHist {
  const uint32_t* rows;
  uint32_t nRows;
  const uint4* table = nullptr;
  const uint16_t* pdf = nullptr;
};

// One compress call of the generic drivers (codec.hip): nb elements `in` of at
// most maxSize units (bytes, or float words) into the archives `out`.
struct CompressCall {
  StackDeviceMemory& res;
  hipStream_t s;
  int pb = 0;
  bool useChecksum = false;
  uint32_t nb = 0;
  BatchDesc in;
  uint32_t maxSize = 0;
  BatchDesc out;
  uint32_t* outSize_dev = nullptr;
  const uint32_t* hist_dev = nullptr;  // byte codec: the caller's histograms
  const DeviceTables* tabs = nullptr;  // the tables `in` / `out` refer to
  // every element's input starts 16 B-aligned (the single-pass compressor
  // reads whole 16 B vectors; anything else takes three kernels)
  bool inAligned16 = false;
  const PartialHist* pre = nullptr;
  // the sparse codec's N per element: the archive's size writer adds the
  // sparse header and bitmap to outSize (EncTail::sparseN)
  const uint32_t* sparseN = nullptr;
};

// One decode call of the generic driver (codec.hip decodeBatchDevice) or of
// the sparse one (sparse.hip sparseDecompressT: full and accumulate): nb
// archives `in` into `out`, in one of the forms of decode_plan.h.
//  - full, accumulate: capacities out.size(b), at most maxCapacity units;
//    an accumulate call's `out` are the accumulators, counted in their words.
//  - range: words [in.size(b), + out.size(b)) of archive in.start(b) (the
//    `first` column rides as the input descriptor's size column, which the
//    other forms leave empty); both columns may be device arrays a previous
//    kernel wrote.  maxRangeBlocks: the most 4096-word blocks a member's range
//    touches.  maxCapacity is not read.
struct DecodeCall {
  StackDeviceMemory& res;
  hipStream_t s;
  DecodeForm form = DecodeForm::kFull;
  int pb = 0;
  uint32_t nb = 0;
  BatchDesc in, out;
  uint32_t maxCapacity = 0;
  uint32_t maxRangeBlocks = 0;
  uint8_t* outSuccess_dev = nullptr;
  uint32_t* outSize_dev = nullptr;
  const DeviceTables* tabs = nullptr;
  // full only: streaming output stores (nobody re-reads the output right away)
  bool streamOut = true;
  // full only: maxCapacity may far exceed the archives' sizes
  bool capacityOnly = false;
};

// The calls of a batch built by batch_tables.h (b outlives the call).
inline CompressCall compressCall(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const BatchTables& b,
                                 uint32_t* outSize_dev) {
  CompressCall c{res, s};
  c.nb = nb;
  c.in = b.in;
  c.maxSize = b.maxSize;
  c.out = b.out;
  c.outSize_dev = outSize_dev;
  c.tabs = &b.t;
  c.inAligned16 = b.inAligned16;
  return c;
}

inline DecodeCall decodeCall(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const BatchTables& b,
                             uint8_t* outSuccess_dev, uint32_t* outSize_dev) {
  DecodeCall c{res, s};
  c.nb = nb;
  c.in = b.in;
  c.out = b.out;
  c.maxCapacity = b.maxSize;
  c.outSuccess_dev = outSuccess_dev;
  c.outSize_dev = outSize_dev;
  c.tabs = &b.t;
  return c;
}

// The two decode-and-accumulate entry points: every
// host check, before the first allocation, upload or launch, then
// run(call) on the batch's DecodeCall.  archiveAlign: 4 dense, 16 sparse
// (checkArchiveAligned).
template <typename Run>
void accumulateEntry(StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t nb, const void** in,
                     void** acc, const uint32_t* accCapacity, FloatType accType, uint8_t* outSuccess_dev,
                     uint32_t* outSize_dev, hipStream_t stream, uint32_t archiveAlign, Run&& run) {
  checkFloatConfig(config);
  checkNoChecksum(config.useChecksum, PartialDecode::kAccumulate);
  const DecodeForm form = accumulateForm(config.floatType, accType);
  if (nb == 0) return;
  for (uint32_t i = 0; i < nb; ++i) checkArchiveAligned(reinterpret_cast<uintptr_t>(in[i]), i, archiveAlign);
  const auto b = pointerBatch(res, stream, nb, in, acc, accCapacity, false, floatWordBytes(int(accType)));
  DecodeCall c = decodeCall(res, stream, nb, b, outSuccess_dev, outSize_dev);
  c.form = form;
  run(c);
}

// f(std::integral_constant<int, FT>{}) for the float type's FT (1 fp16,
// 2 bf16, 3 fp32, 4 fp64; the type has been validated).
template <typename F>
decltype(auto) dispatchFloatType(FloatType ft, F&& f) {
  switch (ft) {
    case FloatType::kFloat16: return f(std::integral_constant<int, 1>{});
    case FloatType::kBFloat16: return f(std::integral_constant<int, 2>{});
    case FloatType::kFloat32: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// f(y0, ny) for each slice of a batch that fits a grid's y dimension.
constexpr uint32_t kMaxGridY = 65535;
template <typename F>
void forGridYSlices(uint32_t nb, F&& f) {
  for (uint32_t y0 = 0; y0 < nb; y0 += kMaxGridY) f(y0, std::min(kMaxGridY, nb - y0));
}

// query(device) for the current device, cached per (device, key): the
// runtime's queries cost host time on every call.  Each call site has a cache
// of its own (its lambda's type instantiates the function).
template <typename V, typename K, typename Q>
V cachedPerDevice(const K& key, Q&& query) {
  static std::mutex m;
  static std::map<std::pair<int, K>, V> cache;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(m);
  auto it = cache.find({dev, key});
  if (it == cache.end()) it = cache.emplace(std::make_pair(dev, key), query(dev)).first;
  return it->second;
}

// c.pb / c.useChecksum come from the config.
void floatCompressDescs(const FloatCompressConfig& config, CompressCall c);

// The plan (compress_plan.h) that encodeBatchDevice follows for nb elements of
// at most maxSize units of float type ft (0: the byte codec) on the current
// device, in the current compressPath() mode, with no PartialHist.
CompressPlan planCompressCall(int ft, uint32_t nb, uint32_t maxSize, bool useChecksum, bool userHist,
                              bool inAligned16);

// The dense float decode of a call in any form.  The float type and c.pb come
// from the config, which is validated here.  A full call verifies the checksum
// when the config asks for one (it then reads its output back, so it never
// streams); the other forms cannot, and their callers refuse such a config.
FloatDecompressStatus floatDecompressDescs(const FloatDecompressConfig& config, DecodeCall c);

// Compare the checksums stored in the archives c.in with the XOR of the
// first c.out.size(b) bytes of each decoded element; synchronises c.s.
std::vector<std::pair<int, std::string>> verifyChecksums(const DecodeCall& c, bool isFloat);

// The status of a checksummed decode call (verifyChecksums).
template <typename Status>
Status verifiedStatus(const DecodeCall& c, bool isFloat) {
  Status status;
  status.errorInfo = verifyChecksums(c, isFloat);
  if (!status.errorInfo.empty()) status.error = decltype(status.error)::ChecksumMismatch;
  return status;
}

// The device error word (elements whose compression was abandoned after a
// bounded wait ran out; their outSize is 0), codec.hip.
uint32_t* deviceErrorWord();

}  // namespace dietgpu
