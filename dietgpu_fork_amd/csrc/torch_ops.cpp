// Native PyTorch-ROCm operator library: TORCH_LIBRARY(dietgpu), loadable with
// torch.ops.load_library("dietgpu_fork_amd/_lib/libdietgpu_torch.so").
//
// Every operator runs on the current HIP stream of its inputs' device and
// calls the C++ codec API of libdietgpu_amd.so (include/dietgpu/*.h); all
// compute is in its HIP kernels.  "ref": one of the reference's ten operators
// (dietgpu/DietGpu.cpp:921-978) with its schema, argument meaning, validation
// (TORCH_CHECK -> RuntimeError) and return values; "ext": not in the reference.
//
//   operator                          from  codec entry points (float / byte mode)
//   max_float_compressed_output_size  ref   getMaxFloatCompressedSize
//   max_float_compressed_size         ref   getMaxFloatCompressedSize
//   max_any_compressed_output_size    ref   getMaxCompressedSize
//   max_any_compressed_size           ref   getMaxCompressedSize
//   compress_data                     ref   floatCompress / ansEncodeBatchPointer
//   compress_data_split_size          ref   floatCompressSplitSize / ansEncodeBatchSplitSize
//   compress_data_simple              ref   compress_data's
//   decompress_data                   ref   floatDecompress / ansDecodeBatchPointer
//   decompress_data_split_size        ref   floatDecompressSplitSize / ansDecodeBatchSplitSize
//   decompress_data_simple            ref   float / ansGetCompressedInfo, then decompress_data's
//   decompress_data_range             ext   floatDecompressRange / ansDecodeBatchRange
//   decompress_data_accumulate        ext   floatDecompressAccumulate (*)
//   gather_rows                       ext   floatGatherRows / ansGatherRows
//   reduce_data                       ext   floatReduceArchives (*)
//   gather_rows_sum                   ext   floatGatherRowsSum (*)
//   (*) after floatGetCompressedInfo on ts_in[0] / t_in where only float32 tensors
//       would name the archives' type (peekArchiveType)
//
// An operator builds one CallContext (device guard, stream, arena over
// temp_mem and the high-water mark it returns), fills its Members columns
// (archive() / dest(), both on checkDeviceTensor), takes its config from
// floatConfig / byteConfig and makes its codec call.
//
// Other extensions over the reference: fp64 tensors are accepted on
// decompression too (the reference rejects them at DietGpu.cpp:569-573 /
// 742-746 although its compressor produces them), and an archive the
// compressor had to abandon (outSize 0, see dietgpu_device_error_count in
// include/dietgpu_c.h) raises instead of being returned as an empty tensor.
//
// Argument checks the reference lacks (its DietGpu.cpp says "FIXME: total
// range checking" where they belong); each raises before any temp-memory
// allocation or launch, and archives and results of valid calls are unchanged:
//  - byte mode sizes the archive rows from the widest tensor in bytes, each
//    with its own element size (the reference: the largest numel() times the
//    first tensor's element size, too small for [uint8[4097], int32[4096]]);
//  - compress_data_split_size: the splits must end inside t_in;
//  - decompress_data_split_size: the splits must end inside t_out;
//  - decompress_data in float mode: every ts_out[i] has ts_out[0]'s dtype
//    (the capacities are counted in words of it);
//  - every compressed input is 4-byte aligned and holds at least the 32-byte
//    header that the decoders read first.
// Not checked: a compressed input shorter than the archive that its header
// describes (the header is on the device).
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <cstdint>
#include <limits>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "dietgpu/GpuANSCodec.h"
#include "dietgpu/GpuFloatCodec.h"
#include "dietgpu/StackDeviceMemory.h"
#include "dietgpu_c.h"

namespace dietgpu {
namespace {

constexpr int kDefaultPrecision = 10;  // DietGpu.cpp:119
constexpr uint64_t kU32Max = std::numeric_limits<uint32_t>::max();

FloatType floatTypeOf(at::ScalarType t) {
  switch (t) {
    case at::ScalarType::Half:
      return FloatType::kFloat16;
    case at::ScalarType::BFloat16:
      return FloatType::kBFloat16;
    case at::ScalarType::Float:
      return FloatType::kFloat32;
    case at::ScalarType::Double:
      return FloatType::kFloat64;
    default:
      TORCH_CHECK(false, "unsupported dtype ", t, " for float compression");
  }
}

at::ScalarType dtypeOf(uint32_t ft) {
  switch (ft) {
    case 1:
      return at::ScalarType::Half;
    case 2:
      return at::ScalarType::BFloat16;
    case 3:
      return at::ScalarType::Float;
    case 4:
      return at::ScalarType::Double;
    default:
      TORCH_CHECK(false, "not a float archive (float type ", ft, ")");
  }
}

// The codec configs of every operator (the only users of kDefaultPrecision).
FloatCodecConfig floatConfig(FloatType ft, bool checksum) {
  return FloatCodecConfig(ft, ANSCodecConfig(kDefaultPrecision), false, checksum);
}
ANSCodecConfig byteConfig(bool checksum) { return ANSCodecConfig(kDefaultPrecision, checksum); }

// getTotalAndMaxSize, DietGpu.cpp:63-80 (elements)
std::pair<uint64_t, uint64_t> totalAndMax(const std::vector<at::Tensor>& ts) {
  uint64_t total = 0, mx = 0;
  for (const auto& t : ts) {
    const uint64_t n = uint64_t(t.numel());
    TORCH_CHECK(n * uint64_t(t.element_size()) <= kU32Max, "tensor too large");
    total += n;
    mx = std::max(mx, n);
  }
  TORCH_CHECK(mx <= kU32Max);
  return {total, mx};
}

// The device of an operator's ts_in, a non-empty list of GPU tensors.
int inputDevice(const std::vector<at::Tensor>& tsIn) {
  TORCH_CHECK(!tsIn.empty(), "ts_in must not be empty");
  const int dev = tsIn.front().get_device();
  TORCH_CHECK(dev >= 0, "inputs must be GPU tensors");
  return dev;
}

void checkGpuTensor(const at::Tensor& t, int dev) {
  TORCH_CHECK(t.device().type() == at::kCUDA, "inputs must be GPU tensors");
  TORCH_CHECK(t.is_contiguous(), "inputs must be contiguous");
  TORCH_CHECK(t.get_device() == dev, "inputs must be on one device");
}

// The splits of the split-size operators tile `t` from its start and must
// end inside it: they are words when asFloat and bytes otherwise.  (The
// reference checks neither: DietGpu.cpp "FIXME: total range checking".)
void checkSplitSum(uint64_t sum, const at::Tensor& t, bool asFloat, const char* name) {
  const uint64_t have = asFloat ? uint64_t(t.numel()) : uint64_t(t.numel()) * uint64_t(t.element_size());
  TORCH_CHECK(sum <= have, "the split sizes sum to ", sum, asFloat ? " words" : " bytes", " but ", name, " holds ",
              have);
}

// The split sizes of a split-size operator (argument `name`): a contiguous
// CPU int32 tensor; take(i) checks entry i and adds it to the u32 column.
struct SplitSizes {
  const int32_t* sp;
  int64_t n;
  std::vector<uint32_t> sizes;
  uint64_t sum = 0;
  uint32_t mx = 0;
  SplitSizes(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_contiguous() && t.device().type() == at::kCPU && t.scalar_type() == at::kInt, name,
                " must be a contiguous CPU int32 tensor");
    sp = t.data_ptr<int32_t>();
    n = t.numel();
    sizes.resize(size_t(n));
  }
  void take(int64_t i) {
    TORCH_CHECK(sp[i] > 0, "split sizes must be > 0");
    sizes[size_t(i)] = uint32_t(sp[i]);
    mx = std::max(mx, sizes[size_t(i)]);
    sum += sizes[size_t(i)];
  }
  const uint32_t* data() const { return sizes.data(); }
};

// A contiguous GPU tensor on the operator's device, or `message`.
void checkDeviceTensor(const at::Tensor& t, int dev, const char* message) {
  TORCH_CHECK(t.device().type() == at::kCUDA && t.get_device() == dev && t.is_contiguous(), message);
}

// An archive on the device: contiguous uint8, 4-byte aligned (k_decode reads
// the headers with scalar loads, which drop the low two address bits: the
// header of an archive off 4 B alignment would be read from up to three
// bytes before the tensor; ansDecodeBatchRange checks this itself, the full
// decoders do not), and at least the 32-byte header that every archive
// begins with and every decoder and k_info reads first.  (Whether the tensor
// holds all of the archive that its header describes is not checked: the
// header is on the device.)
constexpr int64_t kArchiveHeaderBytes = 32;
void checkArchiveTensor(const at::Tensor& t, int dev) {
  checkDeviceTensor(t, dev, "compressed inputs must be contiguous GPU tensors on one device");
  TORCH_CHECK(t.scalar_type() == at::kByte, "compressed inputs must be uint8");
  TORCH_CHECK(t.numel() >= kArchiveHeaderBytes, "compressed inputs must hold at least the ", kArchiveHeaderBytes,
              "-byte archive header");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 4 == 0, "compressed inputs must be 4-byte aligned");
}

// What every launching operator holds: the guard of its device, the current
// stream there and the arena over the caller's temp_mem tensor
// (DietGpu.cpp:303-315), or an empty one whose every allocation overflows to
// hipMalloc.  The temp_mem checks run where the arena is built: at once, or
// where an operator that checks other arguments first calls stack().
struct CallContext {
  const int dev;
  c10::hip::HIPGuard guard;
  const hipStream_t stream;
  std::optional<StackDeviceMemory> res;
  explicit CallContext(int d) : dev(d), guard(d), stream(c10::hip::getCurrentHIPStream(d).stream()) {}
  CallContext(int d, const std::optional<at::Tensor>& tempMem) : CallContext(d) { stack(tempMem); }
  void stack(const std::optional<at::Tensor>& tempMem) {
    if (tempMem) {
      TORCH_CHECK(tempMem->device().type() == at::kCUDA, "temp_mem must be a GPU tensor");
      TORCH_CHECK(tempMem->is_contiguous(), "temp_mem must be contiguous");
      TORCH_CHECK(tempMem->get_device() == dev, "temp_mem must be on the input device");
      const size_t bytes = size_t(tempMem->numel()) * tempMem->element_size();
      res.emplace(dev, bytes ? tempMem->data_ptr() : nullptr, bytes);
    } else {
      res.emplace(dev, nullptr, 0);
    }
  }
  // what the operators return: the arena's high-water mark
  int64_t used() const { return int64_t(res->getMaxMemoryUsage()); }
};

// Sizes of archives the compressor could not finish are 0: never hand one out.
void checkArchiveSizes(const int32_t* sizes, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (sizes[i] <= 0) {
      // (read and reset, as _native.check_archive_sizes does: a later error
      // reports only the elements abandoned since this one)
      const uint32_t errs = dietgpu_device_error_count(1);
      TORCH_CHECK(false, "compression of batch element ", i,
                  " was abandoned (a cross-workgroup wait ran out of polls; ", errs,
                  " element(s) counted in the device error word since the last report)");
    }
  }
}

// ---------------------------------------------------------------- sizes ----

std::tuple<int64_t, int64_t> max_float_compressed_output_size(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK(!ts.empty(), "the tensor list must not be empty");
  const auto tm = totalAndMax(ts);
  return {int64_t(ts.size()), int64_t(getMaxFloatCompressedSize(floatTypeOf(ts.front().scalar_type()),
                                                                uint32_t(tm.second)))};
}

int64_t max_float_compressed_size(const at::Tensor& dtype, int64_t size) {
  TORCH_CHECK(size >= 0 && uint64_t(size) <= kU32Max, "size out of range");
  return int64_t(getMaxFloatCompressedSize(floatTypeOf(dtype.scalar_type()), uint32_t(size)));
}

std::tuple<int64_t, int64_t> max_any_compressed_output_size(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK(!ts.empty(), "the tensor list must not be empty");
  totalAndMax(ts);
  // byte mode takes lists of mixed dtypes: the widest member in bytes, each
  // tensor with its own element size (the reference multiplies the largest
  // numel() by the first tensor's, DietGpu.cpp:139-148)
  uint64_t bytes = 0;
  for (const auto& t : ts) bytes = std::max(bytes, uint64_t(t.numel()) * uint64_t(t.element_size()));
  TORCH_CHECK(bytes <= kU32Max, "tensor too large");
  return {int64_t(ts.size()), int64_t(getMaxCompressedSize(uint32_t(bytes)))};
}

int64_t max_any_compressed_size(int64_t bytes) {
  TORCH_CHECK(bytes >= 0 && uint64_t(bytes) <= kU32Max, "size out of range");
  return int64_t(getMaxCompressedSize(uint32_t(bytes)));
}

// ------------------------------------------------------------- compress ----

// The caller's out_compressed / out_compressed_bytes, validated for n rows of
// cols bytes on `dev`, or fresh tensors with the options of `like`.
std::pair<at::Tensor, at::Tensor> outputTensors(const std::optional<at::Tensor>& outCompressed,
                                                const std::optional<at::Tensor>& outSizes, int64_t n,
                                                int64_t cols, int dev, const at::Tensor& like) {
  at::Tensor comp;
  if (outCompressed) {
    const auto& c = *outCompressed;
    TORCH_CHECK(c.scalar_type() == at::kByte && c.device().type() == at::kCUDA && c.is_contiguous(),
                "out_compressed must be a contiguous uint8 GPU tensor");
    TORCH_CHECK(c.dim() == 2 && c.size(0) >= n && c.size(1) >= cols, "out_compressed must be 2-d, at least [", n,
                ", ", cols, "]");
    TORCH_CHECK(c.get_device() == dev, "out_compressed must be on the input device");
    comp = c;
  } else {
    comp = at::empty({n, cols}, like.options().dtype(at::kByte));
  }
  at::Tensor sizes;
  if (outSizes) {
    const auto& s = *outSizes;
    TORCH_CHECK(s.scalar_type() == at::kInt && s.device().type() == at::kCUDA && s.dim() == 1,
                "out_compressed_bytes must be a 1-d int32 GPU tensor");
    TORCH_CHECK(s.is_contiguous() && s.size(0) >= n && s.get_device() == dev,
                "out_compressed_bytes must be contiguous, on the input device, with at least ", n, " entries");
    sizes = s;
  } else {
    sizes = at::empty({n}, like.options().dtype(at::kInt));
  }
  return {comp, sizes};
}

// Row i of `matrix` narrowed to its archive's size (host sizes h, checked).
std::vector<at::Tensor> narrowRows(const at::Tensor& matrix, const int32_t* h, int64_t n, bool clone) {
  checkArchiveSizes(h, n);
  const at::Tensor flat = matrix.view({-1});
  const int64_t cols = matrix.size(1);
  std::vector<at::Tensor> out;
  out.reserve(size_t(n));
  for (int64_t i = 0; i < n; ++i) {
    const at::Tensor row = flat.narrow(0, i * cols, h[i]);
    out.push_back(clone ? row.clone() : row);
  }
  return out;
}

// compress_data_res, DietGpu.cpp:161-287
std::tuple<at::Tensor, at::Tensor, int64_t> compress_data(bool asFloat, const std::vector<at::Tensor>& ts,
                                                          bool checksum, const std::optional<at::Tensor>& tempMem,
                                                          const std::optional<at::Tensor>& outCompressed,
                                                          const std::optional<at::Tensor>& outSizes) {
  CallContext cx(inputDevice(ts), tempMem);
  const auto rc = asFloat ? max_float_compressed_output_size(ts) : max_any_compressed_output_size(ts);
  const int64_t cols = std::get<1>(rc);
  for (const auto& t : ts) {
    checkGpuTensor(t, cx.dev);
    if (asFloat) {
      TORCH_CHECK(t.scalar_type() == ts.front().scalar_type(), "float inputs must share a dtype");
      floatTypeOf(t.scalar_type());
    }
  }
  const auto n = int64_t(ts.size());
  const auto [comp, sizes] = outputTensors(outCompressed, outSizes, n, cols, cx.dev, ts.front());
  std::vector<const void*> in(ts.size());
  std::vector<uint32_t> inSize(ts.size());
  std::vector<void*> out(ts.size());
  auto* base = static_cast<uint8_t*>(comp.data_ptr());
  for (size_t i = 0; i < ts.size(); ++i) {
    in[i] = ts[i].data_ptr();
    inSize[i] = uint32_t(asFloat ? ts[i].numel() : ts[i].numel() * ts[i].element_size());
    out[i] = base + int64_t(i) * comp.size(1);
  }
  auto* osz = reinterpret_cast<uint32_t*>(sizes.data_ptr<int32_t>());
  if (asFloat) {
    floatCompress(*cx.res, floatConfig(floatTypeOf(ts.front().scalar_type()), checksum), uint32_t(n), in.data(),
                  inSize.data(), out.data(), osz, cx.stream);
  } else {
    ansEncodeBatchPointer(*cx.res, byteConfig(checksum), uint32_t(n), in.data(), inSize.data(), nullptr, out.data(),
                          osz, cx.stream);
  }
  return {comp, sizes, cx.used()};
}

// compressedMatrixToTensors, DietGpu.cpp:84-108
std::vector<at::Tensor> matrixToTensors(int64_t n, const at::Tensor& matrix, const at::Tensor& sizes) {
  const at::Tensor host = sizes.narrow(0, 0, n).to(at::kCPU);
  return narrowRows(matrix, host.data_ptr<int32_t>(), n, /*clone=*/false);
}

// DietGpu.cpp:322-470
std::tuple<std::vector<at::Tensor>, at::Tensor, int64_t> compress_data_split_size(
    bool asFloat, const at::Tensor& tIn, const at::Tensor& tSplit, bool checksum,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outCompressed,
    const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(tIn.device().type() == at::kCUDA && tIn.is_contiguous(), "t_in must be a contiguous GPU tensor");
  CallContext cx(tIn.get_device());
  const FloatType ft = asFloat ? floatTypeOf(tIn.scalar_type()) : FloatType::kUndefined;
  if (!asFloat) {
    TORCH_CHECK(reinterpret_cast<uintptr_t>(tIn.data_ptr()) % 4 == 0,
                "All splits should start on a 16 byte boundary; start pointer is not aligned");
  }
  SplitSizes split(tSplit, "t_in_split_sizes");
  const int64_t n = split.n;
  for (int64_t i = 0; i < n; ++i) {
    split.take(i);
    if (!asFloat && i != n - 1) {
      TORCH_CHECK(split.sp[i] % 4 == 0,
                  "All splits should start on a 16 byte boundary; the size of an interior split is not a "
                  "multiple of 16 bytes");
    }
  }
  checkSplitSum(split.sum, tIn, asFloat, "t_in");
  const uint32_t mx = split.mx;
  const int64_t cols = asFloat ? int64_t(getMaxFloatCompressedSize(ft, mx)) : int64_t(getMaxCompressedSize(mx));
  const auto [comp, sizes] = outputTensors(outCompressed, outSizes, n, cols, cx.dev, tIn);
  cx.stack(tempMem);
  auto* osz = reinterpret_cast<uint32_t*>(sizes.data_ptr<int32_t>());
  if (asFloat) {
    floatCompressSplitSize(*cx.res, floatConfig(ft, checksum), uint32_t(n), tIn.data_ptr(), split.data(),
                           comp.data_ptr(), uint32_t(comp.size(1)), osz, cx.stream);
  } else {
    ansEncodeBatchSplitSize(*cx.res, byteConfig(checksum), uint32_t(n), tIn.data_ptr(), split.data(), nullptr,
                            comp.data_ptr(), uint32_t(comp.size(1)), osz, cx.stream);
  }
  auto lst = matrixToTensors(n, comp, sizes);
  return {lst, sizes, cx.used()};
}

// DietGpu.cpp:472-526
std::vector<at::Tensor> compress_data_simple(bool asFloat, const std::vector<at::Tensor>& tsIn, bool checksum,
                                             std::optional<int64_t> tempMem) {
  const int dev = inputDevice(tsIn);
  c10::hip::HIPGuard guard(dev);
  std::optional<at::Tensor> scratch;
  if (tempMem && *tempMem > 0) scratch = at::empty({*tempMem}, tsIn.front().options().dtype(at::kByte));
  auto out = compress_data(asFloat, tsIn, checksum, scratch, std::nullopt, std::nullopt);
  const at::Tensor& comp = std::get<0>(out);
  const at::Tensor host = std::get<1>(out).to(at::kCPU);
  TORCH_CHECK(host.size(0) == int64_t(tsIn.size()));
  return narrowRows(comp, host.data_ptr<int32_t>(), host.size(0), /*clone=*/true);
}

// ----------------------------------------------------------- decompress ----

// The dtype rule of a list of float tensors: `subject` must be float16,
// bfloat16, float32 or (with fp64) float64, and `sharers` must share a dtype,
// the list's first (a lone tensor is its own first).
struct DtypeRule {
  bool fp64;
  const char* subject;
  const char* sharers;
};
constexpr DtypeRule kFloatOutputs{true, "float outputs", "float outputs (ts_out)"};

void checkDtype(const at::Tensor& t, at::ScalarType first, const DtypeRule& r) {
  const auto d = t.scalar_type();
  TORCH_CHECK(d == at::kHalf || d == at::kBFloat16 || d == at::kFloat || (r.fp64 && d == at::kDouble), r.subject,
              " must be float16, bfloat16", r.fp64 ? ", float32 or float64" : " or float32");
  TORCH_CHECK(d == first, r.sharers, " must share a dtype");
}

at::ScalarType sharedDtype(const std::vector<at::Tensor>& ts, const DtypeRule& r) {
  for (const auto& t : ts) checkDtype(t, ts.front().scalar_type(), r);
  return ts.front().scalar_type();
}

// The device pointers of the optional out_status / out_decompressed_words
// tensors (n entries on `dev`), null when absent.
std::pair<uint8_t*, uint32_t*> statusPointers(const std::optional<at::Tensor>& status,
                                              const std::optional<at::Tensor>& sizes, int64_t n, int dev) {
  if (status) {
    TORCH_CHECK(status->is_contiguous() && status->device().type() == at::kCUDA && status->scalar_type() == at::kByte,
                "out_status must be a contiguous uint8 GPU tensor");
    TORCH_CHECK(status->numel() == n && status->get_device() == dev, "out_status must have ", n,
                " entries on the input device");
  }
  if (sizes) {
    TORCH_CHECK(sizes->is_contiguous() && sizes->device().type() == at::kCUDA && sizes->scalar_type() == at::kInt,
                "out_decompressed_words must be a contiguous int32 GPU tensor");
    TORCH_CHECK(sizes->numel() == n && sizes->get_device() == dev, "out_decompressed_words must have ", n,
                " entries on the input device");
  }
  return {status ? status->data_ptr<uint8_t>() : nullptr,
          sizes ? reinterpret_cast<uint32_t*>(sizes->data_ptr<int32_t>()) : nullptr};
}

// The member columns of a decode-side operator on device `dev`, filled one
// checked tensor at a time, so that an operator keeps the order of its
// members' checks: archive(t) appends a compressed input, dest(t, ...) a
// destination (`message` if it is no contiguous tensor on the device) with its
// capacity, which counts words of its dtype when asFloat and bytes otherwise.
// Under a `rule` the destinations share the first one's dtype: the config's
// float type is that one and every capacity is counted in words of it.
struct Members {
  const int dev;
  std::vector<const void*> in;
  std::vector<void*> out;
  std::vector<uint32_t> cap;
  at::ScalarType first = at::ScalarType::Undefined;
  Members(int d, size_t archives, size_t dests) : dev(d) {
    in.reserve(archives);
    out.reserve(dests);
    cap.reserve(dests);
  }
  void archive(const at::Tensor& t) {
    checkArchiveTensor(t, dev);
    in.push_back(t.data_ptr());
  }
  void dest(const at::Tensor& t, bool asFloat, const char* message, const DtypeRule* rule = nullptr) {
    checkDeviceTensor(t, dev, message);
    if (out.empty()) first = t.scalar_type();
    if (rule) checkDtype(t, first, *rule);
    const uint64_t c = asFloat ? uint64_t(t.numel()) : uint64_t(t.numel()) * t.element_size();
    TORCH_CHECK(c <= kU32Max);
    out.push_back(t.data_ptr());
    cap.push_back(uint32_t(c));
  }
};

void raiseOnChecksum(bool asFloat, bool mismatch) {
  if (!mismatch) return;
  if (asFloat) TORCH_CHECK(false, "floatDecompress: checksum mismatch seen on decoded data; archive cannot be unpacked");
  TORCH_CHECK(false, "ANSDecode: checksum mismatch seen on decoded data; archive cannot be unpacked");
}

// decompress_data_res, DietGpu.cpp:536-650: the full decode of the checked members
int64_t decompressRes(bool asFloat, CallContext& cx, Members& m, bool checksum, uint8_t* st, uint32_t* sz) {
  const auto n = uint32_t(m.in.size());
  if (asFloat) {
    const auto r = floatDecompress(*cx.res, floatConfig(floatTypeOf(m.first), checksum), n, m.in.data(),
                                   m.out.data(), m.cap.data(), st, sz, cx.stream);
    raiseOnChecksum(true, r.error != FloatDecompressError::None);
  } else {
    const auto r = ansDecodeBatchPointer(*cx.res, byteConfig(checksum), n, m.in.data(), m.out.data(), m.cap.data(),
                                         st, sz, cx.stream);
    raiseOnChecksum(false, r.error != ANSDecodeError::None);
  }
  return cx.used();
}

constexpr const char* kTsOutMessage = "ts_out must be contiguous GPU tensors on the input device";

// DietGpu.cpp:652-683
int64_t decompress_data(bool asFloat, const std::vector<at::Tensor>& tsIn, const std::vector<at::Tensor>& tsOut,
                        bool checksum, const std::optional<at::Tensor>& tempMem,
                        const std::optional<at::Tensor>& status, const std::optional<at::Tensor>& sizes) {
  CallContext cx(inputDevice(tsIn), tempMem);
  TORCH_CHECK(!tsIn.empty() && tsIn.size() == tsOut.size(), "ts_in and ts_out must have the same, nonzero length");
  Members m(cx.dev, tsIn.size(), tsIn.size());
  for (size_t i = 0; i < tsIn.size(); ++i) {
    m.archive(tsIn[i]);
    m.dest(tsOut[i], asFloat, kTsOutMessage, asFloat ? &kFloatOutputs : nullptr);
  }
  const auto [st, sz] = statusPointers(status, sizes, int64_t(tsIn.size()), cx.dev);
  return decompressRes(asFloat, cx, m, checksum, st, sz);
}

// Extension (no reference counterpart): words [t_first[i], t_first[i] +
// ts_out[i].numel()) of archive ts_in[i] into ts_out[i] (bytes of the element
// when !asFloat: the range is then first byte + ts_out[i]'s size in bytes).
int64_t decompress_data_range(bool asFloat, const std::vector<at::Tensor>& tsIn,
                              const std::vector<at::Tensor>& tsOut, const at::Tensor& tFirst,
                              const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& status,
                              const std::optional<at::Tensor>& sizes) {
  TORCH_CHECK(!tsIn.empty() && tsIn.size() == tsOut.size(), "ts_in and ts_out must have the same, nonzero length");
  CallContext cx(inputDevice(tsIn));
  TORCH_CHECK(tFirst.is_contiguous() && tFirst.device().type() == at::kCPU && tFirst.scalar_type() == at::kLong,
              "t_first must be a contiguous CPU int64 tensor");
  TORCH_CHECK(tFirst.numel() == int64_t(tsIn.size()), "one t_first entry per compressed input");
  const int64_t* fp = tFirst.data_ptr<int64_t>();
  std::vector<uint32_t> first(tsIn.size());
  // (the members' capacities are the ranges' counts)
  Members m(cx.dev, tsIn.size(), tsIn.size());
  for (size_t i = 0; i < tsIn.size(); ++i) {
    m.archive(tsIn[i]);
    m.dest(tsOut[i], asFloat, kTsOutMessage, asFloat ? &kFloatOutputs : nullptr);
    TORCH_CHECK(fp[i] >= 0 && uint64_t(fp[i]) <= kU32Max, "t_first[", i, "] = ", fp[i], " is outside [0, 2^32)");
    first[i] = uint32_t(fp[i]);
  }
  const auto [st, sz] = statusPointers(status, sizes, int64_t(tsIn.size()), cx.dev);
  cx.stack(tempMem);
  if (asFloat) {
    floatDecompressRange(*cx.res, floatConfig(floatTypeOf(m.first), false), uint32_t(tsIn.size()), m.in.data(),
                         first.data(), m.cap.data(), m.out.data(), st, sz, cx.stream);
  } else {
    ansDecodeBatchRange(*cx.res, byteConfig(false), uint32_t(tsIn.size()), m.in.data(), first.data(), m.cap.data(),
                        m.out.data(), st, sz, cx.stream);
  }
  return cx.used();
}

// float32 accumulators or outputs do not name their archives' type: fp32, or
// fp16 / bf16 with the sum kept in fp32.  Which of the three is read from the
// header of ts_in[0] = m.in[0]: one k_info launch and a 4-byte copy to the
// host, so such a call synchronises the stream once.  `who` ("... take")
// begins the refusal of a float64 archive.  Anything that is no float archive
// is taken as fp32 and fails on the device with status 0, like any other
// invalid member.
FloatType peekArchiveType(CallContext& cx, Members& m, const at::Tensor& tsIn0, const char* who) {
  at::Tensor type = at::zeros({1}, tsIn0.options().dtype(at::kInt));
  floatGetCompressedInfo(*cx.res, m.in.data(), 1, nullptr, reinterpret_cast<uint32_t*>(type.data_ptr<int32_t>()),
                         nullptr, cx.stream);
  const int32_t t0 = type.to(at::kCPU).data_ptr<int32_t>()[0];
  TORCH_CHECK(t0 != 4, who, " float16, bfloat16 or float32 archives; ts_in[0] is a float64 one");
  return t0 == 1 || t0 == 2 ? FloatType(t0) : FloatType::kFloat32;
}

// Extension (no reference counterpart): ts_acc[i] += the element that dense
// float archive ts_in[i] encodes, in place, in one kernel
// (floatDecompressAccumulate).  The accumulators share one dtype, which
// selects the mode: float16 / bfloat16 / float64 accumulators take archives
// of their own type; float32 accumulators take fp32 archives or, with the
// sum kept in fp32, fp16 / bf16 ones (peekArchiveType tells which).  A member
// whose archive has another type fails with status 0, as in decompress_data.
// No checksum flag: none can be verified, and archives written with one are
// accepted.
int64_t decompress_data_accumulate(const std::vector<at::Tensor>& tsIn, const std::vector<at::Tensor>& tsAcc,
                                   const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& status,
                                   const std::optional<at::Tensor>& sizes) {
  TORCH_CHECK(!tsIn.empty() && tsIn.size() == tsAcc.size(), "ts_in and ts_acc must have the same, nonzero length");
  const FloatType accType = floatTypeOf(sharedDtype(tsAcc, {true, "float outputs", "the accumulators (ts_acc)"}));
  CallContext cx(inputDevice(tsIn));
  Members m(cx.dev, tsIn.size(), tsIn.size());
  for (size_t i = 0; i < tsIn.size(); ++i) {
    m.archive(tsIn[i]);
    m.dest(tsAcc[i], /*asFloat=*/true, "ts_acc must be contiguous GPU tensors on the input device");
  }
  const auto [st, sz] = statusPointers(status, sizes, int64_t(tsIn.size()), cx.dev);
  cx.stack(tempMem);
  FloatType ft = accType;
  if (ft == FloatType::kFloat32) ft = peekArchiveType(cx, m, tsIn.front(), "float32 accumulators take");
  floatDecompressAccumulate(*cx.res, floatConfig(ft, false), uint32_t(tsIn.size()), m.in.data(), m.out.data(),
                            m.cap.data(), accType, st, sz, cx.stream);
  return cx.used();
}

// Extension (no reference counterpart): the fused multi-archive reduce
// (floatReduceArchives).  ts_in holds num_sources archives per member,
// source-major: archive k of member b is ts_in[k * len(ts_out) + b].
//   ts_out[b] = round((..(ts_init[b] + x_1) + ..) + x_K), every add in fp32
// in one kernel pass over the K archives (without ts_init the sum starts as
// x_1).  The outputs share one dtype, as do the inits: float16 / bfloat16
// name the archives' type themselves; when both are float32 (or there is no
// init and the outputs are float32) peekArchiveType reads it.  ts_out[b] may
// be ts_init[b].  A member with an invalid archive, archives of different
// sizes or a short output fails as a whole with status 0 and is left untouched.
int64_t reduce_data(const std::vector<at::Tensor>& tsIn, int64_t numSources, const std::vector<at::Tensor>& tsOut,
                    const std::optional<std::vector<at::Tensor>>& tsInit, const std::optional<at::Tensor>& tempMem,
                    const std::optional<at::Tensor>& status, const std::optional<at::Tensor>& sizes) {
  TORCH_CHECK(numSources >= 1 && numSources <= 64, "num_sources (", numSources, ") must be in 1 .. 64");
  TORCH_CHECK(!tsOut.empty() && int64_t(tsIn.size()) == numSources * int64_t(tsOut.size()),
              "ts_in must hold num_sources archives for each of the (one or more) ts_out");
  TORCH_CHECK(!tsInit || tsInit->size() == tsOut.size(), "ts_init and ts_out must have the same length");
  const at::ScalarType outD = sharedDtype(tsOut, {false, "ts_out", "ts_out"});
  const at::ScalarType initD = tsInit ? sharedDtype(*tsInit, {false, "ts_init", "ts_init"}) : outD;
  TORCH_CHECK(outD == at::kFloat || initD == at::kFloat || outD == initD,
              "ts_init and ts_out name different 16-bit archive types");
  CallContext cx(inputDevice(tsIn));
  const size_t nb = tsOut.size();
  Members m(cx.dev, tsIn.size(), nb);
  std::vector<const void*> init(tsInit ? nb : 0);
  for (const auto& ti : tsIn) m.archive(ti);
  for (size_t b = 0; b < nb; ++b) {
    m.dest(tsOut[b], /*asFloat=*/true, kTsOutMessage);
    if (tsInit) {
      const auto& ti = (*tsInit)[b];
      checkDeviceTensor(ti, cx.dev, "ts_init must be contiguous GPU tensors on the input device");
      // (a member whose element is longer than its init fails like one whose
      // output is short: the capacity covers both)
      m.cap[b] = uint32_t(std::min<int64_t>(tsOut[b].numel(), ti.numel()));
      init[b] = ti.data_ptr();
    }
  }
  const auto [st, sz] = statusPointers(status, sizes, int64_t(nb), cx.dev);
  cx.stack(tempMem);
  const FloatType outType = floatTypeOf(outD), initType = floatTypeOf(initD);
  FloatType ft = outType != FloatType::kFloat32 ? outType : initType;
  if (ft == FloatType::kFloat32) ft = peekArchiveType(cx, m, tsIn.front(), "reduce_data takes");
  floatReduceArchives(*cx.res, floatConfig(ft, false), uint32_t(nb), uint32_t(numSources), m.in.data(),
                      tsInit ? init.data() : nullptr, initType, m.out.data(), m.cap.data(), outType, st, sz,
                      cx.stream);
  return cx.used();
}

// Extension (no reference counterpart): rows t_idx[...] of the [R, row_words]
// table that archive t_in holds, into t_out [*t_idx.shape, row_words]
// (floatGatherRows / ansGatherRows).  t_idx is an int32 or int64 tensor on the
// archive's device: the call reads nothing back and uploads nothing.  t_out
// may be a view whose last dimension is contiguous and whose rows lie at a
// constant stride.  out_status[i] = 1 iff row t_idx[i] lies inside the
// element and the archive is valid; a failing row is left untouched.  The
// checks that need no device come first.
int64_t gather_rows(bool asFloat, const at::Tensor& tIn, int64_t rowWords, const at::Tensor& tIdx,
                    const at::Tensor& tOut, const std::optional<at::Tensor>& tempMem,
                    const std::optional<at::Tensor>& status) {
  TORCH_CHECK(rowWords >= 1 && uint64_t(rowWords) <= kU32Max, "row_words must be at least 1 (and below 2^32), not ",
              rowWords);
  TORCH_CHECK(tIdx.scalar_type() == at::kInt || tIdx.scalar_type() == at::kLong, "t_idx must be int32 or int64, not ",
              tIdx.scalar_type());
  if (asFloat) {
    checkDtype(tOut, tOut.scalar_type(), kFloatOutputs);
  } else {
    TORCH_CHECK(tOut.scalar_type() == at::kByte, "t_out must be uint8 in byte mode, not ", tOut.scalar_type());
  }
  const int64_t k = tIdx.dim();
  bool shapeOk = tOut.dim() == k + 1 && tOut.size(k) == rowWords;
  for (int64_t d = 0; shapeOk && d < k; ++d) shapeOk = tOut.size(d) == tIdx.size(d);
  TORCH_CHECK(shapeOk, "t_out must have the shape [*t_idx.shape, row_words] = [", tIdx.sizes(), ", ", rowWords,
              "], not ", tOut.sizes());
  // rows at one stride: leading dimension d strides over the rows inside it
  TORCH_CHECK(rowWords == 1 || tOut.stride(k) == 1, "t_out's last dimension must be contiguous");
  int64_t rowStride = -1, inner = 1;
  for (int64_t d = k - 1; d >= 0; --d) {
    if (tOut.size(d) != 1) {
      if (rowStride < 0) rowStride = tOut.stride(d);
      else TORCH_CHECK(tOut.stride(d) == rowStride * inner, "t_out's rows must lie at a constant stride");
    }
    inner *= tOut.size(d);
  }
  if (rowStride < 0) rowStride = rowWords;
  TORCH_CHECK(rowStride >= rowWords, "t_out's rows must not overlap (row stride ", rowStride, " < row_words)");
  TORCH_CHECK(uint64_t(tIdx.numel()) <= kU32Max, "too many indices");
  TORCH_CHECK(tIdx.device().type() == at::kCUDA && tIdx.is_contiguous(),
              "t_idx must be a contiguous GPU tensor (on the archive's device)");
  const int dev = tIdx.get_device();
  checkArchiveTensor(tIn, dev);
  TORCH_CHECK(tOut.device().type() == at::kCUDA && tOut.get_device() == dev, "t_out must be on the archive's device");
  CallContext cx(dev);
  const auto st = statusPointers(status, std::nullopt, tIdx.numel(), dev).first;
  cx.stack(tempMem);
  const bool is64 = tIdx.scalar_type() == at::kLong;
  if (asFloat) {
    floatGatherRows(*cx.res, floatConfig(floatTypeOf(tOut.scalar_type()), false), tIn.data_ptr(), uint32_t(rowWords),
                    uint32_t(tIdx.numel()), tIdx.data_ptr(), is64, tOut.data_ptr(), uint64_t(rowStride), st,
                    cx.stream);
  } else {
    ansGatherRows(*cx.res, byteConfig(false), tIn.data_ptr(), uint32_t(rowWords), uint32_t(tIdx.numel()),
                  tIdx.data_ptr(), is64, tOut.data_ptr(), uint64_t(rowStride), st, cx.stream);
  }
  return cx.used();
}

// Extension (no reference counterpart): embedding_bag(mode="sum") on a
// compressed table (floatGatherRowsSum).  Bag b is t_idx[t_offsets[b] ..
// t_offsets[b + 1]) (t_offsets holds B + 1 boundaries; both tensors int32 or
// both int64, on the archive's device) and t_out [B, row_words] row b the fp32
// sum of the bag's rows in list order, started from the first row and rounded
// once to t_out's dtype; an empty bag gives +0.0.  float16 / bfloat16 outputs
// name the archive's type themselves; for float32 outputs peekArchiveType
// reads it (fp32, or fp16 / bf16 summed into fp32), which synchronises the
// stream once.  out_status[b] = 1 iff the archive is valid, the bag's offsets
// are ordered and inside t_idx and all its rows lie inside the element; a
// failing bag's row is left untouched.  t_out's rows may lie at a stride.  The
// checks that need no device come first.
int64_t gather_rows_sum(const at::Tensor& tIn, int64_t rowWords, const at::Tensor& tIdx, const at::Tensor& tOffsets,
                        const at::Tensor& tOut, const std::optional<at::Tensor>& tempMem,
                        const std::optional<at::Tensor>& status) {
  TORCH_CHECK(rowWords >= 1 && uint64_t(rowWords) <= kU32Max, "row_words must be at least 1 (and below 2^32), not ",
              rowWords);
  TORCH_CHECK(tIdx.scalar_type() == at::kInt || tIdx.scalar_type() == at::kLong, "t_idx must be int32 or int64, not ",
              tIdx.scalar_type());
  TORCH_CHECK(tOffsets.scalar_type() == tIdx.scalar_type(), "t_offsets must have t_idx's dtype (", tIdx.scalar_type(),
              "), not ", tOffsets.scalar_type());
  TORCH_CHECK(tIdx.dim() == 1 && tOffsets.dim() == 1 && tOffsets.numel() >= 1,
              "t_idx and t_offsets must be 1-d, t_offsets with B + 1 >= 1 entries");
  checkDtype(tOut, tOut.scalar_type(), {false, "t_out", "t_out"});
  const int64_t bags = tOffsets.numel() - 1;
  TORCH_CHECK(tOut.dim() == 2 && tOut.size(0) == bags && tOut.size(1) == rowWords,
              "t_out must have the shape [t_offsets.numel() - 1, row_words] = [", bags, ", ", rowWords, "], not ",
              tOut.sizes());
  TORCH_CHECK(rowWords == 1 || tOut.stride(1) == 1, "t_out's last dimension must be contiguous");
  const int64_t rowStride = bags > 1 ? tOut.stride(0) : rowWords;
  TORCH_CHECK(rowStride >= rowWords, "t_out's rows must not overlap (row stride ", rowStride, " < row_words)");
  TORCH_CHECK(uint64_t(tIdx.numel()) <= kU32Max && uint64_t(bags) <= kU32Max, "too many indices or bags");
  TORCH_CHECK(tOffsets.device().type() == at::kCUDA && tOffsets.is_contiguous() &&
                  tIdx.device().type() == at::kCUDA && tIdx.is_contiguous() &&
                  tIdx.get_device() == tOffsets.get_device(),
              "t_idx and t_offsets must be contiguous GPU tensors (on the archive's device)");
  const int dev = tOffsets.get_device();
  CallContext cx(dev);
  Members m(dev, 1, 0);
  m.archive(tIn);
  TORCH_CHECK(tOut.device().type() == at::kCUDA && tOut.get_device() == dev, "t_out must be on the archive's device");
  const auto st = statusPointers(status, std::nullopt, bags, dev).first;
  cx.stack(tempMem);
  const FloatType outType = floatTypeOf(tOut.scalar_type());
  FloatType ft = outType;
  if (ft == FloatType::kFloat32) ft = peekArchiveType(cx, m, tIn, "gather_rows_sum takes");
  floatGatherRowsSum(*cx.res, floatConfig(ft, false), tIn.data_ptr(), uint32_t(rowWords), uint32_t(bags),
                     uint32_t(tIdx.numel()), tIdx.data_ptr(), tOffsets.data_ptr(), tIdx.scalar_type() == at::kLong,
                     tOut.data_ptr(), outType == FloatType::kFloat32, uint64_t(rowStride), st, cx.stream);
  return cx.used();
}

// DietGpu.cpp:685-832
int64_t decompress_data_split_size(bool asFloat, const std::vector<at::Tensor>& tsIn, const at::Tensor& tOut,
                                   const at::Tensor& tSplit, bool checksum, const std::optional<at::Tensor>& tempMem,
                                   const std::optional<at::Tensor>& status, const std::optional<at::Tensor>& sizes) {
  CallContext cx(inputDevice(tsIn));
  SplitSizes split(tSplit, "t_out_split_sizes");
  const int64_t n = split.n;
  TORCH_CHECK(n == int64_t(tsIn.size()), "one split size per compressed input");
  Members m(cx.dev, tsIn.size(), 0);
  for (int64_t i = 0; i < n; ++i) {
    m.archive(tsIn[size_t(i)]);
    split.take(i);
  }
  checkDeviceTensor(tOut, cx.dev, "t_out must be a contiguous GPU tensor on the input device");
  if (asFloat) checkDtype(tOut, tOut.scalar_type(), kFloatOutputs);
  checkSplitSum(split.sum, tOut, asFloat, "t_out");
  const auto [st, sz] = statusPointers(status, sizes, n, cx.dev);
  cx.stack(tempMem);
  if (asFloat) {
    const auto r = floatDecompressSplitSize(*cx.res, floatConfig(floatTypeOf(tOut.scalar_type()), checksum),
                                            uint32_t(n), m.in.data(), tOut.data_ptr(), split.data(), st, sz, cx.stream);
    raiseOnChecksum(true, r.error != FloatDecompressError::None);
  } else {
    const auto r = ansDecodeBatchSplitSize(*cx.res, byteConfig(checksum), uint32_t(n), m.in.data(), tOut.data_ptr(),
                                           split.data(), st, sz, cx.stream);
    raiseOnChecksum(false, r.error != ANSDecodeError::None);
  }
  return cx.used();
}

// DietGpu.cpp:834-917
std::vector<at::Tensor> decompress_data_simple(bool asFloat, const std::vector<at::Tensor>& tsIn, bool checksum,
                                               std::optional<int64_t> tempMem) {
  std::optional<at::Tensor> scratch;  // (declared first: it outlives the arena over it)
  CallContext cx(inputDevice(tsIn));
  const auto n = int64_t(tsIn.size());
  Members m(cx.dev, tsIn.size(), tsIn.size());
  for (const auto& t : tsIn) m.archive(t);  // (checked once, before k_info reads the headers)
  if (tempMem && *tempMem >= int64_t(kSDMAlignment)) {
    scratch = at::empty({*tempMem}, tsIn.front().options().dtype(at::kByte));
  }
  at::Tensor info = at::zeros({2, n}, tsIn.front().options().dtype(at::kInt));
  cx.stack(scratch);
  auto* sizesDev = reinterpret_cast<uint32_t*>(info.data_ptr<int32_t>());
  if (asFloat) {
    floatGetCompressedInfo(*cx.res, m.in.data(), uint32_t(n), sizesDev, sizesDev + n, nullptr, cx.stream);
  } else {
    ansGetCompressedInfo(*cx.res, m.in.data(), uint32_t(n), sizesDev, nullptr, cx.stream);
  }
  const at::Tensor host = info.to(at::kCPU);
  const int32_t* h = host.data_ptr<int32_t>();
  std::vector<at::Tensor> outs;
  outs.reserve(tsIn.size());
  for (int64_t i = 0; i < n; ++i) {
    const int64_t size = h[i];
    if (asFloat) {
      const uint32_t ty = uint32_t(h[n + i]);
      TORCH_CHECK(ty == uint32_t(h[n]), "all archives must have the same float type");
      outs.push_back(at::empty({size}, tsIn.front().options().dtype(dtypeOf(ty))));
    } else {
      outs.push_back(at::empty({size}, tsIn.front().options().dtype(at::kByte)));
    }
    m.dest(outs.back(), asFloat, kTsOutMessage);
  }
  decompressRes(asFloat, cx, m, checksum, nullptr, nullptr);
  return outs;
}

}  // namespace
}  // namespace dietgpu

// DietGpu.cpp:921-978: schemas identical to the reference's
TORCH_LIBRARY(dietgpu, m) {
  m.def("max_float_compressed_output_size(Tensor[] ts) -> (int, int)");
  m.def("max_float_compressed_size(Tensor dtype, int size) -> int");
  m.def("max_any_compressed_output_size(Tensor[] ts) -> (int, int)");
  m.def("max_any_compressed_size(int bytes) -> int");
  m.def(
      "compress_data(bool compress_as_float, Tensor[] ts_in, bool checksum=False, Tensor? temp_mem=None, "
      "Tensor? out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor, Tensor, int)");
  m.def(
      "compress_data_split_size(bool compress_as_float, Tensor t_in, Tensor t_in_split_sizes, bool checksum=False, "
      "Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor[], Tensor, "
      "int)");
  m.def(
      "compress_data_simple(bool compress_as_float, Tensor[] ts_in, bool checksum=False, int? temp_mem=67108864) -> "
      "Tensor[]");
  m.def(
      "decompress_data(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, bool checksum=False, Tensor? "
      "temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> (int)");
  m.def(
      "decompress_data_split_size(bool compress_as_float, Tensor[] ts_in, Tensor t_out, Tensor t_out_split_sizes, "
      "bool checksum=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> "
      "(int)");
  m.def(
      "decompress_data_simple(bool compress_as_float, Tensor[] ts_in, bool checksum=False, int? temp_mem=67108864) "
      "-> Tensor[]");
  // extension: not one of the reference's ten operators
  m.def(
      "decompress_data_range(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, Tensor t_first, Tensor? "
      "temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> int");
  m.def(
      "decompress_data_accumulate(Tensor[] ts_in, Tensor[] ts_acc, Tensor? temp_mem=None, Tensor? out_status=None, "
      "Tensor? out_sizes=None) -> int");
  m.def(
      "gather_rows(bool compress_as_float, Tensor t_in, int row_words, Tensor t_idx, Tensor t_out, Tensor? "
      "temp_mem=None, Tensor? out_status=None) -> int");
  m.def(
      "reduce_data(Tensor[] ts_in, int num_sources, Tensor[] ts_out, Tensor[]? ts_init=None, Tensor? temp_mem=None, "
      "Tensor? out_status=None, Tensor? out_sizes=None) -> int");
  m.def(
      "gather_rows_sum(Tensor t_in, int row_words, Tensor t_idx, Tensor t_offsets, Tensor t_out, Tensor? "
      "temp_mem=None, Tensor? out_status=None) -> int");
}

TORCH_LIBRARY_IMPL(dietgpu, CompositeExplicitAutograd, m) {
  m.impl("max_float_compressed_output_size", &dietgpu::max_float_compressed_output_size);
  m.impl("max_float_compressed_size", &dietgpu::max_float_compressed_size);
  m.impl("max_any_compressed_output_size", &dietgpu::max_any_compressed_output_size);
  m.impl("max_any_compressed_size", &dietgpu::max_any_compressed_size);
  m.impl("compress_data", &dietgpu::compress_data);
  m.impl("compress_data_split_size", &dietgpu::compress_data_split_size);
  m.impl("compress_data_simple", &dietgpu::compress_data_simple);
  m.impl("decompress_data", &dietgpu::decompress_data);
  m.impl("decompress_data_split_size", &dietgpu::decompress_data_split_size);
  m.impl("decompress_data_simple", &dietgpu::decompress_data_simple);
  m.impl("decompress_data_range", &dietgpu::decompress_data_range);
  m.impl("decompress_data_accumulate", &dietgpu::decompress_data_accumulate);
  m.impl("gather_rows", &dietgpu::gather_rows);
  m.impl("reduce_data", &dietgpu::reduce_data);
  m.impl("gather_rows_sum", &dietgpu::gather_rows_sum);
}
