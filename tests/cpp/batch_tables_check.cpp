// Host-only check of the batch-table builder (csrc/batch_tables.h), meant to
// run under AddressSanitizer / UBSan without a GPU: the "device" arena is a
// host buffer and the upload a memcpy.  Not part of the library build:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//     -I include -I dietgpu_fork_amd/csrc tests/cpp/batch_tables_check.cpp \
//     dietgpu_fork_amd/csrc/stack_memory.cpp -o batch_tables_check && ./batch_tables_check
// Pointer-, split- and sparse-shaped tables at batch sizes on both sides of
// the 8 KB inline limit: entries, tags, and DeviceDescs::map (the one-element
// stride mapping, the rebased device copy).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_tables.h"

namespace dietgpu {
// stands in for upload.hip
bool uploadViaKernargs(void* dst, const void* src, size_t bytes, hipStream_t) {
  std::memcpy(dst, src, bytes);
  return true;
}
}  // namespace dietgpu

using namespace dietgpu;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: nb=%u: %s\n", __FILE__, __LINE__, gNb, #c); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)
static uint32_t gNb = 0;

// entry i of a table column, wherever the table lives
template <typename T>
static T entry(const DeviceTables& t, const T* col, uint32_t i) {
  const uintptr_t base = t.inl ? reinterpret_cast<uintptr_t>(t.image->w) : 0;
  T v;
  std::memcpy(&v, reinterpret_cast<const void*>(base + reinterpret_cast<uintptr_t>(col) + i * sizeof(T)), sizeof(T));
  return v;
}

// what a kernel's BatchDesc::start / size would see for a mapped descriptor
static uint64_t startOf(const BatchDesc& d, uint32_t b) {
  if (d.mode == BatchDesc::kPointer) return d.ptrs[b];
  if (d.mode == BatchDesc::kSplit) return reinterpret_cast<uint64_t>(d.base) + d.offsets[b];
  return reinterpret_cast<uint64_t>(d.base) + d.stride * b;
}
static uint32_t sizeOf(const BatchDesc& d, uint32_t b) { return d.sizes ? d.sizes[b] : d.fixedSize; }

static void checkBatch(StackDeviceMemory& res, uint32_t nb, int nCols, uint32_t unit) {
  gNb = nb;
  std::vector<std::vector<uint64_t>> cols(nCols, std::vector<uint64_t>(nb));
  std::vector<uint32_t> raw(nb);
  for (uint32_t i = 0; i < nb; ++i) {
    raw[i] = 1 + (i * 2654435761u) % 5000;
    for (int c = 0; c < nCols; ++c) cols[c][i] = 0x100000ull * (c + 1) + 48ull * i + (c == 0 && i == 3 ? 8 : 0);
  }
  const SizeColumn sz(raw.data(), nb);
  uint32_t mx = 0;
  for (uint32_t v : raw) mx = std::max(mx, v);
  REQUIRE(sz.maxSize == mx && sz.sizes == raw);
  REQUIRE(allAligned16(cols[0]) == (nb <= 3));

  // split offsets
  const SplitColumns sc(raw.data(), nb, unit);
  uint64_t run = 0;
  bool al = true;
  for (uint32_t i = 0; i < nb; ++i) {
    REQUIRE(sc.offsets[i] == run * unit);
    al = al && (run * unit) % 16 == 0;
    run += raw[i];
  }
  REQUIRE(sc.aligned16 == al && sc.maxSize == mx);

  const size_t avail = res.getSizeAvailable();
  {
    // pointer- (2 columns) or sparse-shaped (3 columns) table
    DeviceTables t = nCols == 3 ? uploadTables(res, nullptr, {&cols[0], &cols[1], &cols[2]}, sz.sizes, true)
                                : uploadTables(res, nullptr, {&cols[0], &cols[1]}, sz.sizes, true);
    const size_t bytes = size_t(nb) * (8 * nCols + 4);
    REQUIRE(t.host.size() == bytes && int(t.u64.size()) == nCols);
    REQUIRE(t.inl == (kInlineBias + bytes <= sizeof(InlineTable)));
    REQUIRE((res.getSizeAvailable() == avail) == t.inl);  // inline: no device table
    for (uint32_t i = 0; i < nb; ++i) {
      for (int c = 0; c < nCols; ++c) REQUIRE(entry(t, t.u64[c], i) == cols[c][i]);
      REQUIRE(entry(t, t.u32, i) == raw[i]);
    }
    const BatchDesc in = t.tag(BatchDesc::pointers(t.u64[0], t.u32));
    const BatchDesc out = t.tag(BatchDesc::pointers(t.u64[nCols - 1], nullptr));
    REQUIRE(in.inl == (t.inl ? (BatchDesc::kInlPtrs | BatchDesc::kInlSizes) : 0u));
    REQUIRE(out.inl == (t.inl ? uint32_t(BatchDesc::kInlPtrs) : 0u));
    const size_t before = res.getSizeAvailable();
    {
      const DeviceDescs dd(res, nullptr, &t, nb);
      REQUIRE((res.getSizeAvailable() == before) == (!t.inl || nb == 1));  // one copy, never for one element
      const BatchDesc mi = dd.map(in), mo = dd.map(out);
      REQUIRE(mi.inl == 0 && mo.inl == 0);
      if (nb == 1 && t.inl) REQUIRE(mi.mode == BatchDesc::kStride && mi.stride == 0 && mi.sizes == nullptr);
      for (uint32_t i = 0; i < nb; ++i) {
        REQUIRE(startOf(mi, i) == cols[0][i] && sizeOf(mi, i) == raw[i]);
        REQUIRE(startOf(mo, i) == cols[nCols - 1][i] && sizeOf(mo, i) == 0);
      }
    }
    REQUIRE(res.getSizeAvailable() == before);
  }
  {
    // split-shaped table (offsets, sizes) over a base buffer
    uint8_t* const base = reinterpret_cast<uint8_t*>(0x7000000);
    DeviceTables t = uploadTables(res, nullptr, {&sc.offsets}, sc.sizes, true);
    const BatchDesc in = t.tag(BatchDesc::split(base, t.u64[0], t.u32));
    REQUIRE(in.inl == (t.inl ? (BatchDesc::kInlOffsets | BatchDesc::kInlSizes) : 0u));
    const DeviceDescs dd(res, nullptr, &t, nb);
    const BatchDesc m = dd.map(in);
    REQUIRE(m.inl == 0);
    for (uint32_t i = 0; i < nb; ++i)
      REQUIRE(startOf(m, i) == reinterpret_cast<uint64_t>(base) + sc.offsets[i] && sizeOf(m, i) == raw[i]);
  }
  {
    // a lone pointer column, never inline (the *GetCompressedInfo upload)
    DeviceTables t = uploadTables(res, nullptr, {&cols[0]}, {});
    REQUIRE(!t.inl && t.host.size() == size_t(nb) * 8);
    for (uint32_t i = 0; i < nb; ++i) REQUIRE(t.u64[0][i] == cols[0][i]);
  }
  REQUIRE(res.getSizeAvailable() == avail);  // everything released, in stack order
}

// The sparse compressor's batch through the shared pointerBatch: inputs,
// archives and, as the third column, the dense archives at out[i] +
// prefix(size[i]); mapped for the sparse kernels by DeviceDescs (one element:
// stride descriptors, nothing uploaded).
static uint64_t prefixOf(uint32_t n) { return 16 + (uint64_t(n) + 7) / 8; }

static void checkSparseCompressBatch(StackDeviceMemory& res, uint32_t nb, uint32_t unit) {
  gNb = nb;
  std::vector<const void*> in(nb);
  std::vector<void*> out(nb);
  std::vector<uint32_t> raw(nb);
  uint32_t mx = 0;
  for (uint32_t i = 0; i < nb; ++i) {
    raw[i] = (i * 2654435761u) % 70000;  // element 0 is empty
    mx = std::max(mx, raw[i]);
    in[i] = reinterpret_cast<const void*>(0x100000ull + 80ull * unit * i + (i == 3 ? unit : 0));
    out[i] = reinterpret_cast<void*>(0x40000000ull + 0x10000ull * i);
  }
  const size_t avail = res.getSizeAvailable();
  {
    const BatchTables b = pointerBatch(res, nullptr, nb, in.data(), out.data(), raw.data(), true, unit, prefixOf);
    const size_t bytes = size_t(nb) * 28;
    REQUIRE(b.t.host.size() == bytes && b.t.u64.size() == 3);
    REQUIRE(b.t.inl == (kInlineBias + bytes <= sizeof(InlineTable)));
    REQUIRE((res.getSizeAvailable() == avail) == b.t.inl);
    REQUIRE(b.maxSize == mx && b.inAligned16 == (nb <= 3));
    const uint32_t tagged = b.t.inl ? uint32_t(BatchDesc::kInlPtrs) : 0u;
    REQUIRE(b.in.inl == (b.t.inl ? (BatchDesc::kInlPtrs | BatchDesc::kInlSizes) : 0u));
    REQUIRE(b.out.inl == tagged && b.out2.inl == tagged);
    for (uint32_t i = 0; i < nb; ++i) {
      REQUIRE(entry(b.t, b.t.u64[0], i) == reinterpret_cast<uint64_t>(in[i]));
      REQUIRE(entry(b.t, b.t.u64[1], i) == reinterpret_cast<uint64_t>(out[i]));
      REQUIRE(entry(b.t, b.t.u64[2], i) == reinterpret_cast<uint64_t>(out[i]) + prefixOf(raw[i]));
      REQUIRE(entry(b.t, b.t.u32, i) == raw[i]);
    }
    const size_t before = res.getSizeAvailable();
    {
      const DeviceDescs dd(res, nullptr, &b.t, nb);
      REQUIRE((res.getSizeAvailable() == before) == (!b.t.inl || nb == 1));
      const BatchDesc mi = dd.map(b.in), mo = dd.map(b.out), md = dd.map(b.out2);
      REQUIRE(mi.inl == 0 && mo.inl == 0 && md.inl == 0);
      if (nb == 1) REQUIRE(mi.mode == BatchDesc::kStride && mo.mode == BatchDesc::kStride && md.mode == BatchDesc::kStride);
      for (uint32_t i = 0; i < nb; ++i) {
        REQUIRE(startOf(mi, i) == reinterpret_cast<uint64_t>(in[i]) && sizeOf(mi, i) == raw[i]);
        REQUIRE(startOf(mo, i) == reinterpret_cast<uint64_t>(out[i]) && sizeOf(mo, i) == 0);
        REQUIRE(startOf(md, i) == reinterpret_cast<uint64_t>(out[i]) + prefixOf(raw[i]) && sizeOf(md, i) == 0);
      }
    }
    REQUIRE(res.getSizeAvailable() == before);
  }
  REQUIRE(res.getSizeAvailable() == avail);
  // the alignment checks: the input to its unit, the archive to 16 bytes
  auto refused = [&](const void* i0, void* o0) {
    const void* ii[1] = {i0};
    void* oo[1] = {o0};
    try {
      pointerBatch(res, nullptr, 1, ii, oo, raw.data(), true, unit, prefixOf);
    } catch (const DietGpuError&) {
      return true;
    }
    return false;
  };
  REQUIRE(!refused(in[0], out[0]) && refused(in[0], static_cast<uint8_t*>(out[0]) + 8));
  REQUIRE(refused(static_cast<const uint8_t*>(in[0]) + 1, out[0]) == (unit > 1));
  REQUIRE(res.getSizeAvailable() == avail);
}

int main() {
  std::vector<uint8_t> arena((1 << 20) + kSDMAlignment);
  StackDeviceMemory res(0, arena.data(), arena.size());
  for (uint32_t nb : {1u, 2u, 4u, 292u, 293u, 400u})
    for (uint32_t unit : {2u, 4u, 8u}) checkSparseCompressBatch(res, nb, unit);
  // 1, 2; 400 / 401; the inline limits of 28-, 20- and 12-byte entries
  for (uint32_t nb : {1u, 2u, 4u, 292u, 293u, 400u, 401u, 409u, 410u, 682u, 683u})
    for (int nCols : {2, 3})
      for (uint32_t unit : {1u, 2u, 4u, 8u}) checkBatch(res, nb, nCols, unit);
  std::puts("batch tables ok");
  return 0;
}
