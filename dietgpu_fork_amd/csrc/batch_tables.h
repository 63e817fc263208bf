// Per-call parameter tables of a batch (the reference's BatchProvider pointer /
// size arrays), built on the host by every pointer and split-size entry point
// of the dense and sparse codecs.  Host code only.
//
// Small tables (allowInline, <= 8 KB) ride in the InlineTable kernel argument
// of k_pcompress / k_decode: the BatchDesc fields then hold byte offsets into
// it (biased by 8, so none is 0) and BatchDesc::inl says which.  Any other
// kernel gets a device copy made in its driver's scope (DeviceDescs).  Larger
// tables, or callers that need device pointers, get one upload here.
#pragma once

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <type_traits>
#include <vector>

#include "batch.h"
#include "common.h"
#include "dietgpu/StackDeviceMemory.h"

namespace dietgpu {

struct DeviceTables {
  GpuMemoryReservation<uint8_t> mem;
  std::vector<uint8_t> host;
  std::unique_ptr<InlineTable> image;  // kernarg image when inline
  bool inl = false;
  std::vector<const uint64_t*> u64;  // the u64 columns, in the order given
  const uint32_t* u32 = nullptr;     // the u32 column that follows them
  const uint32_t* u32b = nullptr;    // the second u32 column (range decode: `first`), if given

  // mark the table-backed fields of a descriptor built from u64 / u32
  BatchDesc tag(BatchDesc d) const {
    if (!inl) return d;
    if (d.ptrs) d.inl |= BatchDesc::kInlPtrs;
    if (d.sizes) d.inl |= BatchDesc::kInlSizes;
    if (d.offsets) d.inl |= BatchDesc::kInlOffsets;
    return d;
  }
};
constexpr size_t kInlineBias = 8;

inline const InlineTable& kernargTable(const DeviceTables* t) {
  static const InlineTable kEmpty{};
  return t && t->inl ? *t->image : kEmpty;
}

// One table of the u64 columns `cols` followed by the u32 column `last`
// (either may be empty) and, if given, a second u32 column `last2`.
inline DeviceTables uploadTables(StackDeviceMemory& res, hipStream_t s,
                                 std::initializer_list<const std::vector<uint64_t>*> cols,
                                 const std::vector<uint32_t>& last, bool allowInline = false,
                                 const std::vector<uint32_t>* last2 = nullptr) {
  DeviceTables t;
  size_t bytes = last.size() * 4 + (last2 ? last2->size() * 4 : 0);
  for (const auto* c : cols) bytes += c->size() * 8;
  t.host.resize(bytes);
  size_t off = 0;  // column offsets now, addresses once the base is known
  for (const auto* c : cols) {
    t.u64.push_back(reinterpret_cast<const uint64_t*>(off));
    if (!c->empty()) std::memcpy(t.host.data() + off, c->data(), c->size() * 8);
    off += c->size() * 8;
  }
  if (!last.empty()) std::memcpy(t.host.data() + off, last.data(), last.size() * 4);
  const size_t off2 = off + last.size() * 4;
  if (last2 && !last2->empty()) std::memcpy(t.host.data() + off2, last2->data(), last2->size() * 4);
  t.inl = allowInline && kInlineBias + bytes <= sizeof(InlineTable);
  uintptr_t base;
  if (t.inl) {
    t.image.reset(new InlineTable());
    std::memcpy(reinterpret_cast<uint8_t*>(t.image->w) + kInlineBias, t.host.data(), bytes);
    base = kInlineBias;
  } else {
    t.mem = res.alloc<uint8_t>(s, std::max<size_t>(bytes, 1));
    StackDeviceMemory::copyToDevice(t.mem.data(), t.host.data(), bytes, s);
    base = reinterpret_cast<uintptr_t>(t.mem.data());
  }
  for (auto& p : t.u64) p = reinterpret_cast<const uint64_t*>(base + reinterpret_cast<uintptr_t>(p));
  t.u32 = reinterpret_cast<const uint32_t*>(base + off);
  if (last2) t.u32b = reinterpret_cast<const uint32_t*>(base + off2);
  return t;
}

// The addresses of a host array of nb pointers, as a table column.
template <typename P>
std::vector<uint64_t> addressColumn(P* const* p, uint32_t nb) {
  std::vector<uint64_t> v(nb);
  for (uint32_t i = 0; i < nb; ++i) v[i] = reinterpret_cast<uint64_t>(p[i]);
  return v;
}

inline bool allAligned16(const std::vector<uint64_t>& addrs) {
  for (uint64_t a : addrs)
    if (a % 16) return false;
  return true;
}

// A u32 column (sizes or capacities) and its largest entry.
struct SizeColumn {
  std::vector<uint32_t> sizes;
  uint32_t maxSize = 0;
  SizeColumn(const uint32_t* v, uint32_t nb) : sizes(v, v + nb) {
    for (uint32_t x : sizes) maxSize = std::max(maxSize, x);
  }
};

// The columns of a split-size batch: element i starts `unitBytes` x (the sum
// of the earlier sizes) bytes into the base buffer.  aligned16: every offset
// is a multiple of 16.
struct SplitColumns : SizeColumn {
  std::vector<uint64_t> offsets;
  bool aligned16 = true;
  SplitColumns(const uint32_t* v, uint32_t nb, uint32_t unitBytes) : SizeColumn(v, nb), offsets(nb) {
    uint64_t run = 0;
    for (uint32_t i = 0; i < nb; ++i) {
      offsets[i] = run * unitBytes;
      run += sizes[i];
    }
    aligned16 = allAligned16(offsets);
  }
};

inline void checkOutAligned(const void* p, const char* what) {
  DG_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0,
           what << " must be 16-byte aligned (archives are written with 16 B stores)");
}

// Archive i of a range or accumulate call: 4-byte aligned for a dense archive
// (the decoder reads the headers with scalar loads, which drop the low two
// address bits; the full decoders do not check this), 16-byte for a sparse one
// (the compressor requires it of its output; the bitmap is read as u64).
inline void checkArchiveAligned(uint64_t address, uint32_t i, uint32_t align) {
  DG_CHECK(address % align == 0, "archive " << i << " must be " << align << "-byte aligned");
}

// The tables of a batch and the descriptors that refer to them.
struct BatchTables {
  DeviceTables t;
  BatchDesc in, out;
  BatchDesc out2;            // pointerBatch's extra column, if asked for
  uint32_t maxSize = 0;      // the largest size (compress) or capacity (decode)
  bool inAligned16 = false;  // compress: every input starts 16 B-aligned
};

// in[i] -> out[i]; `sizes` are the inputs' sizes (compress) or the outputs'
// capacities (decode).  `unit` is the size of the codec's unit in bytes: 1 for
// the byte codec, the word size for the float codec (whose pointers must be
// aligned to it; 1 checks nothing).  out2Offset (the sparse compressor's): a
// third address column, out[i] + out2Offset(sizes[i]), as BatchTables::out2.
inline BatchTables pointerBatch(StackDeviceMemory& res, hipStream_t s, uint32_t nb, const void** in, void** out,
                                const uint32_t* sizes, bool compress, uint32_t unit,
                                uint64_t (*out2Offset)(uint32_t) = nullptr) {
  const auto ip = addressColumn(in, nb), op = addressColumn(out, nb);
  for (uint32_t i = 0; i < nb; ++i) {
    if (compress) {
      DG_CHECK(ip[i] % unit == 0, "float input " << i << " not aligned to its word size");
      checkOutAligned(out[i], "out[i]");
    } else {
      DG_CHECK(op[i] % unit == 0, "float output " << i << " not aligned to its word size");
    }
  }
  const SizeColumn sz(sizes, nb);
  BatchTables b;
  if (out2Offset) {
    std::vector<uint64_t> op2(nb);
    for (uint32_t i = 0; i < nb; ++i) op2[i] = op[i] + out2Offset(sz.sizes[i]);
    b.t = uploadTables(res, s, {&ip, &op, &op2}, sz.sizes, true);
    b.out2 = b.t.tag(BatchDesc::pointers(b.t.u64[2], nullptr));
  } else {
    b.t = uploadTables(res, s, {&ip, &op}, sz.sizes, true);
  }
  b.in = b.t.tag(BatchDesc::pointers(b.t.u64[0], compress ? b.t.u32 : nullptr));
  b.out = b.t.tag(BatchDesc::pointers(b.t.u64[1], compress ? nullptr : b.t.u32));
  b.maxSize = sz.maxSize;
  b.inAligned16 = allAligned16(ip);
  return b;
}

// Device copy of inline tables for kernels without an InlineTable argument,
// allocated in the calling driver's scope (the arena is LIFO) and only when
// the tables are inline.  A one-element batch needs no copy at all: its
// descriptors become stride descriptors of that element (its address, and
// its size as the fixed size), so the three-kernel path of a batch-1
// pointer / split-size call launches no upload kernel (fp64 1 x 16M words
// and the float_benchmark's batch-1 grid: a 4.7 us k_table launch before
// k_hist).
struct DeviceDescs {
  GpuMemoryReservation<uint8_t> mem;
  uintptr_t base = 0;
  const InlineTable* single = nullptr;  // nb == 1: entries read from the kernarg image
  DeviceDescs(StackDeviceMemory& res, hipStream_t s, const DeviceTables* t, uint32_t nb) {
    if (!t || !t->inl) return;
    if (nb == 1) {
      single = t->image.get();
      return;
    }
    mem = res.alloc<uint8_t>(s, std::max<size_t>(t->host.size(), 1));
    StackDeviceMemory::copyToDevice(mem.data(), t->host.data(), t->host.size(), s);
    base = reinterpret_cast<uintptr_t>(mem.data()) - kInlineBias;
  }
  BatchDesc map(BatchDesc d) const {
    if (!d.inl) return d;
    if (single) {
      auto entry = [&](auto p) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(p)>>;
        T v;
        std::memcpy(&v, reinterpret_cast<const uint8_t*>(single->w) + reinterpret_cast<uintptr_t>(p), sizeof(T));
        return v;
      };
      uint8_t* start = d.mode == BatchDesc::kPointer ? reinterpret_cast<uint8_t*>(entry(d.ptrs))
                       : d.mode == BatchDesc::kSplit ? d.base + entry(d.offsets)
                                                     : d.base;
      DG_CHECK(!d.sizes || (d.inl & BatchDesc::kInlSizes), "mixed inline / device size table");
      const uint32_t size = d.sizes ? entry(d.sizes) : d.fixedSize;
      return BatchDesc::strided(start, 0, size);
    }
    auto rebase = [&](auto p) { return reinterpret_cast<decltype(p)>(base + reinterpret_cast<uintptr_t>(p)); };
    if (d.inl & BatchDesc::kInlPtrs) d.ptrs = rebase(d.ptrs);
    if (d.inl & BatchDesc::kInlSizes) d.sizes = rebase(d.sizes);
    if (d.inl & BatchDesc::kInlOffsets) d.offsets = rebase(d.offsets);
    d.inl = 0;
    return d;
  }
};

}  // namespace dietgpu
