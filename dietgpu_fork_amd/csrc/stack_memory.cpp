// LIFO device arena + pinned H2D staging ring.
// Semantics follow dietgpu/utils/StackDeviceMemory.cpp:34-250 (LIFO frees,
// overflow to hipMalloc with a warning, high-water mark).
#include "dietgpu/StackDeviceMemory.h"

#include <algorithm>
#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>

#include "common.h"
#include "staging_plan.h"

namespace dietgpu {

StackDeviceMemory::StackDeviceMemory(int device, size_t bytes) : device_(device) {
  if (bytes) {
    bytes = std::max(bytes, kSDMAlignment);
    int prev = 0;
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&owned_), bytes));
    HIP_CHECK(hipSetDevice(prev));
    start_ = owned_;
    head_ = start_;
    end_ = owned_ + bytes;
  }
}

StackDeviceMemory::StackDeviceMemory(int device, void* p, size_t bytes)
    : device_(device) {
  DG_CHECK(p || bytes == 0, "null temp memory with nonzero size");
  if (p && bytes >= kSDMAlignment) {
    // the managed region must start 256-byte aligned; trim the front if not
    uintptr_t a = reinterpret_cast<uintptr_t>(p);
    uintptr_t aligned = (a + kSDMAlignment - 1) / kSDMAlignment * kSDMAlignment;
    size_t lost = aligned - a;
    if (bytes > lost) {
      start_ = reinterpret_cast<char*>(aligned);
      head_ = start_;
      end_ = start_ + (bytes - lost) / kSDMAlignment * kSDMAlignment;
    }
  }
}

StackDeviceMemory::~StackDeviceMemory() {
  for (auto& kv : overflow_) {
    (void)hipFree(kv.first);
  }
  if (owned_) {
    (void)hipFree(owned_);
  }
}

void* StackDeviceMemory::allocPointer(hipStream_t stream, size_t bytes, AllocType type) {
  DG_CHECK(bytes >= kSDMAlignment && bytes % kSDMAlignment == 0, "bad size " << bytes);
  void* out = nullptr;
  size_t used = size_t(head_ - start_);
  if (type == AllocType::Permanent || bytes > getSizeAvailable()) {
    // the reference warns on every overflow; we warn once per arena
    if (type == AllocType::Temporary && !warned_) {
      warned_ = true;
      std::cerr << "WARNING: StackDeviceMemory: attempting to allocate " << bytes
                << " bytes with " << getSizeAvailable()
                << " bytes available; calling hipMalloc. Resize temp memory to >= "
                << std::max(maxSeen_, used + overflowBytes_ + bytes)
                << " bytes to avoid performance problems.\n";
    }
    int prev = 0;
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(device_));
    hipError_t e = hipMalloc(&out, bytes);
    HIP_CHECK(hipSetDevice(prev));
    HIP_CHECK(e);
    overflow_[out] = bytes;
    overflowBytes_ += bytes;
  } else {
    out = head_;
    head_ += bytes;
    used += bytes;
  }
  maxSeen_ = std::max(maxSeen_, used + overflowBytes_);
  return out;
}

void StackDeviceMemory::deallocPointer(int device, hipStream_t stream, size_t bytes, void* p) {
  DG_CHECK(p, "null free");
  DG_CHECK(device == device_, "device mismatch");
  auto it = overflow_.find(p);
  if (it != overflow_.end()) {
    DG_CHECK(it->second == bytes, "overflow size mismatch");
    // the block may still be in use by work queued on `stream`
    (void)hipStreamSynchronize(stream);
    (void)hipFree(p);
    overflowBytes_ -= bytes;
    overflow_.erase(it);
    return;
  }
  char* pc = static_cast<char*>(p);
  DG_CHECK(pc >= start_ && pc < end_, "pointer not owned by this arena");
  DG_CHECK(pc + bytes == head_, "allocations must be freed in LIFO order");
  head_ = pc;
}

std::string StackDeviceMemory::toString() const {
  std::ostringstream s;
  s << "SDM device " << device_ << ": total " << getSizeTotal() << " B, available "
    << getSizeAvailable() << " B, max seen " << maxSeen_ << " B, overflow "
    << overflowBytes_ << " B";
  return s.str();
}

// ---------------------------------------------------------------------------
// pinned staging ring for host->device parameter tables
// ---------------------------------------------------------------------------
namespace {
// The ring's memory, its events and its lock; where an upload goes and what it
// waits for is StagingPlan's (staging_plan.h).
struct StagingRing {
  std::mutex mu;
  char* host = nullptr;
  StagingPlan<hipEvent_t> plan;
  std::vector<hipEvent_t> freeEvents;

  hipEvent_t getEvent() {
    if (!freeEvents.empty()) {
      auto e = freeEvents.back();
      freeEvents.pop_back();
      return e;
    }
    hipEvent_t e;
    // completion of the copy is all the ring needs: no system-scope fence
    // (it would write back and invalidate L2 at every upload)
    HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    return e;
  }
  static bool complete(hipEvent_t e) { return hipEventQuery(e) == hipSuccess; }
  static void wait(hipEvent_t e) { HIP_CHECK(hipEventSynchronize(e)); }
};
StagingRing& ring() {
  static StagingRing r;
  return r;
}
} // namespace

bool uploadViaKernargs(void* dst, const void* src, size_t bytes, hipStream_t s);  // upload.hip

void StackDeviceMemory::copyToDevice(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return;
  if (uploadViaKernargs(dst, src, bytes, s)) return;  // tables up to 64 KB: no blit
  auto& r = ring();
  if (bytes > kStagingMaxUpload) {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return;
  }
  std::lock_guard<std::mutex> g(r.mu);
  if (!r.host) {
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&r.host), kStagingRingBytes, hipHostMallocDefault));
  }
  const size_t off = r.plan.place(bytes, StagingRing::complete, StagingRing::wait,
                                  [&](hipEvent_t e) { r.freeEvents.push_back(e); });
  std::memcpy(r.host + off, src, bytes);
  HIP_CHECK(hipMemcpyAsync(dst, r.host + off, bytes, hipMemcpyHostToDevice, s));
  hipEvent_t ev = r.getEvent();
  HIP_CHECK(hipEventRecord(ev, s));
  r.plan.commit(off, bytes, ev);
}

void stagingRingReset() {
  auto& r = ring();
  std::lock_guard<std::mutex> g(r.mu);
  r.plan.drain(StagingRing::complete, StagingRing::wait, [&](hipEvent_t e) { r.freeEvents.push_back(e); });
}

StackDeviceMemory makeStackMemory(size_t bytes) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  return StackDeviceMemory(dev, bytes);
}

} // namespace dietgpu
