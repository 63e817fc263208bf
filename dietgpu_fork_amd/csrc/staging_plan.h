// Placement policy of the pinned host->device staging ring (stack_memory.cpp,
// StackDeviceMemory::copyToDevice): where an upload's bytes go in the ring and
// which earlier uploads must have left it first.  Host-only, no HIP headers:
// an in-flight use carries an opaque Token (the driver's hipEvent_t) and the
// policy learns about the device through three callbacks,
//   complete(tok) -> bool   has the copy out of this use finished?
//   wait(tok)               block until it has
//   release(tok)            the policy has forgotten the use; recycle tok
// so tests/cpp/staging_plan_check.cpp drives it against a model of streams.
//
// The rule.  A region is handed out only when every in-flight use that
// overlaps it has been seen complete or waited for, wherever that use sits in
// the order of placement and whichever stream it belongs to.  The uses in
// flight are therefore pairwise disjoint (at most ring / smallest upload of
// them), and one pass over all of them per candidate region is cheap.
//   1. The candidate starts at the head, or at 0 when the upload does not fit
//      before the end (the tail is skipped, and whatever is in flight there
//      stays in flight and stays tracked).
//   2. Overlapping uses that are complete are retired.  If none is left the
//      candidate is taken: an upload behind finished work waits for nothing.
//   3. Otherwise the candidate moves to the end of the furthest pending use
//      it ran into (wrapping again if need be) and step 2 repeats: a stream
//      that is stalled with an upload in the ring does not hold up uploads of
//      other streams as long as the ring has room elsewhere.
//   4. Once the candidates have travelled a whole turn of the ring without
//      finding room, the first candidate is taken after waiting for exactly
//      its pending overlapping uses.
#pragma once

#include <cstddef>
#include <stdexcept>
#include <vector>

namespace dietgpu {

constexpr size_t kStagingRingBytes = size_t(8) << 20;
constexpr size_t kStagingAlign = 256;
// uploads above a quarter of the ring do not go through it
constexpr size_t kStagingMaxUpload = kStagingRingBytes / 4;

constexpr size_t stagingRound(size_t bytes) { return (bytes + kStagingAlign - 1) / kStagingAlign * kStagingAlign; }

template <typename Token>
class StagingPlan {
 public:
  struct Use {
    size_t off, bytes;  // bytes rounded to kStagingAlign
    Token tok;
  };

  explicit StagingPlan(size_t ringBytes = kStagingRingBytes) : ring_(ringBytes) {}

  // The offset of a region of stagingRound(bytes) that nothing in flight
  // overlaps any more.  The caller fills it, enqueues the copy out of it and
  // then commit()s the use with a token that completes after that copy.
  template <typename Complete, typename Wait, typename Release>
  size_t place(size_t bytes, Complete&& complete, Wait&& wait, Release&& release) {
    const size_t n = stagingRound(bytes);
    if (bytes == 0 || n > ring_) throw std::length_error("staging ring: upload of 0 bytes or larger than the ring");
    const size_t first = head_ + n > ring_ ? 0 : head_;
    size_t off = first, travelled = 0;
    for (;;) {
      size_t pendingEnd = 0;  // end of the furthest pending use under [off, off + n)
      for (size_t i = uses_.size(); i-- > 0;) {
        const Use u = uses_[i];
        if (!(u.off < off + n && off < u.off + u.bytes)) continue;
        if (complete(u.tok)) {
          release(u.tok);
          drop(i);
        } else if (u.off + u.bytes > pendingEnd) {
          pendingEnd = u.off + u.bytes;
        }
      }
      if (pendingEnd == 0) break;
      const size_t next = pendingEnd + n > ring_ ? 0 : pendingEnd;
      travelled += next > off ? next - off : ring_ - off + next;
      if (travelled >= ring_) {
        // no room anywhere: wait where the upload would have gone first
        off = first;
        for (size_t i = uses_.size(); i-- > 0;) {
          const Use u = uses_[i];
          if (!(u.off < off + n && off < u.off + u.bytes)) continue;
          if (!complete(u.tok)) wait(u.tok);
          release(u.tok);
          drop(i);
        }
        break;
      }
      off = next;
    }
    head_ = off + n;
    return off;
  }

  void commit(size_t off, size_t bytes, Token tok) { uses_.push_back(Use{off, stagingRound(bytes), tok}); }

  // Waits for every use still pending, forgets them all and puts the head at 0.
  template <typename Complete, typename Wait, typename Release>
  void drain(Complete&& complete, Wait&& wait, Release&& release) {
    for (const Use& u : uses_) {
      if (!complete(u.tok)) wait(u.tok);
      release(u.tok);
    }
    uses_.clear();
    head_ = 0;
  }

  size_t ringBytes() const { return ring_; }
  size_t head() const { return head_; }
  const std::vector<Use>& inflight() const { return uses_; }

 private:
  void drop(size_t i) {
    uses_[i] = uses_.back();
    uses_.pop_back();
  }

  size_t ring_;
  size_t head_ = 0;
  std::vector<Use> uses_;
};

}  // namespace dietgpu
