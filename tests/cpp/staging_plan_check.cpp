// Host-only check of the staging ring's placement policy (csrc/staging_plan.h)
// against a brute-force model of in-order streams: no HIP, no GPU.
//   g++ -std=c++17 -Wall -Werror -I dietgpu_fork_amd/csrc tests/cpp/staging_plan_check.cpp -o staging_plan_check
// and, being host code with its own main, the same with -O1 -g
// -fsanitize=address,undefined.  tests/test_staging_plan.py runs the cases
// one by one:  staging_plan_check <case> ...  (no argument: all of them).
//
// The model knows every use ever committed: its region, its stream and
// whether its copy has run.  A stream completes its uses in order; which
// stream moves when is the test's choice.  The policy sees the model only
// through complete / wait / release.  After every placement:
//   * the region is 256 B-aligned and lies inside the ring;
//   * it overlaps no use whose copy has not run (the overwrite the ring
//     exists to prevent);
//   * wait was called only for uses that were pending, release only for uses
//     that were complete, once each;
//   * the uses the policy still tracks are pairwise disjoint and include
//     every pending one.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <string>
#include <vector>

#include "staging_plan.h"

using namespace dietgpu;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static constexpr size_t MIB = size_t(1) << 20;

// The rule the ring had before StagingPlan, kept here as the control: only
// the front of the queue is looked at, on the assumption that the oldest use
// is the first one a new region can run into.  A wrap that skips a tail
// holding the oldest use breaks it (skippedTail below).
template <typename Token>
class FrontOnlyPlan {
 public:
  struct Use {
    size_t off, bytes;
    Token tok;
  };
  template <typename Complete, typename Wait, typename Release>
  size_t place(size_t bytes, Complete&& complete, Wait&& wait, Release&& release) {
    const size_t n = stagingRound(bytes);
    if (head_ + n > kStagingRingBytes) head_ = 0;
    const size_t off = head_;
    while (!uses_.empty()) {
      const Use u = uses_.front();
      const bool overlap = u.off < off + n && off < u.off + u.bytes;
      if (overlap) {
        if (!complete(u.tok)) wait(u.tok);
      } else if (!complete(u.tok)) {
        break;
      }
      release(u.tok);
      uses_.pop_front();
    }
    head_ = off + n;
    return off;
  }
  void commit(size_t off, size_t bytes, Token tok) { uses_.push_back(Use{off, stagingRound(bytes), tok}); }
  template <typename Complete, typename Wait, typename Release>
  void drain(Complete&& complete, Wait&& wait, Release&& release) {
    for (const Use& u : uses_) {
      if (!complete(u.tok)) wait(u.tok);
      release(u.tok);
    }
    uses_.clear();
    head_ = 0;
  }
  size_t ringBytes() const { return kStagingRingBytes; }
  const std::deque<Use>& inflight() const { return uses_; }

 private:
  size_t head_ = 0;
  std::deque<Use> uses_;
};

struct Model {
  struct Use {
    size_t off, bytes;
    int stream;
    bool done, released;
  };
  std::vector<Use> uses;                 // token = index
  size_t lo = 0;                         // every use below it is done (the checks start here)
  std::vector<std::deque<int>> pending;  // per stream, in order
  bool instant = false;                  // every copy has run by the time upload() returns
  uint64_t placements = 0, waits = 0, queries = 0;
  std::vector<std::string> bad;

  explicit Model(int streams) : pending(streams) {}

  void fail(const std::string& s) {
    if (bad.size() < 8) bad.push_back(s);
  }
  // the stream runs its next `count` copies
  void progress(int stream, size_t count) {
    auto& q = pending[stream];
    while (count-- && !q.empty()) {
      uses[q.front()].done = true;
      q.pop_front();
    }
  }
  void sync(int stream) { progress(stream, pending[stream].size()); }
  size_t pendingBytes() {
    size_t n = 0;
    for (size_t i = firstPending(); i < uses.size(); ++i) n += uses[i].done ? 0 : uses[i].bytes;
    return n;
  }
  size_t firstPending() {
    while (lo < uses.size() && uses[lo].done) ++lo;
    return lo;
  }

  template <typename Plan>
  size_t upload(Plan& plan, size_t bytes, int stream) {
    const uint64_t waitsBefore = waits;
    bool everyDone = true;
    for (size_t i = firstPending(); i < uses.size(); ++i) everyDone = everyDone && uses[i].done;
    const size_t off = plan.place(bytes, [&](int t) { return complete(t); }, [&](int t) { wait(t); },
                                  [&](int t) { release(t); });
    const size_t n = stagingRound(bytes);
    ++placements;
    char msg[200];
    if (off % kStagingAlign || off + n > plan.ringBytes() || n < bytes) {
      std::snprintf(msg, sizeof msg, "placement %llu: [%zu, %zu) is not an aligned region of the ring",
                    (unsigned long long)placements, off, off + n);
      fail(msg);
    }
    if (everyDone && waits != waitsBefore) fail("waited although every earlier use was complete");
    for (size_t i = firstPending(); i < uses.size(); ++i) {
      const Use& u = uses[i];
      if (!u.done && u.off < off + n && off < u.off + u.bytes) {
        std::snprintf(msg, sizeof msg, "placement %llu: [%zu, %zu) overwrites pending use %zu [%zu, %zu) of stream %d",
                      (unsigned long long)placements, off, off + n, i, u.off, u.off + u.bytes, u.stream);
        fail(msg);
      }
    }
    const int tok = int(uses.size());
    uses.push_back(Use{off, n, stream, instant, false});
    if (!instant) pending[stream].push_back(tok);
    plan.commit(off, bytes, tok);
    return off;
  }

  // what the policy tracks: disjoint, and every pending use among it
  template <typename Plan>
  void checkTracked(const Plan& plan) {
    std::vector<std::pair<size_t, size_t>> r;
    std::vector<bool> tracked(uses.size(), false);
    for (const auto& u : plan.inflight()) {
      r.push_back({u.off, u.off + u.bytes});
      tracked[u.tok] = true;
      if (uses[u.tok].released) fail("a released use is still tracked");
    }
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
      if (r[i].first < r[i - 1].second) fail("tracked uses overlap");
    for (size_t i = firstPending(); i < uses.size(); ++i)
      if (!uses[i].done && !tracked[i]) fail("a pending use is no longer tracked");
  }

  template <typename Plan>
  void drain(Plan& plan) {
    plan.drain([&](int t) { return complete(t); }, [&](int t) { wait(t); }, [&](int t) { release(t); });
    for (const Use& u : uses)
      if (!u.done || !u.released) fail("a use survived a drain");
    if (plan.head() != 0 || !plan.inflight().empty()) fail("a drain left the ring in use");
  }

 private:
  bool complete(int t) {
    ++queries;
    return uses[t].done;
  }
  void wait(int t) {
    if (uses[t].done) fail("wait for a use that was complete");
    ++waits;
    auto& q = pending[uses[t].stream];
    while (!uses[t].done) {  // in order: everything before it on its stream runs first
      uses[q.front()].done = true;
      q.pop_front();
    }
  }
  void release(int t) {
    if (!uses[t].done) fail("release of a pending use");
    if (uses[t].released) fail("use released twice");
    uses[t].released = true;
  }
};

// Section "skipped tail": seven 1 MiB uploads and a sync leave the head at
// 7 MiB; the stream stalls; H (917,504 B) lands in the tail at 7 MiB; N1..N7
// (1 MiB each) wrap to 0 and end at 7 MiB; N8 (1,310,720 B) wraps again, onto
// N1 and the first 256 KiB of N2, both pending behind H.
template <typename Plan>
static Model skippedTail(Plan& plan, size_t* at) {
  Model m(1);
  for (int i = 0; i < 7; ++i) REQUIRE(m.upload(plan, MIB, 0) == size_t(i) * MIB);
  m.sync(0);
  REQUIRE(m.upload(plan, 917504, 0) == 7 * MIB);                                   // H
  for (int i = 0; i < 7; ++i) REQUIRE(m.upload(plan, MIB, 0) == size_t(i) * MIB);  // N1..N7
  REQUIRE(m.bad.empty() && m.waits == 0);  // nothing so far had to wait: the old uploads were done
  *at = m.upload(plan, 1310720, 0);        // N8
  return m;
}

static void caseSkippedTail() {
  size_t at = 0;
  {
    StagingPlan<int> plan;
    Model m = skippedTail(plan, &at);
    for (const auto& s : m.bad) std::fprintf(stderr, "%s\n", s.c_str());
    REQUIRE(m.bad.empty());
    // the ring was full of pending uses: N8 waited, where it would have gone first
    REQUIRE(at == 0 && m.waits >= 1);
    // H, N1 and N2 ran (stream order); N3..N7 are still pending and tracked
    for (int t = 7; t <= 9; ++t) REQUIRE(m.uses[t].done);
    for (int t = 10; t <= 14; ++t) REQUIRE(!m.uses[t].done);
    m.checkTracked(plan);
    REQUIRE(m.bad.empty());
  }
  {
    // the control: the front-only rule hands N8 the bytes of N1 and N2
    FrontOnlyPlan<int> plan;
    Model m = skippedTail(plan, &at);
    REQUIRE(at == 0 && m.waits == 0);
    REQUIRE(m.bad.size() == 2);
    REQUIRE(m.bad[0].find("overwrites pending use 8 [0, 1048576)") != std::string::npos);
    REQUIRE(m.bad[1].find("overwrites pending use 9 [1048576, 2097152)") != std::string::npos);
    std::printf("front-only control: %s\nfront-only control: %s\n", m.bad[0].c_str(), m.bad[1].c_str());
  }
  std::puts("skipped-tail ok");
}

static size_t randomSize(std::mt19937_64& rng) {
  const uint64_t r = rng() % 100;
  if (r < 4) return kStagingMaxUpload;  // exactly 2 MiB
  if (r < 8) return 65540;              // the first size past the kernel arguments
  if (r < 12) return kStagingMaxUpload - (rng() % 300);
  if (r < 50) return 65540 + rng() % (256 * 1024);  // tables of a few thousand members
  return 65540 + rng() % (kStagingMaxUpload - 65540 + 1);
}

// Random uploads on `streams` streams that run, stall and catch up
// independently; drains at random points.
static void caseRandom(int streams, uint64_t seed, uint64_t placements) {
  std::mt19937_64 rng(seed);
  StagingPlan<int> plan;
  Model m(streams);
  std::vector<bool> stalled(streams, false);
  uint64_t total = 0, drains = 0, exact = 0, most = 0, aheadPeak = 0;
  while (total < placements) {
    const uint64_t r = rng() % 1000;
    const int s = int(rng() % streams);
    if (r < 500) {
      const size_t bytes = randomSize(rng);
      exact += bytes == kStagingMaxUpload;
      const uint64_t before = m.placements;
      m.upload(plan, bytes, s);
      total += m.placements - before;
      m.checkTracked(plan);
      most = std::max<uint64_t>(most, plan.inflight().size());
      aheadPeak = std::max<uint64_t>(aheadPeak, m.pendingBytes());
      // whatever is tracked is disjoint, so the ring bounds how many there are
      REQUIRE(plan.inflight().size() <= kStagingRingBytes / stagingRound(65540));
    } else if (r < 850) {
      if (!stalled[s]) m.progress(s, 1 + rng() % 6);
    } else if (r < 900) {
      if (!stalled[s]) m.sync(s);
    } else if (r < 960) {
      stalled[s] = !stalled[s];
    } else if (r < 975) {
      m.drain(plan);
      std::fill(stalled.begin(), stalled.end(), false);
      ++drains;
    }
    if (!m.bad.empty()) break;
  }
  const uint64_t waits = m.waits;
  for (const auto& s : m.bad) std::fprintf(stderr, "%s\n", s.c_str());
  REQUIRE(m.bad.empty());
  // the run must have been worth it: the host ran the ring full, and waited
  REQUIRE(exact >= 100 && drains >= 10 && waits >= 100 && aheadPeak > 6 * MIB);
  std::printf("random ok: streams %d placements %llu waits %llu drains %llu of-2MiB %llu most-tracked %llu "
              "most-pending-bytes %llu\n",
              streams, (unsigned long long)total, (unsigned long long)waits, (unsigned long long)drains,
              (unsigned long long)exact, (unsigned long long)most, (unsigned long long)aheadPeak);
}

// Every copy has run by the time its upload returns: no placement waits.
static void caseInstant(uint64_t seed, uint64_t placements) {
  std::mt19937_64 rng(seed);
  StagingPlan<int> plan;
  Model m(3);
  m.instant = true;
  for (uint64_t i = 0; i < placements; ++i) {
    m.upload(plan, randomSize(rng), int(rng() % 3));
    if (i % 64 == 0) m.checkTracked(plan);
  }
  for (const auto& s : m.bad) std::fprintf(stderr, "%s\n", s.c_str());
  REQUIRE(m.bad.empty() && m.waits == 0 && m.placements == placements);
  std::printf("instant ok: placements %llu waits 0\n", (unsigned long long)placements);
}

// Stream 0 is stalled with one pending upload in the tail; stream 1 is not
// stalled (its copies run at once) and makes 40 uploads that go round the
// ring several times: they step over the stalled region and never wait.
static void caseTwoStreams() {
  StagingPlan<int> plan;
  Model m(2);
  for (int i = 0; i < 7; ++i) m.upload(plan, MIB, 1);
  m.sync(1);
  REQUIRE(m.upload(plan, 917504, 0) == 7 * MIB);  // stalled: never progresses below
  std::mt19937_64 rng(5);
  size_t bytes = 0, wraps = 0, last = 7 * MIB;
  for (int i = 0; i < 40; ++i) {
    const size_t n = i % 5 == 0 ? kStagingMaxUpload : randomSize(rng);
    const size_t off = m.upload(plan, n, 1);
    m.sync(1);
    wraps += off < last;
    last = off;
    bytes += n;
    REQUIRE(!(off < 7 * MIB + 917504 && 7 * MIB < off + stagingRound(n)));
  }
  for (const auto& s : m.bad) std::fprintf(stderr, "%s\n", s.c_str());
  REQUIRE(m.bad.empty() && m.waits == 0 && !m.uses[7].done);
  REQUIRE(wraps >= 3);
  m.checkTracked(plan);
  REQUIRE(m.bad.empty());
  std::printf("two-streams ok: uploads 40 bytes %zu wraps %zu waits 0\n", bytes, wraps);
}

static void caseRounding() {
  static_assert(stagingRound(1) == 256 && stagingRound(256) == 256 && stagingRound(257) == 512, "");
  static_assert(stagingRound(65540) == 65792 && stagingRound(kStagingMaxUpload) == 2 * MIB, "");
  static_assert(kStagingRingBytes == 8 * MIB && kStagingMaxUpload == 2 * MIB, "");
  StagingPlan<int> plan;
  Model m(1);
  // four uploads of 2 MiB fill the ring exactly; the fifth wraps and waits for the first alone
  for (int i = 0; i < 4; ++i) REQUIRE(m.upload(plan, 2 * MIB, 0) == size_t(i) * 2 * MIB);
  REQUIRE(plan.head() == 8 * MIB && m.waits == 0);
  REQUIRE(m.upload(plan, 2 * MIB, 0) == 0 && m.waits == 1);
  REQUIRE(m.uses[0].done && !m.uses[1].done);
  // one byte more than fits before the end skips the tail
  StagingPlan<int> p2;
  Model m2(1);
  m2.instant = true;
  REQUIRE(m2.upload(p2, 8 * MIB - 65792, 0) == 0);
  REQUIRE(m2.upload(p2, 65792, 0) == 8 * MIB - 65792);
  REQUIRE(m2.upload(p2, 8 * MIB - 65792, 0) == 0);
  REQUIRE(m2.upload(p2, 65793, 0) == 0);
  REQUIRE(m.bad.empty() && m2.bad.empty());
  bool threw = false;
  try {
    p2.place(8 * MIB + 1, [](int) { return true; }, [](int) {}, [](int) {});
  } catch (const std::length_error&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    p2.place(0, [](int) { return true; }, [](int) {}, [](int) {});
  } catch (const std::length_error&) {
    threw = true;
  }
  REQUIRE(threw);
  std::puts("rounding ok");
}

int main(int argc, char** argv) {
  std::vector<std::string> cases(argv + 1, argv + argc);
  if (cases.empty()) cases = {"rounding", "skipped-tail", "two-streams", "instant", "random2", "random3"};
  for (const auto& c : cases) {
    if (c == "rounding") caseRounding();
    else if (c == "skipped-tail") caseSkippedTail();
    else if (c == "two-streams") caseTwoStreams();
    else if (c == "instant") caseInstant(7, 10000);
    else if (c == "random2") caseRandom(2, 20241, 12000);
    else if (c == "random3") caseRandom(3, 20242, 12000);
    else {
      std::fprintf(stderr, "unknown case %s\n", c.c_str());
      return 2;
    }
  }
  return 0;
}
