// Host check of the compress rule (dietgpu_fork_amd/csrc/compress_plan.h),
// built by tests/test_compress_plan.py with a plain C++ compiler: literal
// anchors computed by hand from the drivers the rule replaced, then a sweep
// against those drivers' formulas, kept here as reference functions
// (encodeBatchDevice's condition, persistentPreferred / planPersistent,
// compressPersistent's derivations and compressThreeKernel's booleans).
//
// One difference is deliberate: the drivers' divUp was 32-bit and wrapped for
// sizes above 2^32 - 4096 (more than any archive holds: the size queries
// refuse them); the reference below forms it in 64 bits, as the plan does.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "compress_plan.h"

using namespace dietgpu;

static uint64_t divUp(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
static uint64_t roundUp(uint64_t a, uint64_t b) { return divUp(a, b) * b; }

// ---------------------------------------------------------------------------
// the replaced drivers
// ---------------------------------------------------------------------------
static uint32_t refHistChunkWords(uint32_t nb, uint32_t maxSize, int segs) {
  uint32_t chunk = 64 * 1024;
  auto enough = [&](uint32_t c) {
    const uint64_t total = uint64_t(nb) * divUp(std::max(maxSize, 1u), c);
    return total >= 2048 || (segs == 1 && c <= 16 * 1024 && total >= 512);
  };
  while (chunk > 4096 && !enough(chunk)) chunk /= 2;
  while (divUp(maxSize, chunk) > 4096) chunk *= 2;
  return chunk;
}

struct RefPersistent {
  uint32_t team = 0, teamsPerRound = 0, rounds = 0;
  bool xcd = false;
};

static RefPersistent refPlanPersistent(uint32_t nb, uint32_t maxWords, uint32_t slots) {
  RefPersistent p;
  const uint32_t team = std::max<uint32_t>(1, divUp(divUp(maxWords, 4096), 8));
  if (team > 32 || nb == 0) return p;
  const uint32_t maxTeams = std::max(1u, slots / team);
  p.team = team;
  p.rounds = uint32_t(divUp(nb, maxTeams));
  p.teamsPerRound = uint32_t(divUp(nb, p.rounds));
  p.xcd = roundUp(p.teamsPerRound, 8) <= maxTeams;
  if (p.xcd) p.teamsPerRound = uint32_t(roundUp(p.teamsPerRound, 8));
  return p;
}

static bool refPersistentPreferred(int mode, uint32_t nb, uint32_t maxWords, uint32_t slots) {
  if (mode == 2) return false;
  const RefPersistent p = refPlanPersistent(nb, maxWords, slots);
  if (p.team == 0) return false;
  if (mode == 1) return true;
  if (uint64_t(p.team) * nb <= 256) return false;
  return !(p.rounds == 1 && !p.xcd);
}

// compressPersistent; false: it declined and the call fell through
static bool refCompressPersistent(const CompressShape& sh, bool kCk, CompressPlan& out) {
  const bool floatCk = !sh.byteCodec && sh.useChecksum;
  const RefPersistent plan = refPlanPersistent(sh.nb, sh.maxSize, sh.pcompressSlots);
  const uint32_t team = plan.team;
  if (team == 0) return false;
  out.singlePass = true;
  const uint64_t items64 = uint64_t(team) * sh.nb;
  if (!(items64 < (1ull << 30))) {
    out.tooManyItems = true;  // DG_CHECK "batch too large for one compress call"
    return true;
  }
  const uint32_t items = uint32_t(items64);
  const uint32_t grid = plan.teamsPerRound * team;
  out.spillSlots = uint64_t(grid) * 8;
  out.floatCkWords = floatCk ? sh.nb : 1;
  const uint64_t partBytes = uint64_t(items) * 256 * 4;
  const uint32_t teams = grid / team;
  const uint32_t maxR = 2 * uint32_t(divUp(sh.nb, teams)) + 2;
  out.flagBytes = uint64_t(items) * 8;
  out.partialBytes = partBytes + (kCk ? uint64_t(items) * 4 : 0);
  out.logBytes = uint64_t(teams) * maxR * 8;
  out.rounds = plan.rounds;
  out.teamsPerRound = teams;
  out.xcd = plan.xcd;
  out.grid = grid;
  out.maxR = maxR;
  out.items = items;
  out.slotSpan = std::max(1u, sh.cus);
  return true;
}

static void refCompressThreeKernel(const CompressShape& sh, CompressPlan& out) {
  const uint64_t kSegs = uint64_t(sh.segs), nb = sh.nb;
  const bool kFused = sh.segs == 1;
  const bool useChecksum = sh.useChecksum;
  const uint32_t MB = uint32_t(divUp(sh.maxSize, 4096));
  const bool userHist = sh.byteCodec && sh.userHist;
  const bool preHist = !sh.byteCodec && sh.pre != PreHist::kNone;
  const bool preNorm = preHist && sh.pre == PreHist::kRowsAndTable;
  const uint32_t chunkWords = refHistChunkWords(sh.nb, sh.maxSize, sh.segs);
  const uint32_t chunks =
      preHist ? std::max(1u, sh.preRows) : std::max<uint32_t>(1, uint32_t(divUp(sh.maxSize, chunkWords)));
  const bool runHist = !preHist && (!userHist || useChecksum);
  const bool rawCk = sh.byteCodec && useChecksum;
  const uint32_t nW = std::max<uint32_t>(1, uint32_t(divUp(MB, 8)));
  const uint64_t proRowsBytes = kSegs * nb * std::min(chunks, 64u) * 256 * 4;
  const bool pro = runHist && !userHist && !rawCk && MB > 0 && proRowsBytes <= (32ull << 20) &&
                   nb * nW <= 2ull * sh.encodeProSlots;
  out.partHist = runHist && !pro ? kSegs * nb * chunks * 256 : 1;
  out.partCk = rawCk ? nb * chunks : 1;
  const uint32_t groups = uint32_t(divUp(chunks, 64));
  const bool reduce2 = (runHist || preHist) && !preNorm && !pro && chunks > 64;
  out.groupHist = reduce2 ? kSegs * nb * groups * 256 : 1;
  out.groupCk = reduce2 && rawCk ? nb * groups : 1;
  out.ck = nb;
  out.table = out.pdf = preNorm ? 1 : kSegs * nb * 256;
  out.slots = kSegs * nb * std::max(MB, 1u);
  out.cw = kFused ? 1 : kSegs * nb * std::max(MB, 1u);
  const bool finalInHist = !reduce2 && !pro && runHist && uint64_t(chunks) * nb <= 4096;
  out.lookbackBytes = kSegs * nb * nW * 8;
  out.arriveBytes = nb * kSegs * 4;
  out.rowsBytes = pro ? proRowsBytes : 0;
  out.coalesceFromFlags = kFused || MB > 8192;
  // the launch lambda's tests
  out.runHist = runHist;
  out.hist = pro ? HistKernel::kRows : rawCk ? HistKernel::kChecksum : HistKernel::kPlain;
  const bool normKernel = !reduce2 && !finalInHist && !preNorm && !pro;
  out.normalise = reduce2       ? Normalise::kInReduce
                  : normKernel  ? Normalise::kKernel
                  : pro         ? Normalise::kPrologue
                  : finalInHist ? Normalise::kInHist
                                : Normalise::kCaller;
  out.encodeRuns = MB > 0 || kFused;
  out.rowsPer = pro ? std::min(chunks, 64u) : 0;
  out.chunkWords = chunkWords;
  out.chunks = chunks;
  out.groups = groups;
  out.encodeWGs = nW;
}

// encodeBatchDevice
static CompressPlan refEncodeBatch(const CompressShape& sh) {
  CompressPlan out;
  out.maxBlocks = uint32_t(divUp(sh.maxSize, 4096));
  out.team = std::max<uint32_t>(1, uint32_t(divUp(out.maxBlocks, 8)));
  out.rawCk = sh.byteCodec && sh.useChecksum;
  if (sh.segs == 1) {
    const bool userHist = sh.byteCodec && sh.userHist;
    const bool rawCk = sh.byteCodec && sh.useChecksum;
    if (!userHist && sh.inAligned16 &&
        ((rawCk && sh.mode != 2) || refPersistentPreferred(sh.mode, sh.nb, sh.maxSize, sh.pcompressSlots))) {
      if (refCompressPersistent(sh, rawCk, out)) return out;
    }
  }
  refCompressThreeKernel(sh, out);
  // the reason, which the drivers never named: the first that applies
  out.refused = sh.segs == 2        ? Refused::kTwoSegments
                : sh.userHist      ? Refused::kUserHist
                : !sh.inAligned16  ? Refused::kUnaligned
                : sh.mode == 2     ? Refused::kForced
                : out.team > 32    ? Refused::kTooLarge
                                   : Refused::kSizeRule;
  return out;
}

// ---------------------------------------------------------------------------
static int failures = 0;

static bool same(const CompressPlan& a, const CompressPlan& b) {
#define F(x) if (a.x != b.x) { std::printf("  field " #x ": got %llu, expected %llu\n", (unsigned long long)a.x, (unsigned long long)b.x); return false; }
  F(singlePass) F(refused) F(maxBlocks) F(team) F(rawCk) F(tooManyItems) F(rounds) F(teamsPerRound) F(xcd)
  F(grid) F(maxR) F(items) F(slotSpan) F(spillSlots) F(floatCkWords) F(flagBytes) F(partialBytes) F(logBytes)
  F(chunkWords) F(chunks) F(groups) F(runHist) F(hist) F(normalise) F(encodeWGs) F(encodeRuns)
  F(coalesceFromFlags) F(rowsPer) F(partHist) F(partCk) F(groupHist) F(groupCk) F(ck) F(table) F(pdf) F(slots)
  F(cw) F(lookbackBytes) F(arriveBytes) F(rowsBytes)
#undef F
  return true;
}

static void expect(const char* what, bool ok) {
  if (ok) return;
  ++failures;
  std::printf("FAIL %s\n", what);
}

// a 16 B-aligned batch with 1024 single-pass slots
static CompressShape shape(bool bytes, uint32_t nb, uint32_t maxSize, bool ck = false, int mode = 0) {
  CompressShape sh;
  sh.byteCodec = bytes;
  sh.nb = nb;
  sh.maxSize = maxSize;
  sh.useChecksum = ck;
  sh.inAligned16 = true;
  sh.mode = mode;
  sh.pcompressSlots = 1024;
  sh.encodeProSlots = 2048;
  sh.cus = 256;
  return sh;
}

int main() {
  {  // bf16, DESIGN.md 5.1c
    CompressPlan p = planCompress(shape(false, 256, 524288));
    expect("c2", p.singlePass && p.team == 16 && p.rounds == 4 && p.teamsPerRound == 64 && p.xcd && p.grid == 1024 &&
                     p.maxR == 10 && p.items == 4096 && !p.tooManyItems);
    p = planCompress(shape(false, 16, 1000000));
    expect("16 x 1e6", p.singlePass && p.team == 31 && p.grid == 496 && p.xcd);
    p = planCompress(shape(false, 1, 1000000));
    expect("1 x 1e6", !p.singlePass && p.team == 31 && p.refused == Refused::kSizeRule);
    p = planCompress(shape(false, 8, 524288));
    expect("8 x 524288", !p.singlePass && p.team == 16 && p.refused == Refused::kSizeRule);
    // one round of 33 teams; the 40 of XCD-aligned teams do not fit the 33 available
    p = planCompress(shape(false, 33, 1000000));
    expect("33 x 1e6", !p.singlePass && p.team == 31 && p.refused == Refused::kSizeRule);
    p = planCompress(shape(true, 1, (1u << 20) + 1));
    expect("1 MiB + 1 bytes", !p.singlePass && p.team == 33 && p.refused == Refused::kTooLarge);
    p = planCompress(shape(true, 1, 5000, true));
    expect("5000 bytes with checksum", p.singlePass && p.team == 1 && p.rawCk);
    p = planCompress(shape(true, 1, 5000, true, 2));
    expect("5000 bytes with checksum, mode 2", !p.singlePass && p.refused == Refused::kForced);
    p = planCompress(shape(false, 1, 1000000, false, 1));
    expect("1 x 1e6, mode 1", p.singlePass && p.team == 31);
    // 64-bit sizes: 2^20 blocks, 2^17 encode workgroups, 4096 chunks of 2^20 words
    p = planCompress(shape(false, 1, 0xffffffffu));
    expect("2^32 - 1 words", !p.singlePass && p.maxBlocks == (1u << 20) && p.encodeWGs == (1u << 17) &&
                                 p.chunkWords == (1u << 20) && p.chunks == 4096 &&
                                 p.normalise == Normalise::kInReduce);
  }

  // Normalisation routes the GPU tests (tests/test_gpu_compress_plan.py) state
  // as literals: they must hold whatever the two occupancies are.
  const uint32_t slotCounts[] = {1, 1024, 1536, 2048};
  for (uint32_t ps : slotCounts)
    for (uint32_t es : slotCounts) {
      auto with = [&](CompressShape sh) {
        sh.pcompressSlots = ps;
        sh.encodeProSlots = es;
        return planCompress(sh);
      };
      CompressPlan p = with(shape(true, 1, 100000, true, 2));
      expect("100000 bytes with checksum: kInHist", !p.singlePass && p.chunks == 25 && p.normalise == Normalise::kInHist);
      p = with(shape(true, 1, 1u << 20, true, 2));
      expect("1 MiB with checksum: kInReduce", !p.singlePass && p.chunks == 256 && p.normalise == Normalise::kInReduce);
      CompressShape uh = shape(true, 4, 65536);
      uh.userHist = true;
      p = with(uh);
      expect("caller's histogram: kKernel", !p.singlePass && !p.runHist && p.normalise == Normalise::kKernel);
      CompressShape sp = shape(false, 1, 200000);
      expect("sparse list: three kernels", !with(sp).singlePass);
      sp.pre = PreHist::kRowsAndTable;
      sp.preRows = 49;
      p = with(sp);
      expect("sparse list: kCaller", !p.singlePass && !p.runHist && p.normalise == Normalise::kCaller);
      expect("5000 bytes with checksum: single-pass", with(shape(true, 1, 5000, true)).singlePass);
      expect("16 x 1e6: single-pass", with(shape(false, 16, 1000000)).singlePass);
    }

  const uint32_t nbs[] = {1, 7, 8, 9, 16, 33, 256, 257, 1024, 65535, 65536, 1u << 25};
  const uint32_t sizes[] = {0, 1, 4096, 4097, 32768, 32769, 1u << 20, (1u << 20) + 1, 1000000, 1u << 24,
                            100000000, 0xffffffffu};
  // PartialHist: none, then rows and rows with a table of 1, 64 and 65 rows
  struct Pre {
    PreHist state;
    uint32_t rows;
  };
  const Pre pres[] = {{PreHist::kNone, 0},  {PreHist::kRows, 1},          {PreHist::kRows, 64},
                      {PreHist::kRows, 65}, {PreHist::kRowsAndTable, 1},  {PreHist::kRowsAndTable, 64},
                      {PreHist::kRowsAndTable, 65}};
  unsigned cases = 0, skipped = 0, refusedItems = 0;
  for (int segs = 1; segs <= 2; ++segs)
    for (int bytes = 0; bytes < 2; ++bytes)
      for (uint32_t nb : nbs)
        for (uint32_t size : sizes)
          for (uint32_t ps : slotCounts)
            for (uint32_t es : slotCounts)
              for (int ck = 0; ck < 2; ++ck)
                for (int uh = 0; uh < 2; ++uh)
                  for (const Pre& pre : pres)
                    for (int al = 0; al < 2; ++al)
                      for (int mode = 0; mode < 3; ++mode) {
                        // what no caller can form: a two-segment byte codec, a
                        // histogram for floats, counted rows for bytes
                        if ((bytes && segs == 2) || (uh && !bytes) || (pre.state != PreHist::kNone && bytes)) {
                          ++skipped;
                          continue;
                        }
                        CompressShape sh;
                        sh.segs = segs;
                        sh.byteCodec = bytes != 0;
                        sh.nb = nb;
                        sh.maxSize = size;
                        sh.useChecksum = ck != 0;
                        sh.userHist = uh != 0;
                        sh.pre = pre.state;
                        sh.preRows = pre.rows;
                        sh.inAligned16 = al != 0;
                        sh.mode = mode;
                        sh.pcompressSlots = ps;
                        sh.encodeProSlots = es;
                        sh.cus = 256;
                        const CompressPlan got = planCompress(sh), want = refEncodeBatch(sh);
                        ++cases;
                        refusedItems += got.tooManyItems;
                        if (!same(got, want)) {
                          ++failures;
                          std::printf("FAIL segs %d bytes %d nb %u size %u slots %u/%u ck %d hist %d pre %d/%u "
                                      "aligned %d mode %d\n",
                                      segs, bytes, nb, size, ps, es, ck, uh, int(pre.state), pre.rows, al, mode);
                          if (failures > 20) return 1;
                        }
                      }
  expect("the sweep reaches nb x team = 2^30", refusedItems > 0);
  std::printf("%u sweep cases, %u skipped, %u refused for their item count, %d failures\n", cases, skipped,
              refusedItems, failures);
  return failures ? 1 : 0;
}
