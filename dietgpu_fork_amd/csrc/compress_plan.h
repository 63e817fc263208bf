// The compress rule: which compressor takes a batch -- the single-pass
// k_pcompress (pcompress.h) or k_hist -> k_encode (encode.h) -- with what
// grids, which kernel normalises the histograms, and how much scratch and
// arena memory the call takes.  Host only and free of HIP headers, so that the
// rule -- performance policy, DESIGN.md 5.1c -- is stated once and tested
// without a GPU (tests/test_compress_plan.py).  The drivers (codec.hip
// compressPersistent, compressThreeKernel) allocate what the plan sizes and
// launch what it names; the sparse compressor (sparse.hip) asks the same plan
// whether the dense stage will count its own histogram.
//
// All products are formed in 64 bits.
#pragma once

#include <algorithm>
#include <cstdint>

namespace dietgpu {

// ---------------------------------------------------------------------------
// constants of the rule (the kernels use or static_assert them)
// ---------------------------------------------------------------------------
namespace cplan {
constexpr uint32_t kBlockWords = 4096;  // symbols per ANS block (kBlockSize)
constexpr uint32_t kSymbols = 256;      // bins of a histogram row (kNumSymbols)
constexpr uint32_t kXcds = 8;           // workgroups w, w + 8, ... share an XCD
}  // namespace cplan

namespace pc {
// A k_pcompress item: 8 consecutive blocks of one element, one block pair per
// wave of its workgroup.
constexpr uint32_t kBlocksPerItem = 8;
// Largest team summed by every member (a 1 MiB-symbol element): its partials
// are one sc1 load per member and bin.
constexpr uint32_t kMaxTeam = 32;
}  // namespace pc

// Blocks of a k_encode workgroup: one block pair per wave (EncCfg::kBlocksPerWG).
constexpr uint32_t kEncBlocksPerWG = 8;

// kRows (small three-kernel grids, k_encode's prologue normalisation):
// chunk c adds its counts with atomics into row c % P of [segs][nb][P][256],
// P = proRowsOf(chunks) = min(chunks, kProRows) (this call's zeroed buffer of
// the sync arena), so the encoder sums P rows instead of a k_histReduce /
// k_normalize launch summing thousands; zero bins add nothing.  Sized by the
// chunk count, so a batch of many one-chunk elements holds one row per
// element and segment, not 64.
constexpr uint32_t kProRows = 64;
constexpr uint32_t proRowsOf(uint32_t chunks) { return chunks < kProRows ? chunks : kProRows; }
// The rows are double-buffered in the stream's arena, which never shrinks:
// the prologue route only while they stay within this many bytes.
constexpr uint64_t kProRowsBudget = 32ull << 20;

// Chunks that one k_histReduce workgroup sums (first level of the partial-
// histogram sum when an element has many chunks: one 128 MiB fp64 tensor is
// 2048 chunks, which k_normalize's single workgroup would sum serially for
// ~0.3 ms).
constexpr uint32_t kReduceRows = 64;

// The normalisation runs in the last workgroup of the kernel that writes an
// element's final partial rows (k_histReduce, or a k_hist of at most this
// many workgroups), saving the k_normalize launch.  Each of those workgroups
// pays a wait for its rows' write-through stores and a counter round trip:
// with many (c3's k_hist: 65,536) that costs more than the launch (c3 hist
// 0.74 -> 1.09 ms), so k_normalize runs there.
constexpr uint64_t kMaxLastArrivalWGs = 4096;

// fp64 (two segments): k_encode's per-segment look-back leaves each
// workgroup's prefix in its flag for k_coalesce, whose per-workgroup sums
// over every earlier block are otherwise quadratic in the blocks (1e8 words:
// coalesce 129 us).  Up to this many blocks per element the sums are cheaper
// than the look-back's hand-offs (16.7M words: compress +1.5 us with it).
constexpr uint32_t kCoalFlagBlocks = 8192;

// At most this many k_pcompress items leave most of the chip idle while a
// team's members wait on each other's partial histograms: three kernels.
constexpr uint64_t kMinPersistentItems = 256;

// ---------------------------------------------------------------------------
// the shape of a compress call and its plan
// ---------------------------------------------------------------------------
// What the caller counted already (PartialHist, codec_internal.h).
enum class PreHist : uint8_t { kNone, kRows, kRowsAndTable };

struct CompressShape {
  int segs = 1;            // ANS segments of the format: 2 for fp64
  bool byteCodec = false;  // the byte codec (FT 0), not a float format
  uint32_t nb = 0;         // elements (>= 1)
  uint32_t maxSize = 0;    // the largest, in bytes or float words
  bool useChecksum = false;
  bool userHist = false;   // byte codec: the caller's histograms
  PreHist pre = PreHist::kNone;
  uint32_t preRows = 0;    // PartialHist::nRows
  bool inAligned16 = false;
  int mode = 0;            // compressPath(): 0 the rule, 1 single-pass, 2 three-kernel
  // workgroups of k_pcompress and of k_encode's prologue instance resident on
  // the device at once; its CUs
  uint32_t pcompressSlots = 1, encodeProSlots = 1, cus = 1;
};

// Why a batch does not go single-pass, in the order the rule asks.
enum class Refused : uint8_t {
  kNot,          // it does
  kTwoSegments,  // fp64: k_pcompress codes one segment
  kUserHist,     // the caller's histogram: nothing to count
  kUnaligned,    // k_pcompress reads whole 16 B vectors
  kForced,       // mode 2 (dietgpu_set_compress_path: test hook)
  kTooLarge,     // an element of more than pc::kMaxTeam items
  kSizeRule,     // too few items, or one round of unaligned teams (below)
};

enum class HistKernel : uint8_t { kPlain, kChecksum, kRows };  // the k_hist instance

// Who turns an element's histogram into its encode table.
enum class Normalise : uint8_t {
  kCaller,    // PartialHist::table: straight to k_encode
  kPrologue,  // every k_encode workgroup, from k_hist's atomic rows (kProRows)
  kInHist,    // the element's last k_hist workgroup
  kInReduce,  // the last k_histReduce workgroup of the element and segment
  kKernel,    // a k_normalize launch
};

struct CompressPlan {
  bool singlePass = false;
  Refused refused = Refused::kNot;
  uint32_t maxBlocks = 0;  // 4096-symbol blocks of the largest element
  uint32_t team = 0;       // ... and its k_pcompress items
  bool rawCk = false;      // byte codec with a checksum: k_pcompress's kCk, k_hist's kChecksum

  // --- single pass (zero otherwise) ---
  bool tooManyItems = false;  // nb * team >= 2^30: the driver refuses the call
  uint32_t rounds = 0, teamsPerRound = 0;  // teamsPerRound: also PCompArgs::teams
  bool xcd = false;     // teams laid out XCD-aligned (k_pcompress's kXcd)
  uint32_t grid = 0;    // workgroups: teamsPerRound teams
  uint32_t maxR = 0;    // rounds a team logs at most
  uint32_t items = 0;   // nb * team
  uint32_t slotSpan = 0;
  uint64_t spillSlots = 0;  // of kSlotDataBytes
  uint64_t floatCkWords = 0;
  uint64_t flagBytes = 0, partialBytes = 0, logBytes = 0;  // arena regions

  // --- three kernels (otherwise zero, `normalise` left at kKernel) ---
  uint32_t chunkWords = 0, chunks = 0, groups = 0;  // k_hist chunks per element, k_histReduce groups
  bool runHist = false;  // k_hist runs (not with the caller's rows; with the caller's histogram for a checksum only)
  HistKernel hist = HistKernel::kPlain;
  Normalise normalise = Normalise::kKernel;
  uint32_t encodeWGs = 0;  // k_encode workgroups per element
  bool encodeRuns = false;
  bool coalesceFromFlags = false;  // the look-back flags feed k_coalesce (single-segment: always in use)
  uint32_t rowsPer = 0;            // kPrologue: proRowsOf(chunks)
  // scratch allocations in elements of their type, in allocation order
  uint64_t partHist = 0, partCk = 0, groupHist = 0, groupCk = 0, ck = 0, table = 0, pdf = 0;
  uint64_t slots = 0;  // of kSlotBytes
  uint64_t cw = 0;
  uint64_t lookbackBytes = 0, arriveBytes = 0, rowsBytes = 0;  // arena regions
};

namespace cplan {
constexpr uint64_t divUp(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
constexpr uint64_t roundUp(uint64_t a, uint64_t b) { return divUp(a, b) * b; }
}  // namespace cplan

// k_hist chunk (words): 4 K .. 64 K words, halved while the batch has fewer
// than 2,048 chunks -- for single-segment formats only down to 16 K words
// once there are 512: a k_hist workgroup zeroes and sums 32 KB of LDS
// counters, which 4 K- or 8 K-word chunks do not amortise (1 x 16M bf16
// compress 41.6 -> 37.0 us, fp32 48.2 -> 46.3 us, same box; 1e8-word
// elements keep their 32 K-word chunks, 64 K measured slower).  fp64's two
// 16-column counter sets keep the 2,048 rule.  Doubled while an element has
// more than 4096 chunks.
inline uint32_t histChunkWords(uint32_t nb, uint32_t maxSize, int segs) {
  uint32_t chunk = 64 * 1024;
  auto enough = [&](uint32_t c) {
    const uint64_t total = uint64_t(nb) * cplan::divUp(std::max(maxSize, 1u), c);
    return total >= 2048 || (segs == 1 && c <= 16 * 1024 && total >= 512);
  };
  while (chunk > 4096 && !enough(chunk)) chunk /= 2;
  while (cplan::divUp(maxSize, chunk) > 4096) chunk *= 2;
  return chunk;
}

inline CompressPlan planCompress(const CompressShape& sh) {
  using cplan::divUp;
  CompressPlan p;
  const uint64_t nb = sh.nb;
  const uint32_t MB = uint32_t(divUp(sh.maxSize, cplan::kBlockWords));  // blocks of the largest element
  const bool rawCk = sh.byteCodec && sh.useChecksum;
  p.maxBlocks = MB;
  p.team = std::max(1u, uint32_t(divUp(MB, pc::kBlocksPerItem)));
  p.rawCk = rawCk;

  // ---- which path ----
  // Teams of k_pcompress in rounds of whole teams, balanced: R rounds of
  // ceil(nb / R) teams.  XCD-aligned teams (kXcd, pcompress.h) whenever the
  // teams per round round up to a multiple of 8 within the resident grid
  // (never more rounds; a batch of fewer than 8 elements gets idle teams that
  // exit at once), so the partial histograms stay in one L2.  Otherwise (e.g.
  // 33 elements of 31 items in 1,024 slots) the team members span XCDs and
  // the partials go out write-through.
  const uint64_t maxTeams = std::max(1u, sh.pcompressSlots / p.team);
  const uint32_t rounds = uint32_t(divUp(nb, maxTeams));
  uint32_t teamsPerRound = uint32_t(divUp(nb, rounds));
  const bool xcd = cplan::roundUp(teamsPerRound, cplan::kXcds) <= maxTeams;
  if (xcd) teamsPerRound = uint32_t(cplan::roundUp(teamsPerRound, cplan::kXcds));
  // The size rule: at most 256 items, or one round whose teams cannot be
  // XCD-aligned, leave most of the chip idle while a team's members wait on
  // each other's partial histograms; there the chip-wide histogram pass plus
  // the encoder are faster (bf16: 1 x 1e6 words 30.7 -> 22.9 us, 8 x 524288
  // 26.9 -> 25.1 us, 33 x 1e6 48.9 -> 46.9 us; 16 x 1e6, 496 items, stays
  // single-pass: 33.5 against 37.1 us).  A byte archive with a checksum goes
  // single-pass whatever its size: the three-kernel path has no prologue
  // normalisation for it.  Mode 1 (test hook) skips the rule.
  const bool sized = sh.mode == 1 || rawCk || (nb * p.team > kMinPersistentItems && !(rounds == 1 && !xcd));
  p.refused = sh.segs != 1                ? Refused::kTwoSegments
              : sh.userHist              ? Refused::kUserHist
              : !sh.inAligned16          ? Refused::kUnaligned
              : sh.mode == 2             ? Refused::kForced
              : p.team > pc::kMaxTeam    ? Refused::kTooLarge
              : !sized                   ? Refused::kSizeRule
                                         : Refused::kNot;
  p.singlePass = p.refused == Refused::kNot;

  if (p.singlePass) {
    if (nb * p.team >= (1ull << 30)) {
      p.tooManyItems = true;
      return p;
    }
    p.rounds = rounds;
    p.teamsPerRound = teamsPerRound;
    p.xcd = xcd;
    p.grid = teamsPerRound * p.team;
    p.items = uint32_t(nb * p.team);
    // A team takes at most maxR rounds (pcompress.h, "Teams and elements"):
    // twice the static share bounds the log while leaving the teams below it
    // room for every element.
    p.maxR = 2 * uint32_t(divUp(nb, teamsPerRound)) + 2;
    p.slotSpan = std::max(1u, sh.cus);
    p.spillSlots = uint64_t(p.grid) * pc::kBlocksPerItem;
    p.floatCkWords = !sh.byteCodec && sh.useChecksum ? nb : 1;
    // per item: a look-back flag, a tagged partial histogram, then (rawCk) a
    // tagged partial checksum; per team and round: a log entry
    p.flagBytes = uint64_t(p.items) * 8;
    p.partialBytes = uint64_t(p.items) * cplan::kSymbols * 4 + (rawCk ? uint64_t(p.items) * 4 : 0);
    p.logBytes = uint64_t(teamsPerRound) * p.maxR * 8;
    return p;
  }

  // ---- three kernels ----
  const uint64_t segs = uint64_t(sh.segs);
  const bool fused = sh.segs == 1;  // k_encode writes the archive itself
  const bool preHist = sh.pre != PreHist::kNone;
  const bool preNorm = sh.pre == PreHist::kRowsAndTable;
  p.chunkWords = histChunkWords(sh.nb, sh.maxSize, sh.segs);
  p.chunks = preHist ? std::max(1u, sh.preRows) : std::max(1u, uint32_t(divUp(sh.maxSize, p.chunkWords)));
  p.groups = uint32_t(divUp(p.chunks, kReduceRows));
  p.runHist = !preHist && (!sh.userHist || sh.useChecksum);
  p.encodeWGs = std::max(1u, uint32_t(divUp(MB, kEncBlocksPerWG)));
  p.encodeRuns = MB > 0 || fused;
  p.coalesceFromFlags = fused || MB > kCoalFlagBlocks;

  // Prologue normalisation (k_encode<.., kPro>, encode.h proNormalize): when
  // the encode grid is at most two generations of resident workgroups.  Not
  // for byte archives with a checksum (their partial checksums are summed by
  // the normalisation kernels) nor for caller-supplied histograms, and only
  // while the rows stay within kProRowsBudget.
  const uint64_t proRowsBytes = segs * nb * proRowsOf(p.chunks) * cplan::kSymbols * 4;
  const bool pro = p.runHist && !sh.userHist && !rawCk && MB > 0 && proRowsBytes <= kProRowsBudget &&
                   nb * p.encodeWGs <= 2ull * sh.encodeProSlots;
  if (preNorm) p.normalise = Normalise::kCaller;
  else if (pro) p.normalise = Normalise::kPrologue;
  else if ((p.runHist || preHist) && p.chunks > kReduceRows) p.normalise = Normalise::kInReduce;
  else if (p.runHist && uint64_t(p.chunks) * nb <= kMaxLastArrivalWGs) p.normalise = Normalise::kInHist;
  else p.normalise = Normalise::kKernel;
  p.hist = pro ? HistKernel::kRows : rawCk ? HistKernel::kChecksum : HistKernel::kPlain;
  p.rowsPer = pro ? proRowsOf(p.chunks) : 0;

  const bool reduce = p.normalise == Normalise::kInReduce;
  const uint64_t tables = segs * nb * cplan::kSymbols;  // a 256-entry row per segment and element
  p.partHist = p.runHist && !pro ? tables * p.chunks : 1;
  p.partCk = rawCk ? nb * p.chunks : 1;
  p.groupHist = reduce ? tables * p.groups : 1;
  p.groupCk = reduce && rawCk ? nb * p.groups : 1;
  p.ck = nb;
  p.table = p.pdf = preNorm ? 1 : tables;
  p.slots = segs * nb * std::max(MB, 1u);
  p.cw = fused ? 1 : segs * nb * std::max(MB, 1u);
  // k_encode's look-back flags (one per segment, element and encode
  // workgroup, epoch-tagged, never zeroed; fp64's end as the prefixes
  // k_coalesce reads), the last-arrival counters and (kPrologue) the
  // histogram rows
  p.lookbackBytes = segs * nb * p.encodeWGs * 8;
  p.arriveBytes = nb * segs * 4;
  p.rowsBytes = pro ? proRowsBytes : 0;
  return p;
}

}  // namespace dietgpu
