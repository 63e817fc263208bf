"""Case tables and the model of the pooled row gather: the
row widths, for each width the bag lists with the edge kinds each list claims
to hold, the value tables, and the sequential fp32 model the kernel is compared
with bit for bit.  numpy and torch on the CPU only; runs none of the codec.
tests/test_gather_sum_inputs.py checks the claims and that the model tells a
wrong sum from a right one, tests/test_gpu_gather_sum.py runs the lists."""
import itertools

import numpy as np
import torch

from tests import gather_cases as G

BLK = G.BLK
N_TABLE = G.N_TABLE  # 17 x 4096 + 1234 words: gather_cases' table
TILE = 128  # kGatherSumTile (csrc/decode_plan.h): the columns of one task
TASKS_PER_WG = 8
ROW_WORDS = (1, 7, 8, 64, TILE - 1, TILE, TILE + 1, 257, 1024, 4097)
LENGTHS = (0, 1, 2, 3, 17, 700)
LONG_RW, LONG_BAGS = 8, 70000  # more task groups than resident workgroups
INT64_MIN = G.INT64_MIN


def tiles_of(rw):
    return -(-rw // TILE)


def flatten(bags):
    """-> (idx, offsets) lists of a list of bags."""
    idx = [r for bag in bags for r in bag]
    offsets = [0] + list(itertools.accumulate(len(bag) for bag in bags))
    return idx, offsets


def bag_lists(rw):
    """name -> (bags, set of kinds the list claims).  Kinds: "len0" .. "len700"
    (a bag of that length), "repeat" (a bag repeating one row), "misaligned"
    (a bag whose rows start at different in-block offsets, in different
    blocks), "edge_neighbours" / "ends_on_edge" / "straddles" (gather_cases'
    kinds, the rows pooled in one bag and alone), "first", "last",
    "tail_block", "idle_half" (an odd task count), "empty_first",
    "empty_last", "empty_adjacent"."""
    R = G.rows_of(rw)
    rng = np.random.default_rng(2000 + rw)
    lists = {}
    bags = [rng.integers(0, R, n).tolist() for n in LENGTHS]
    lists["lengths"] = (bags, {f"len{n}" for n in LENGTHS})
    lists["repeat"] = ([[R // 2] * 5], {"repeat"})
    # rows spread over the table, one further into its block than the last
    # where the width allows it
    spread, seen = [], set()
    period = BLK // int(np.gcd(rw, BLK))  # distinct in-block starts a row can have
    for k in range(5):
        r = k * (R // 5)
        while (r * rw) % BLK in seen and len(seen) < period and r + 1 < (k + 1) * (R // 5):
            r += 1
        seen.add((r * rw) % BLK)
        spread.append(r)
    lists["misaligned"] = ([spread, spread[::-1]], {"misaligned"})
    edge, kinds = G.index_lists(rw)["edges"]
    lists["edges"] = ([edge] + [[r] for r in edge[:6]], set(kinds))
    last_kinds = {"first", "last"} | ({"tail_block"} if G.in_tail_block(R - 1, rw) else set())
    lists["ends"] = ([[0], [R - 1], [0, R - 1], [R - 1, 0]], last_kinds)
    odd = [[1 % R], [R // 3, R // 2], [R - 1]]
    lists["odd"] = (odd, {"idle_half"} if (len(odd) * tiles_of(rw)) % 2 else set())
    lists["empties"] = ([[], [], [R // 4], [], [], [R // 2, 0], []],
                        {"empty_first", "empty_last", "empty_adjacent", "len0"})
    return lists


def all_bags(rw):
    """Every list of the width in one call, in name order."""
    return [bag for _, (bags, _) in sorted(bag_lists(rw).items()) for bag in bags]


def long_bags():
    """70,000 bags of one or two 8-word rows."""
    rng = np.random.default_rng(78)
    R = G.rows_of(LONG_RW)
    lens = rng.integers(1, 3, LONG_BAGS)
    rows = rng.integers(0, R, int(lens.sum())).tolist()
    ends = np.cumsum(lens).tolist()
    return [rows[e - n:e] for e, n in zip(ends, lens.tolist())]


def row_offsets_and_blocks(bag, rw):
    """The in-block start offsets and the first blocks of a bag's rows."""
    return {(r * rw) % BLK for r in bag}, {(r * rw) // BLK for r in bag}


def table_words(ft, n=N_TABLE, seed=0):
    """The table's words (unsigned numpy, as tests/util.float_words): N(0, 1)
    times 2^k, k uniform in -12 .. 12.  Sums of N(0, 1) fp16 / bf16 values are
    exact in fp32 in any order; over 24 binades the fp32 adds round, so the
    order of the adds and the width of the running sum show in the result."""
    rng = np.random.default_rng(9000 + 10 * seed + ft)
    f = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 13, n))).astype(np.float32)
    if ft == 1:
        return f.astype(np.float16).view(np.uint16)
    if ft == 2:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    return f.view(np.uint32)


def as_ints(words):
    """numpy words -> a CPU tensor of signed integers of their width."""
    return torch.from_numpy(words.view({2: np.int16, 4: np.int32}[words.itemsize]).copy())


# ------------------------------------------------------------------- model ----

def pooled(table, rw, bags, out_dtype, order=1, acc_dtype=torch.float32, start_zero=False):
    """The model: table a 1-d CPU float tensor (the archive's type), its first
    (numel // rw) * rw words the rows.  Bag b -> row b of the result: the
    running sum starts as the first row converted to fp32 and takes the other
    rows in list order, one fp32 add each; one rounding to out_dtype; an empty
    bag gives +0.0.  The wrong kernels of test_gather_sum_inputs.py: order -1
    adds in reverse list order, acc_dtype keeps the running sum in another
    type, start_zero starts it as +0.0."""
    R = table.numel() // rw
    rows = table[: R * rw].view(R, rw)
    B = len(bags)
    out = torch.zeros([B, rw], dtype=acc_dtype)
    longest = max([len(b) for b in bags], default=0)
    seq = [b[::order] for b in bags]
    for t in range(longest):
        who = [b for b in range(B) if len(seq[b]) > t]
        term = rows[torch.tensor([seq[b][t] for b in who], dtype=torch.int64)].to(acc_dtype)
        sel = torch.tensor(who, dtype=torch.int64)
        if t == 0 and not start_zero:
            out[sel] = term
        else:
            out[sel] = out[sel] + term
    return out.to(out_dtype)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(got, want):
    """Bitwise where the model is not NaN, NaN where it is -> bool tensor."""
    return (bits(got) == bits(want)) | (torch.isnan(want) & torch.isnan(got))


# ------------------------------------------------------------ value tables ----

def all_patterns(dtype):
    """Every 16-bit pattern as rows of 64 words (1024 rows), followed by a
    second vector of the patterns in another order: row r pooled with row
    1024 + r adds pattern p to pattern (p * 40503 + 12345) % 65536."""
    p = np.arange(65536, dtype=np.int64)
    q = (p * 40503 + 12345) % 65536
    both = np.concatenate([p, q]).astype(np.uint16).view(np.int16)
    return torch.from_numpy(both.copy()).view(dtype)


def pattern_pairs():
    return [[r, 1024 + r] for r in range(1024)]


def fp32_specials():
    """fp32 values whose sums round, cancel, overflow, underflow or are NaN:
    a [k * k, 8] table whose row i * k + j holds special i in every word, pooled
    with row j * k + i it adds every pair in both orders."""
    s = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x80800000, 0x7f7fffff,
                  0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0x3f800000, 0xbf800000, 0x33800000,
                  0x33800001, 0x4b800000, 0x3f7fffff, 0x3f800001], dtype=np.uint32)
    k = s.size
    table = np.repeat(np.repeat(s, k), 8)
    bags = [[i * k + j, j * k + i] for i in range(k) for j in range(k)]
    return torch.from_numpy(table.view(np.int32).copy()).view(torch.float32), bags


def order_probe(dtype):
    """In the style of reduce_cases.order_probe: rows of 8 words holding 1.0,
    2^-24, 2^-24 and -1.0 and one bag per permutation of the four.  1 + 2^-24
    ties to 1 in fp32, so orders that meet 1.0 first lose the small terms and
    orders that add them first keep 2^-23: the sums differ between orders.
    -> (table, bags)."""
    vals = (1.0, 2.0 ** -24, 2.0 ** -24, -1.0)
    table = torch.tensor(vals, dtype=torch.float64).repeat_interleave(8).to(dtype)
    return table, [list(p) for p in itertools.permutations(range(4))]


# ---------------------------------------------------------------- failures ----

def failing_bags(rw, wide):
    """(bags, expect ok): every bad index of gather_cases.failing_indices in a
    bag of its own among good rows (first, middle and last in the bag), good
    bags and an empty one between them."""
    R = G.rows_of(rw)
    bags, ok = [], []
    for k, bad in enumerate(G.failing_indices(rw, wide)):
        good = [0, R - 1, R // 2]
        bag = good[:]
        bag.insert(k % 4, bad)
        bags += [[R // 3, 0], bag, []]
        ok += [1, 0, 1]
    bags.append([R - 1])
    ok.append(1)
    return bags, ok
