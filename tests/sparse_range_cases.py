"""Inputs of the sparse range-decode tests (tests/test_gpu_sparse_range.py on
the GPU, tests/test_sparse_range_inputs.py on the CPU): which elements, which
ranges of each, and a numpy restatement of the rank identity the kernels
implement, so that the identity is checked against plain
slicing before any kernel runs.  Seeded, numpy only."""
import numpy as np

from tests.util import SPARSE_FAR_N, SPARSE_LARGE_B, float_words, sparsify

# a thinned selection of sparse_edge_sizes(): around the 64-word row, the
# 1024-word chunk, the 4096-word list block / tile and the 262,144-word scan
# workgroup
EDGE_SMALL = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
EDGE_LARGE = (SPARSE_LARGE_B - 1, SPARSE_LARGE_B, SPARSE_LARGE_B + 1)
EDGE_POINTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)


def edge_names(sizes):
    """The names sparse_edge_elements() gives the elements of these sizes:
    all four x[n-2] / x[n-1] combinations (n == 1: the two values of x[0])."""
    names = []
    for n in sizes:
        fill = ("zero", "half", "dense")[n % 3]
        tails = ("00", "01", "10", "11") if n >= 2 else ("00", "01")[: n + 1]
        names += [f"n{n}_{fill}_t{t}" for t in tails]
    return names


def edge_ranges(n):
    """(first, count): first <= end both drawn from EDGE_POINTS and n-2, n-1,
    n, clipped to [0, n].  The pairs with first == end are the empty ranges
    (at 0 and at n among them); (0, n) is the whole element."""
    pts = sorted({min(max(p, 0), n) for p in EDGE_POINTS + (n - 2, n - 1, n)})
    return [(a, b - a) for a in pts for b in pts if a <= b]


def rank_table(x):
    """rank[i] = the nonzero words among x[0 : i], 0 <= i <= n."""
    return np.concatenate([[0], np.cumsum(x != 0)]).astype(np.int64)


def model_range(x, lst, first, count):
    """Words [first, first + count) of x from its bitmap and its nonzero list
    `lst` by the rank identity alone: word i < n-1 lives at list index
    rank(i), word n-1 at rank(n-1) + gap, gap = n >= 2 and x[n-2] == 0; the
    slice read is [rank(first), rank(end) + (gap and end == n)), at most
    count + 1 words (an empty range reads nothing).  -> (words, listFirst,
    listCount)."""
    n = x.size
    end = first + count
    assert 0 <= first <= end <= n
    out = np.zeros(count, dtype=x.dtype)
    if count == 0:
        return out, 0, 0
    flag = x != 0
    rank = rank_table(x)
    gap = int(n >= 2 and not flag[n - 2])
    lf = int(rank[first])
    lc = int(rank[end]) - lf + (gap if end == n else 0)
    assert lc <= count + 1 and lf + lc <= lst.size
    piece = lst[lf: lf + lc]
    i = np.arange(first, end)
    idx = rank[i] - lf + np.where(i == n - 1, gap, 0)
    sel = flag[i]
    out[sel] = piece[idx[sel]]
    return out, lf, lc


LIST_BLOCK_N = 3 * 4096 * 2 + 5
LIST_BLOCK_COUNTS = (1, 2, 9000)
LIST_BLOCK_RANKS = (4095, 4096, 4097)


def list_block_element(ft):
    """Half-zero, 3 x 4096 x 2 + 5 words: a nonzero list of about three dense
    rANS blocks."""
    return sparsify(float_words(ft, LIST_BLOCK_N, seed=40 + ft), 0.5, seed=50 + ft)


def list_block_ranges(x):
    """first such that rank(first) is 4095, 4096 and 4097 (the word after the
    4095th, 4096th, 4097th nonzero), each with counts 1, 2 and 9000: the list
    slice starts before, on and after the dense codec's block edge, and the
    long ones span three blocks."""
    rank = rank_table(x)
    out = []
    for r in LIST_BLOCK_RANKS:
        first = int(np.searchsorted(rank, r, side="left"))
        assert rank[first] == r and first + max(LIST_BLOCK_COUNTS) <= x.size
        out += [(first, c) for c in LIST_BLOCK_COUNTS]
    long_slice = rank[out[2][0] + 9000] - rank[out[2][0]]
    assert 4095 + long_slice > 2 * 4096  # blocks 0, 1 and 2
    return out


WG_N = 2 * SPARSE_LARGE_B + 1102


def wg_element():
    """bf16, half-zero, 2 x 262,144 + 1102 words: three counting workgroups,
    the last a partial one."""
    return sparsify(float_words(2, WG_N, seed=60), 0.5, seed=61)


def wg_ranges():
    """Ranges ending before, on and after words 262,144 and 524,288 (where a
    rank starts adding a workgroup total), starting on each side of them, and
    reaching the element's end."""
    out = []
    for e in (SPARSE_LARGE_B, 2 * SPARSE_LARGE_B):
        out += [(e - 5, 4), (e - 5, 5), (e - 5, 6), (e - 1, 1), (e, 1), (e + 1, 7), (e - 1030, 2060),
                (e - 1, 1025), (e, 0)]
    out += [(2 * SPARSE_LARGE_B - 3, 1105), (2 * SPARSE_LARGE_B, 1102), (SPARSE_LARGE_B - 1, SPARSE_LARGE_B + 2)]
    return out


def far_ranges():
    """Of sparse_far_element(): inside its first chunk, straddling word
    64 x 262,144 (the second round of the workgroup-total sum), and the last 3
    and the last 1025 words."""
    n = SPARSE_FAR_N
    return [(10, 500), (64 * SPARSE_LARGE_B - 700, 1400), (n - 3, 3), (n - 1025, 1025)]


QUIRK_SIZES = (65, 1025, 4097)
ALL_ONES = {1: 0xFFFF, 2: 0xFFFF, 3: 0xFFFFFFFF, 4: 0xFFFFFFFFFFFFFFFF}


def quirk_ranges(n):
    """Ranges that end at n-1 and at n, and ranges that start at n-1."""
    return [(0, n - 1), (n - 3, 2), (n - 2, 1), (0, n), (n - 2, 2), (n - 5, 5), (n - 1, 1), (n - 1, 0), (n, 0)]


GATHER_ROWS, GATHER_WORDS = 4096, 1024


def gather_table():
    """[4096, 1024] bf16 words at 90 % zeros."""
    return sparsify(float_words(2, GATHER_ROWS * GATHER_WORDS, seed=70), 0.9, seed=71).reshape(GATHER_ROWS,
                                                                                               GATHER_WORDS)


def gather_rows():
    """256 rows with repeats, the first and the last row among them."""
    rng = np.random.default_rng(72)
    rows = rng.integers(0, GATHER_ROWS, 256)
    rows[:4] = (0, GATHER_ROWS - 1, 0, 17)
    rows[200:204] = rows[100:104]
    return rows

