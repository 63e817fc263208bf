"""The case table and the expected values of the grid-Y slice tests
(tests/test_gpu_slices.py on the GPU, tests/test_slice_inputs.py on the CPU;
DESIGN.md 4, "Batches of any size").

A batch member is a row of a kernel's grid (blockIdx.y), at most GRID_Y rows
per launch: the drivers cut a batch into slices (forGridYSlices,
csrc/codec_internal.h) and hand each kernel its slice's first member.  A
kernel that indexes an array by blockIdx.y alone treats member i as member
i - GRID_Y.  The batches here make that visible: member i holds content
i % K_DISTINCT, whose size and words both depend on the index, and 7 divides
neither 65,535 nor 131,070.  Accumulator and init values cycle with the same
period, ACC_SHIFT further on.

An empty member takes paths of its own in the kernels (an empty element's
header, its zero table, a list length of 0), which write per-member arrays too.
So the families whose size-edge tables hold an empty member (the pointer-form
dense compress and decode, decode-accumulate, sparse compress, decompress and
accumulate) replace the members empty_members() by content EMPTY, of no
words: member 3, member 65,536 and member 131,070, where the batch has
them.  The stride-form compress has one row length, and the range decodes, the reduces,
the info readouts and the operator test keep the seven contents alone.

The expected values are the oracle's archives, plain slices of the inputs, or
the CPU models of tests/accumulate_cases.py, tests/reduce_cases.py,
tests/sparse_accumulate_cases.py and tests/sparse_reduce_cases.py: never the
code under test.  Seeded; numpy and torch on the CPU only."""
import numpy as np
import torch

from tests import accumulate_cases as A
from tests import reduce_cases as R
from tests import sparse_accumulate_cases as S
from tests import sparse_range_cases as SRG
from tests import sparse_reduce_cases as SR
from tests.util import NP_W, exp_bytes, float_words, sparsify

GRID_Y = 65535  # kMaxGridY (csrc/codec_internal.h)

# member counts: one full slice (the control: nothing is sliced), a second
# slice of one member, of two, and three slices with a last one of one member
CONTROL = GRID_Y
COUNTS = (GRID_Y, GRID_Y + 1, GRID_Y + 2)
THREE_SLICES = 2 * GRID_Y + 1
# the sparse reduce slices its chunk count over sources-per-pass x nb rows:
# at INNER_K sources, 65,536 and 65,540 rows
INNER_K = 4
INNER_COUNTS = (16384, 16385)
ALL_COUNTS = COUNTS + (THREE_SLICES,) + INNER_COUNTS

K_DISTINCT = 7
ACC_SHIFT = 3
# words (bytes for the byte codec) of the seven contents: 4097 has a second
# ANS block, 1025 a second 1024-word sparse chunk
SIZES = (1, 33, 255, 1024, 1025, 4096, 4097)
ROW = 4097  # words of every row of a stride-form compress
# of the sparse contents: all words +0.0 / no word +0.0
SPARSE_ALL_ZERO, SPARSE_ZERO_FREE = 2, 4
EMPTY = K_DISTINCT  # the index of the empty content, after the seven
CONTENTS = K_DISTINCT + 1
ALL_SIZES = SIZES + (0,)


def which(i):
    """The content of member i (an index or a numpy array of indices)."""
    return i % K_DISTINCT


def acc_which(i):
    """The accumulator / init values of member i."""
    return (i + ACC_SHIFT) % K_DISTINCT


def empty_members(nb):
    """The members that hold content EMPTY in the families that take one:
    member 3, the second member of the second slice (its first is the
    decode's short-capacity member) and the one member of the third slice.  The
    members GRID_Y and 2 * GRID_Y before each of the latter are not empty.
    A batch of 65,536 members has its one empty member in the first slice: its
    second slice is member 65,535 alone, which stays a non-empty one, and the
    empty-member paths run past the first slice from 65,537 members on."""
    return [i for i in (3, GRID_Y + 1, 2 * GRID_Y) if i < nb]


def member_contents(nb, empty=False):
    """The content index of every member (numpy int64 [nb])."""
    w = which(np.arange(nb, dtype=np.int64))
    if empty:
        w[empty_members(nb)] = EMPTY
    return w


def named_members(nb):
    """The members a test asserts on one by one, by name: both sides of each
    slice edge, the inner row edge of the sparse reduce (row 65,535 is member
    16,383 of the fourth source at 16,384 members) and the last member."""
    pick = (0, 3, 16383, 16384, GRID_Y - 1, GRID_Y, GRID_Y + 1, 2 * GRID_Y - 1, 2 * GRID_Y, nb - 1)
    return sorted({i for i in pick if 0 <= i < nb})


# ------------------------------------------------------------------ contents ----

def words(ft, c, src=0):
    """Content c (SIZES[c] words of float type ft, bytes for ft 0) of source
    `src` (the reduces take several elements of one size per member).  All
    contents of a type share one distribution."""
    seed = 500 + 10 * src + c
    n = ALL_SIZES[c]
    w = exp_bytes(n, lam=20.0, seed=seed) if ft == 0 else float_words(ft, n, seed=seed)
    if ft == 0 and n:
        w[0] = 3 + 5 * c + src  # the one byte of content 0 differs from the others' first
    return w


def row_words(ft, c):
    """Content c of the stride-form compress: ROW words each."""
    seed = 560 + c
    return exp_bytes(ROW, lam=20.0, seed=seed) if ft == 0 else float_words(ft, ROW, seed=seed)


def sparse_words(ft, c, src=0):
    """The sparse version of words(): 90 % zeros at seeded positions, content
    SPARSE_ALL_ZERO all zeros and SPARSE_ZERO_FREE without a zero (source 0;
    the further sources of a reduce are all 90 % zeros)."""
    w = words(ft, c, src)
    if c == EMPTY:
        return w
    if src == 0 and c == SPARSE_ALL_ZERO:
        return np.zeros_like(w)
    if src == 0 and c == SPARSE_ZERO_FREE:
        return w | NP_W[ft](1)
    s = sparsify(w, 0.9, seed=600 + 10 * src + c)
    s[0] = w[0] | NP_W[ft](1)  # a one-word content is not the all-zero one's prefix
    return s


def acc_values(ft, mode, a, sparse=False):
    """Accumulator / init values `a` (0 .. 6): max(SIZES) values of the
    accumulator's dtype, a member takes the first SIZES[content] of them.
    sparse: every fifth one -0.0 (sparse_accumulate_cases.case_acc)."""
    make = S.case_acc if sparse else A.random_acc
    return make(ft, mode, max(SIZES), seed=640 + a)


def ranges(n, count):
    """(firsts, counts), `count` of each: sparse_range_cases.edge_ranges(n),
    the non-empty ones first, cycled."""
    r = sorted(SRG.edge_ranges(n), key=lambda fc: fc[1] == 0)
    r = np.array([r[j % len(r)] for j in range(count)], dtype=np.int64).reshape(count, 2)
    return r[:, 0], r[:, 1]


def member_ranges(nb):
    """(firsts, counts) int64 [nb]: member i reads range (i // 7) of its
    content's ranges(), so that members GRID_Y apart differ in content, first
    and (mostly) count."""
    firsts = np.zeros(nb, dtype=np.int64)
    counts = np.zeros(nb, dtype=np.int64)
    for c in range(K_DISTINCT):
        m = np.arange(c, nb, K_DISTINCT)
        firsts[m], counts[m] = ranges(SIZES[c], m.size)
    return firsts, counts


# ----------------------------------------------------------- expected values ----

def accumulate_rows(ft, mode):
    """[8] torch CPU tensors: content c's accumulator after the call."""
    return [A.model(acc_values(ft, mode, acc_which(c))[:ALL_SIZES[c]], A.words_to_float(words(ft, c), ft), mode)
            for c in range(CONTENTS)]


def sparse_accumulate_rows(ft, mode):
    return [S.expected(acc_values(ft, mode, acc_which(c), sparse=True)[:ALL_SIZES[c]], sparse_words(ft, c), ft, mode)
            for c in range(CONTENTS)]


def reduce_rows(ft, K):
    """[7] torch CPU tensors of the archives' type: fp32 init + K sources."""
    return [R.model([A.words_to_float(words(ft, c, k), ft) for k in range(K)],
                    init=acc_values(ft, SR.acc_mode(ft), acc_which(c))[:SIZES[c]], out_dtype=A.TORCH_FLOAT[ft])
            for c in range(K_DISTINCT)]


def sparse_reduce_rows(ft, K):
    return [SR.model([sparse_words(ft, c, k) for k in range(K)], ft,
                     init=acc_values(ft, SR.acc_mode(ft), acc_which(c), sparse=True)[:SIZES[c]],
                     out_dtype=A.TORCH_FLOAT[ft])
            for c in range(K_DISTINCT)]


def padded(rows, width=None, fill=0):
    """[7, width] numpy: the rows (numpy, one dtype), each filled up."""
    width = max(r.size for r in rows) if width is None else width
    out = np.full([len(rows), width], fill, dtype=rows[0].dtype)
    for k, r in enumerate(rows):
        out[k, : r.size] = r
    return out


def bit_words(t):
    """The bits of a torch CPU float tensor as unsigned numpy words."""
    return A.bits(t).numpy().view({2: np.uint16, 4: np.uint32, 8: np.uint64}[t.element_size()]).copy()


# ------------------------------------------------------------------ the table ----
# Every GPU test of tests/test_gpu_slices.py is one row (its parametrisation).
# A compress writes rows of the codec's bound, 572 KB per bf16 member, so only
# one compress takes THREE_SLICES (75 GB), beside the dense and sparse decodes.

# (id, ft, form, checksum, caller histogram, nb)
COMPRESS_THREE_KERNEL = [
    ("bf16-pointer-65535", 2, "pointer", False, False, 65535),
    ("bf16-pointer-65536", 2, "pointer", False, False, 65536),
    ("bf16-pointer-65537", 2, "pointer", False, False, 65537),
    ("bf16-pointer-131071", 2, "pointer", False, False, THREE_SLICES),
    ("bf16-pointer-ck-65537", 2, "pointer", True, False, 65537),
    ("bytes-pointer-65537", 0, "pointer", False, False, 65537),
    ("bytes-pointer-ck-65537", 0, "pointer", True, False, 65537),
    ("fp32-pointer-65537", 3, "pointer", False, False, 65537),
    ("fp64-pointer-65537", 4, "pointer", False, False, 65537),
    ("bf16-stride-65537", 2, "stride", False, False, 65537),
    ("bytes-stride-userhist-65537", 0, "stride", False, True, 65537),
]
# (id, ft, nb): pointer form, checksum on
COMPRESS_SINGLE_PASS = [
    ("bf16-ck-65535", 2, 65535),
    ("bf16-ck-65537", 2, 65537),
    ("bytes-ck-65537", 0, 65537),
]
# (id, ft, form, checksum, a member with a short capacity, nb)
DECODE = [
    ("bf16-pointer-65535", 2, "pointer", False, False, 65535),
    ("bf16-pointer-65536", 2, "pointer", False, False, 65536),
    ("bf16-pointer-65537", 2, "pointer", False, False, 65537),
    ("bf16-pointer-131071", 2, "pointer", False, False, THREE_SLICES),
    ("bytes-pointer-short-65537", 0, "pointer", False, True, 65537),
    ("fp16-pointer-65537", 1, "pointer", False, False, 65537),
    ("fp32-pointer-ck-65537", 3, "pointer", True, False, 65537),
    ("fp64-pointer-short-65537", 4, "pointer", False, True, 65537),
    ("fp16-stride-65537", 1, "stride", False, False, 65537),
    ("bytes-stride-65537", 0, "stride", False, False, 65537),
]
SHORT_MEMBER = GRID_Y  # the second slice's first member, content 1: 33 words into a capacity of 32
# (id, ft, nb)
RANGE = [("bf16-65537", 2, 65537), ("bytes-65537", 0, 65537)]
# (id, ft, mode, nb)
ACCUMULATE = [("bf16-bf16-65535", 2, 1, 65535), ("bf16-bf16-65537", 2, 1, 65537), ("bf16-fp32-65537", 2, 2, 65537),
              ("fp32-65537", 3, 1, 65537)]
REDUCE_K = 3
# (id, sources per launch (0: the default), nb)
REDUCE = [("default-65535", 0, 65535), ("default-65537", 0, 65537), ("two-passes-65537", 2, 65537)]
# (id, ft, nb)
SPARSE_COMPRESS = [("bf16-65535", 2, 65535), ("bf16-65537", 2, 65537), ("fp32-65537", 3, 65537)]
SPARSE_DECOMPRESS = [("bf16-65535", 2, 65535), ("bf16-65537", 2, 65537), ("bf16-131071", 2, THREE_SLICES)]
# (id, ft, mode, nb)
SPARSE_ACCUMULATE = [("bf16-bf16-65537", 2, 1, 65537), ("bf16-fp32-65537", 2, 2, 65537)]
SPARSE_RANGE = [("bf16-65537", 2, 65537)]
# (id, nb): bf16, INNER_K sources
SPARSE_REDUCE = [("65537", 65537), ("16384", 16384), ("16385", 16385)]
INFO_NB = 65537
OP_NB = 65537

TABLES = {"compress-three-kernel": COMPRESS_THREE_KERNEL, "compress-single-pass": COMPRESS_SINGLE_PASS,
          "decode": DECODE, "range": RANGE, "accumulate": ACCUMULATE, "reduce": REDUCE,
          "sparse-compress": SPARSE_COMPRESS, "sparse-decompress": SPARSE_DECOMPRESS,
          "sparse-accumulate": SPARSE_ACCUMULATE, "sparse-range": SPARSE_RANGE, "sparse-reduce": SPARSE_REDUCE}


def table_counts():
    """Every member count a test runs."""
    return sorted({row[-1] for t in TABLES.values() for row in t} | {INFO_NB, OP_NB})


def ids(table):
    return [row[0] for row in table]
