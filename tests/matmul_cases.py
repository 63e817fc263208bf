"""Inputs of the compressed matmuls whose product is exact in fp32 in any order,
tables of special values, and the shapes that tests/test_gpu_matmul_exact.py
runs them at (CPU only: numpy and torch; tests/test_matmul_cases.py checks that
the reference alone meets what the GPU tests demand).

Exact sums.  W[r, k] = a[r, k] * 2^e[k] and x[m, k] = b[m, k] * 2^-e[k], a and b
nonzero signed integers, e[k] an integer per column.  Every product is the
integer a * b whatever k, and with max|a| * max|b| * rowWords < 2^24 every
partial sum of a row, in any order and any grouping, is an integer below 2^24
and so exact in fp32: out must equal the int64 product b @ a.T bit for bit,
from fmaf chains, from the matrix pipe and after the pieces are added.  One
wrong, missing or doubled weight word moves an output by at least 1.

The columns' exponents depend on (ft, rw, e_lo, e_hi) alone, not on the seed,
so that one x serves the tables of every expert of a grouped call."""
import numpy as np
import torch

from tests.util import NP_WORD, TORCH_FLOAT

A_MAX = 127
B_MAX = 15
# e[k] per type: bf16 and fp32 have 8 exponent bits, fp16 has 5
E_RANGE = {1: (-10, 10), 2: (-100, 100), 3: (-100, 100)}
FP16_MAX = 65504

# (rowWords, R) of the "every word counts" runs: 16 pieces per block; period 3,
# rows straddling blocks; period 2, a full group and a tail of two; period 17
WORD_SHAPES = [(256, 150), (768, 50), (8192, 9), (4352, 9)]
# periods 5 (40.6 blocks: a second run starts), 7 and 43 (one live half per group)
PERIOD_SHAPES = [(1280, 130), (1792, 94), (11008, 3)]
# (rowWords, R of the archive, R' of the call): the table ends at segment 4 of
# block 1 with col == 0 on the first dead segment; one row; a block edge and
# one row past it; a row of two blocks, 9 of 30; a row past one block, 1 of 9
PREFIXES = [(768, 50, 7), (768, 50, 1), (256, 150, 17), (256, 150, 16), (8192, 30, 9), (4352, 9, 1)]
CAP_SHAPES = [(1280, 130, 130), (768, 50, 50), (768, 50, 7)]  # (rowWords, R of the archive, R' of the call)
LARGEST_TABLE = 8192 * 30  # words: the existing suites' largest; the largest new shape is 1792 x 94


def b_max(rw):
    """The largest |b| <= B_MAX with A_MAX * |b| * rw < 2^24."""
    return min(B_MAX, ((1 << 24) - 1) // (A_MAX * rw))


def _signed(rng, hi, shape):
    """Nonzero integers in [-hi, hi] (hi an int or an array that broadcasts)."""
    mag = 1 + (rng.integers(0, 1 << 30, shape) % hi)
    return mag * rng.choice(np.array([-1, 1]), shape)


def exponents(ft, rw, e_lo, e_hi):
    rng = np.random.default_rng([ft, rw, e_lo + 1000, e_hi + 1000])
    e = rng.integers(e_lo, e_hi + 1, rw)
    e[:2] = e_lo, e_hi  # both ends occur
    return e


def exact_table(ft, rw, R, seed=0, e_lo=None, e_hi=None):
    """-> (a [R, rw] int64, e [rw] int64, W [R, rw] of the type, on the CPU).
    |a| <= 127, but for fp16 at most FP16_MAX / 2^e[k] (63 at e = 10, where
    127 * 2^10 is no fp16 number).  e_lo == e_hi == 0 is the constant-exponent
    table: a = +-1 (fp16: +1, its sign bit lies in the ANS symbol), so that one
    symbol has probability 1 and no block has a compressed word."""
    lo, hi = E_RANGE[ft]
    e_lo, e_hi = lo if e_lo is None else e_lo, hi if e_hi is None else e_hi
    assert E_RANGE[ft][0] <= e_lo <= e_hi <= E_RANGE[ft][1]
    e = exponents(ft, rw, e_lo, e_hi)
    rng = np.random.default_rng([ft, rw, R, seed, 1])
    if e_lo == e_hi == 0:
        a = np.ones([R, rw], dtype=np.int64) if ft == 1 else _signed(rng, 1, [R, rw])
    else:
        cap = np.full(rw, A_MAX, dtype=np.int64)
        if ft == 1:
            cap = np.minimum(cap, (FP16_MAX / np.exp2(e)).astype(np.int64))
        a = _signed(rng, cap[None, :], [R, rw])
    W = torch.from_numpy(np.ldexp(a.astype(np.float64), e[None, :])).to(TORCH_FLOAT[ft])
    return a.astype(np.int64), e, W


def exact_acts(ft, M, rw, e, seed=0):
    """-> (b [M, rw] int64, x [M, rw] of the type) for a table of exponents e."""
    rng = np.random.default_rng([ft, rw, M, seed, 2])
    b = _signed(rng, b_max(rw), [M, rw]).astype(np.int64)
    x = torch.from_numpy(np.ldexp(b.astype(np.float64), -e[None, :])).to(TORCH_FLOAT[ft])
    return b, x


def exact_product(b, a):
    """b @ a.T in int64, as the fp32 tensor the GPU must produce."""
    p = b @ a.T
    assert np.abs(p).max() < 1 << 24
    return torch.from_numpy(p.astype(np.float32))


def words_of(W, ft):
    """A table's words as the unsigned numpy line the oracle compresses."""
    return W.contiguous().view(torch.int16 if ft != 3 else torch.int32).numpy().view(NP_WORD[ft]).reshape(-1)


def symbols_of(words, ft):
    """The ANS symbol of every word (tests/pyref.py float_split)."""
    w = words.astype(np.uint32)
    return (w >> 8 if ft == 1 else (w >> 7) & 0xFF if ft == 2 else (w >> 23) & 0xFF).astype(np.uint8)


# ------------------------------------------------------------ special values ----
# One finite table per type, (768, 50): ordinary small integers, except that
#  * columns SPECIAL_KS hold, cycling down the rows, SPECIALS[ft]: denormals of
#    both signs (bf16 a * 2^-133, fp16 a * 2^-24, fp32 a * 2^-149), +-0 and
#    +-(the largest finite);
#  * columns MIRROR_KS hold 2^10 in even rows and 1 in odd rows, to meet
#    denormal activations.
# The columns lie in different lanes (k % 256 / 8), chunk words (k % 8) and
# segments (k / 256); the rows put them into every block of the table, and so
# into different half-waves.
SPECIAL_SHAPE = (768, 50)
SPECIAL_KS = [0, 7, 8, 131, 255, 300, 346, 511, 533, 677, 767]
MIRROR_KS = [3, 9, 250, 260, 513, 766]
DENORM_EXP = {1: -24, 2: -133, 3: -149}
DENORM_A = {1: [1, 2, 513, 1023], 2: [1, 2, 65, 127], 3: [1, 2, (1 << 22) + 1, (1 << 23) - 1]}


def specials(ft):
    """The special values as fp64 (every one a number of the type)."""
    big = float(torch.finfo(TORCH_FLOAT[ft]).max)
    d = [a * 2.0 ** DENORM_EXP[ft] for a in DENORM_A[ft]]
    return d + [-v for v in d] + [0.0, -0.0, big, -big]


def special_table(ft):
    """-> W [50, 768] of the type on the CPU."""
    rw, R = SPECIAL_SHAPE
    rng = np.random.default_rng([ft, 77])
    W = _signed(rng, 7, [R, rw]).astype(np.float64)
    vals = specials(ft)
    for j, k in enumerate(SPECIAL_KS):
        W[:, k] = [vals[(r + j) % len(vals)] for r in range(R)]
    for k in MIRROR_KS:
        W[:, k] = [1024.0 if r % 2 == 0 else 1.0 for r in range(R)]
    Wt = torch.from_numpy(W).to(TORCH_FLOAT[ft])
    assert torch.equal(Wt.double(), torch.from_numpy(W)) and bool(torch.isfinite(Wt).all())
    assert np.array_equal(np.signbit(Wt.double().numpy()), np.signbit(W))  # -0.0 survives
    return Wt


def unit_acts(ft, ks, rw, scale=None):
    """x[m] = scale[m] * e_ks[m] (scale 1 by default), fp64 -> the type, exact."""
    x = torch.zeros([len(ks), rw], dtype=torch.float64)
    x[range(len(ks)), ks] = torch.tensor([1.0] * len(ks) if scale is None else scale, dtype=torch.float64)
    xt = x.to(TORCH_FLOAT[ft])
    assert torch.equal(xt.double(), x)
    return xt


def mirror_scales(ft):
    """A denormal of the type for every column of MIRROR_KS, both signs."""
    d = [a * 2.0 ** DENORM_EXP[ft] for a in DENORM_A[ft]]
    return [(d[j % len(d)] * (-1 if j % 2 else 1)) for j in range(len(MIRROR_KS))]


def int_words(t):
    """A float tensor's bits as signed integers of its width."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])

