"""Inputs and the model of the decode-and-accumulate tests
(tests/test_gpu_accumulate.py on the GPU, tests/test_accumulate_inputs.py and
tests/test_dist_reduce.py on the CPU).

The model is torch on the CPU, never the code under test.  ft: 1 fp16,
2 bf16, 3 fp32, 4 fp64; mode 1: the accumulator has the archive's type,
mode 2: an fp32 accumulator of an fp16 / bf16 archive.  Words travel as
numpy unsigned integers (the archives' view), accumulators as torch CPU
tensors of the float dtype.  Seeded, numpy and torch only."""
import numpy as np
import torch

from tests.util import FT_IDS, NP_SIGNED, NP_WORD, TORCH_FLOAT

TORCH_INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32,
             torch.float64: torch.int64}
# (float type, mode): the six kernel instances
MODES = ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2))
MODE_IDS = [f"{FT_IDS[ft]}-acc{m}" for ft, m in MODES]

# words per member of the size-edge batch: around the 8-word chunk, the
# 256-word segment, the 4096-word block, the 32768-word workgroup chunk (8
# blocks; 32769 starts the next one), and two odd sizes of several blocks
SIZES = (0, 1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 12345, 32767, 32768, 32769, 70001)


def acc_dtype(ft, mode):
    return torch.float32 if mode == 2 else TORCH_FLOAT[ft]


def words_to_float(words, ft):
    """numpy words -> a torch CPU tensor of the float type (same bits)."""
    return torch.from_numpy(np.ascontiguousarray(words).view(NP_SIGNED[ft]).copy()).view(TORCH_FLOAT[ft])


def float_to_words(t, ft):
    return t.contiguous().view(TORCH_INT[TORCH_FLOAT[ft]]).numpy().view(NP_WORD[ft]).copy()


def model(acc, x, mode):
    """acc + x as the feature defines it: mode 1 the correctly rounded sum in
    the words' type (for 16-bit types: widen both to fp32, add, round once to
    nearest even, which is that sum: 24 >= 2 * 11 + 2), mode 2 acc (fp32) +
    float(x)."""
    if mode == 2:
        assert acc.dtype == torch.float32 and x.dtype in (torch.float16, torch.bfloat16)
        return acc + x.float()
    assert acc.dtype == x.dtype
    if x.dtype in (torch.float16, torch.bfloat16):
        return (acc.float() + x.float()).to(x.dtype)
    return acc + x


def bits(t):
    return t.contiguous().view(TORCH_INT[t.dtype])


def same_bits(got, want):
    """Bitwise equal wherever `want` is not a NaN; a NaN where it is."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = torch.isnan(want)
    return bool(torch.isnan(got[nan]).all()) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def mismatch_report(got, want, limit=5):
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), bits(got) != bits(want)).nonzero().view(-1)
    return f"{bad.numel()} words differ, first at {bad[:limit].tolist()}: got " \
           f"{[hex(int(v)) for v in bits(got)[bad[:limit]]]} want {[hex(int(v)) for v in bits(want)[bad[:limit]]]}"


def _from_bits(patterns, dtype):
    it = TORCH_INT[dtype]
    mask = {torch.int16: 0xffff, torch.int32: 0xffffffff, torch.int64: (1 << 64) - 1}[it]
    half = (mask + 1) >> 1
    signed = [(p & mask) - (mask + 1) if (p & mask) >= half else (p & mask) for p in patterns]
    return torch.tensor(signed, dtype=it).view(dtype)


# Special values per float type as bit patterns: 1.0, the next value above it
# (odd significand), both negated; +-0; +-max; the smallest and the largest
# denormal; the smallest normal; +-inf; a NaN; half an ulp of 1.0 (1.0 + it is
# a tie that rounds down to the even 1.0, (1.0 + ulp) + it one that rounds up);
# and max / 2 rounded up (max + it overflows to inf).
SPECIAL_BITS = {
    1: [0x3c00, 0x3c01, 0xbc00, 0xbc01, 0x0000, 0x8000, 0x7bff, 0xfbff, 0x0001, 0x03ff, 0x0400, 0x7c00, 0xfc00,
        0x7e00, 0x1000, 0x7800],
    2: [0x3f80, 0x3f81, 0xbf80, 0xbf81, 0x0000, 0x8000, 0x7f7f, 0xff7f, 0x0001, 0x007f, 0x0080, 0x7f80, 0xff80,
        0x7fc0, 0x3b80, 0x7f00],
    3: [0x3f800000, 0x3f800001, 0xbf800000, 0xbf800001, 0x00000000, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x00000001,
        0x007fffff, 0x00800000, 0x7f800000, 0xff800000, 0x7fc00000, 0x33800000, 0x7f000000],
    4: [0x3ff0000000000000, 0x3ff0000000000001, 0xbff0000000000000, 0xbff0000000000001, 0x0000000000000000,
        0x8000000000000000, 0x7fefffffffffffff, 0xffefffffffffffff, 0x0000000000000001, 0x000fffffffffffff,
        0x0010000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0x3ca0000000000000,
        0x7fe0000000000000],
}


def specials(ft):
    """The 16 special values of the type (SPECIAL_BITS)."""
    return _from_bits(SPECIAL_BITS[ft], TORCH_FLOAT[ft])


def fixed_accumulators(ft, mode):
    """The 16 fixed accumulator values every 16-bit pattern is added to.
    Mode 1: the type's specials.  Mode 2: the fp32 specials; both 16-bit
    types hold 2^-24, half an ulp of the fp32 1.0 (fp16's smallest denormal),
    so the fp32 ties are met, and bf16's large values overflow fp32's."""
    return specials(ft if mode == 1 else 3)


def all_patterns(ft):
    """Every 16-bit pattern as a word of the type, in order."""
    assert ft in (1, 2)
    return words_to_float(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16), ft)


def arithmetic16(ft, mode, seed=0):
    """(x words [17 * 65536] numpy, acc [17 * 65536] torch): every 16-bit
    pattern against each fixed accumulator value, then against one random
    finite accumulator vector."""
    pat = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    fixed = fixed_accumulators(ft, mode)
    accs = [fixed[i].repeat(1 << 16) for i in range(16)]
    accs.append(random_acc(ft, mode, 1 << 16, seed=seed + 17))
    return np.tile(pat, 17), torch.cat(accs)


def random_acc(ft, mode, n, seed=0):
    """Random finite accumulator values over a wide exponent range, both
    signs, in the accumulator's dtype."""
    g = torch.Generator().manual_seed(1000 + seed)
    v = torch.randn(n, generator=g, dtype=torch.float64) * torch.exp2(
        torch.randint(-12, 12, (n,), generator=g).double())
    return v.to(acc_dtype(ft, mode))


def cross_specials(ft, n_random=100000, seed=3):
    """(x, acc) float tensors for fp32 / fp64: the special table crossed with
    itself, then n_random random pairs of nearby magnitude (so that the sums
    round and cancel) with both signs."""
    assert ft in (3, 4)
    s = specials(ft)
    x = s.repeat_interleave(s.numel())
    a = s.repeat(s.numel())
    g = torch.Generator().manual_seed(seed)
    dt = TORCH_FLOAT[ft]
    rx = (torch.randn(n_random, generator=g, dtype=torch.float64)
          * torch.exp2(torch.randint(-6, 6, (n_random,), generator=g).double())).to(dt)
    ra = (torch.randn(n_random, generator=g, dtype=torch.float64)
          * torch.exp2(torch.randint(-6, 6, (n_random,), generator=g).double())).to(dt)
    # some exact cancellations and near-cancellations among the random pairs
    ra[::97] = -rx[::97]
    return torch.cat([x, rx]), torch.cat([a, ra])


def member_words(ft, n, seed=0):
    """The words of a size-edge member: N(0, 1) values of the type."""
    from tests.util import float_words

    return float_words(ft, n, seed=seed)
