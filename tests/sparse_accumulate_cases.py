"""Inputs and the expected result of the sparse decode-and-accumulate tests
(tests/test_gpu_sparse_accumulate.py on the GPU, tests/test_sparse_accumulate_inputs.py
and tests/test_dist_sparse_reduce.py on the CPU).

The arithmetic is the dense feature's model (tests/accumulate_cases.py: torch
on the CPU), applied only where the element's word is nonzero BITWISE: -0.0
in the element is a nonzero word and is added, +0.0 is skipped and its
accumulator word keeps its bits.  Words travel as numpy unsigned integers,
accumulators as torch CPU tensors.  Seeded, numpy and torch only."""
import numpy as np
import torch

from tests.accumulate_cases import (MODE_IDS, MODES, TORCH_FLOAT, acc_dtype, bits, fixed_accumulators,  # noqa: F401
                                    float_to_words, mismatch_report, model, random_acc, same_bits, specials,
                                    words_to_float)
from tests.util import NP_WORD, sparse_edge_elements

# a signalling NaN with an odd payload per accumulator type: an IEEE add of
# +0.0 would quiet it, the skipped position must not
SNAN_BITS = {torch.float16: 0x7d55, torch.bfloat16: 0x7fa5, torch.float32: 0x7fa55555,
             torch.float64: 0x7ff5555555555555}


def expected(acc, words, ft, mode):
    """acc (torch CPU, the accumulator's dtype) after the element `words` was
    added: the model at the nonzero words, the old bits everywhere else."""
    want = acc.clone()
    nz = torch.from_numpy(np.ascontiguousarray(words) != 0)
    x = words_to_float(words, ft)
    want[nz] = model(acc[nz], x[nz], mode)
    return want


def touched(words):
    """The positions an accumulate of `words` may write."""
    return torch.from_numpy(np.ascontiguousarray(words) != 0)


def check(got, want, init, touch):
    """None, or what is wrong: `got` must equal `want` bitwise wherever `want`
    is not a NaN and be a NaN where it is, and must hold init's very bits
    (a NaN's payload included) wherever touch is False."""
    if not same_bits(got, want):
        return mismatch_report(got, want)
    keep = ~touch
    if not torch.equal(bits(got)[keep], bits(init)[keep]):
        bad = (keep & (bits(got) != bits(init))).nonzero().view(-1)
        return f"{bad.numel()} untouched words changed, first at {bad[:5].tolist()}"
    return None


def case_acc(ft, mode, n, seed=0):
    """An accumulator for an n-word element: random finite values, every fifth
    one -0.0 (under zero and under nonzero words alike, whatever the fill)."""
    a = random_acc(ft, mode, n, seed=seed)
    a[::5] = -0.0
    return a


_EDGE = {}


def edge_elements(ft):
    """[(group, name, words)] of util.sparse_edge_elements(ft), generated once."""
    if ft not in _EDGE:
        _EDGE[ft] = sparse_edge_elements(ft)
    return _EDGE[ft]


def small_cases(ft):
    """[(name, words)]: every "small" element."""
    return [(name, w) for g, name, w in edge_elements(ft) if g == "small"]


def large_cases(ft):
    """[(name, words)]: the five sizes 262,144 - 2 .. + 2, one tail each, the
    four tails (x[n-2], x[n-1] zero or not) all among them."""
    out = {}
    for g, name, w in edge_elements(ft):
        if g == "large":
            out.setdefault(w.size, []).append((name, w))
    picked = [v[k % 4] for k, (_, v) in enumerate(sorted(out.items()))]
    assert len(picked) == 5
    return picked


def patterns16_dense(ft, mode):
    """(words, acc): every nonzero 16-bit pattern against each of the 16 fixed
    accumulator values; no zero word."""
    pat = np.arange(1, 1 << 16, dtype=np.uint32).astype(np.uint16)
    fixed = fixed_accumulators(ft, mode)
    return np.tile(pat, 16), torch.cat([fixed[i].repeat(pat.size) for i in range(16)])


def acc_specials(ft, mode):
    """The fixed accumulator values (-0.0, +-inf, a NaN and denormals among
    them) and a signalling NaN with a payload."""
    dt = acc_dtype(ft, mode)
    fixed = fixed_accumulators(ft, mode)
    it = bits(fixed).dtype
    mask = (1 << (8 * dt.itemsize)) - 1
    p = SNAN_BITS[dt]
    snan = torch.tensor([p - (mask + 1) if p > mask >> 1 else p], dtype=it).view(dt)
    return torch.cat([fixed, snan])


def patterns16_interleaved(ft, mode):
    """(words, acc): the same patterns, a zero word after each, over every
    value of acc_specials(); the zero positions must keep their bits."""
    pat = np.arange(1, 1 << 16, dtype=np.uint32).astype(np.uint16)
    one = np.zeros(2 * pat.size, dtype=np.uint16)
    one[0::2] = pat
    sp = acc_specials(ft, mode)
    return np.tile(one, sp.numel()), torch.cat([sp[i].repeat(one.size) for i in range(sp.numel())])


def cross_specials_interleaved(ft):
    """(words, acc) for fp32 / fp64: specials(ft) crossed with itself, a zero
    word after each pair over the same accumulator value (and over a
    signalling NaN at the end)."""
    assert ft in (3, 4)
    s = specials(ft)
    x = float_to_words(s.repeat_interleave(s.numel()), ft)
    a = s.repeat(s.numel())
    words = np.zeros(2 * x.size + 8, dtype=NP_WORD[ft])
    words[0:2 * x.size:2] = x
    acc = torch.cat([a.repeat_interleave(2), acc_specials(ft, 1)[-1:].repeat(8)])
    return words, acc
