"""Inputs and the model of the fused sparse reduce tests
(tests/test_gpu_sparse_reduce.py on the GPU, tests/test_sparse_reduce_inputs.py
on the CPU).

The model is torch on the CPU, never the code under test: an fp32 running sum
that starts as init.float() (or as the decoded first element without an init)
and takes the sources one after the other by the sparse accumulate's rule
(tests/sparse_accumulate_cases.expected: the add where the source's word is
nonzero bitwise, the old bits everywhere else), then one rounding to the out
dtype.  Words travel as numpy unsigned integers, inits and results as torch
CPU tensors.  ft: 1 fp16, 2 bf16, 3 fp32.  Seeded, numpy and torch only."""
import numpy as np
import torch

from tests import accumulate_cases as A
from tests import reduce_cases as R
from tests import sparse_accumulate_cases as S
from tests.util import NP_WORD, SPARSE_FILLS, SPARSE_TAILS, _sparse_fill

FTS = R.FTS
FORMS = R.FORMS
K_SWEEP = R.K_SWEEP
form_dtype = R.form_dtype


def acc_mode(ft):
    """The accumulate mode whose accumulator is fp32: 2 for fp16 / bf16
    archives, 1 (the archives' own type) for fp32."""
    return 2 if ft in (1, 2) else 1


def model(words, ft, init=None, out_dtype=torch.float32, order=None, add_zeros=False, from_zero=False):
    """The reduce as the feature defines it.  words: the K sources' words in
    source order.  The three wrong kernels: order, a permutation of the
    sources; add_zeros, an IEEE add of +0.0 where a bit is clear instead of
    the skip; from_zero, a start from +0.0 instead of the first element when
    there is no init."""
    words = [words[i] for i in order] if order is not None else list(words)
    if init is not None:
        a = init.float()
    elif from_zero:
        a = torch.zeros(words[0].size, dtype=torch.float32)
    else:
        a, words = A.words_to_float(words[0], ft).float(), words[1:]
    for w in words:
        a = a + A.words_to_float(w, ft).float() if add_zeros else S.expected(a, w, ft, acc_mode(ft))
    return a.to(out_dtype)


def sources(ft, K, n, frac_zero, seed=70):
    """K word vectors of n words: reduce_cases.sources' N(0,1)-like values,
    frac_zero of each source's words +0.0 at positions drawn independently per
    source."""
    out = []
    for k, x in enumerate(R.sources(ft, K, n, seed=seed)):
        w = A.float_to_words(x, ft)
        w[np.random.default_rng(7000 + seed + k).random(n) < frac_zero] = 0
        out.append(w)
    return out


def init_fp32(ft, n, seed=0):
    """An fp32 init with every fifth word -0.0 (sparse_accumulate_cases.case_acc)."""
    return S.case_acc(ft, acc_mode(ft), n, seed=seed)


def companion(ft, w, k, tail):
    """Another element of w's size for source k of a sweep member: another
    fill (the fills cycle with n + k) and the tail SPARSE_TAILS[(tail + k) % 4],
    forced as util.sparse_edge_elements forces it."""
    n = w.size
    c = _sparse_fill(ft, n, SPARSE_FILLS[(n + k) % 3], seed=13 * n + 100 * k + ft)
    t2, t1 = SPARSE_TAILS[(tail + k) % 4]
    one = NP_WORD[ft](1)
    if n >= 2:
        c[n - 2] = (c[n - 2] | one) if t2 else 0
    if n >= 1:
        c[n - 1] = (c[n - 1] | one) if t1 else 0
    return c


def sweep_members(cases, ft, K=3):
    """[(name, [x_1 .. x_K])] for [(name, words)] of the sparse edge sweep:
    x_1 the sweep's element, the others companions of its size with other
    fills and tails, so that one position sees every mix of set and clear bits
    and the n-2 quirk differs between the sources of one member."""
    out = []
    for i, (name, w) in enumerate(cases):
        out.append((name, [w] + [companion(ft, w, k, i) for k in range(1, K)]))
    return out


def differing_fraction(a, b):
    return R.differing_fraction(a, b)
