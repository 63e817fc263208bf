"""The inputs of the fused sparse reduce tests tell a wrong kernel from a right
one (tests/sparse_reduce_cases.py), on fp32 output.  CPU only:
the model against three wrong models, none of the feature's kernels.

K = 7, n = 70,001, an fp32 init with every fifth word -0.0, N(0,1)-like
nonzeros, independent random zero positions per source.  A reversed source
order shows at 50 % zeros (at 90 % most positions hold at most one set bit);
an add of +0.0 for a clear bit shows at 90 % zeros (it needs a running sum
that is still -0.0, i.e. no set bit before)."""
import numpy as np
import pytest
import torch

from tests import accumulate_cases as A
from tests import sparse_reduce_cases as SR

K, N = 7, 70001


@pytest.fixture(scope="module")
def inputs():
    made = {}

    def get(ft, frac):
        if (ft, frac) not in made:
            made[ft, frac] = (SR.sources(ft, K, N, frac), SR.init_fp32(ft, N, seed=1))
        return made[ft, frac]

    return get


@pytest.mark.parametrize("ft", SR.FTS, ids=[A.FT_IDS[ft] for ft in SR.FTS])
def test_a_reversed_source_order_shows(inputs, ft):
    xs, init = inputs(ft, 0.5)
    right = SR.model(xs, ft, init=init)
    share = SR.differing_fraction(right, SR.model(xs, ft, init=init, order=list(range(K))[::-1]))
    print(f"reversed order, {A.FT_IDS[ft]}, 50 % zeros: {100 * share:.1f} % of the words differ")
    assert share >= 0.01


@pytest.mark.parametrize("ft", SR.FTS, ids=[A.FT_IDS[ft] for ft in SR.FTS])
def test_an_added_zero_shows(inputs, ft):
    xs, init = inputs(ft, 0.9)
    right = SR.model(xs, ft, init=init)
    share = SR.differing_fraction(right, SR.model(xs, ft, init=init, add_zeros=True))
    print(f"+0.0 added for a clear bit, {A.FT_IDS[ft]}, 90 % zeros: {100 * share:.1f} % of the words differ")
    assert share >= 0.01
    # and every difference is a -0.0 that the wrong kernel turned into +0.0
    wrong = SR.model(xs, ft, init=init, add_zeros=True)
    bad = A.bits(right) != A.bits(wrong)
    assert bool((A.bits(right)[bad] == A.bits(torch.tensor([-0.0]))).all()) and bool((A.bits(wrong)[bad] == 0).all())


@pytest.mark.parametrize("ft", SR.FTS, ids=[A.FT_IDS[ft] for ft in SR.FTS])
def test_a_start_from_zero_shows(inputs, ft):
    """Without an init the sum starts as x_1, not as +0.0: a start from +0.0
    changes every word where x_1 holds -0.0 and no later bit is set, and (on
    this input) nothing else."""
    xs = [w.copy() for w in inputs(ft, 0.9)[0]]
    neg0 = A.float_to_words(torch.tensor([-0.0], dtype=A.TORCH_FLOAT[ft]), ft)[0]
    xs[0][3::50] = neg0
    right = SR.model(xs, ft)
    wrong = SR.model(xs, ft, from_zero=True)
    later = np.zeros(N, dtype=bool)
    for w in xs[1:]:
        later |= w != 0
    must = torch.from_numpy((xs[0] == neg0) & ~later)
    assert int(must.sum()) > 100
    differ = A.bits(right) != A.bits(wrong)
    assert bool(differ[must].all())
    assert bool((A.bits(right)[must] == A.bits(torch.tensor([-0.0]))).all())
    print(f"start from +0.0, {A.FT_IDS[ft]}: {int(differ.sum())} words differ, {int(must.sum())} of them must")
