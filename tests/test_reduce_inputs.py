"""The inputs of the fused-reduce tests can tell a wrong kernel from a right
one (tests/reduce_cases.py; CPU: numpy, torch and the oracle only).  A kernel
that adds in another order, rounds the running sum to 16 bits at every add, or
starts from +0.0 must differ from the model on a large share of the words the
GPU tests compare."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import accumulate_cases as A
from tests import reduce_cases as R

K, N = 7, 70001


@pytest.fixture(scope="module", params=R.FTS, ids=[A.FT_IDS[ft] for ft in R.FTS])
def xs(request):
    return request.param, R.sources(request.param, K, N)


def test_sources_are_finite_and_survive_the_oracle(xs):
    ft, v = xs
    assert all(bool(torch.isfinite(x).all()) for x in v)
    w = A.float_to_words(v[0][:4097], ft)
    st, back = O.float_decompress(O.float_compress(w, ft, 10), ft, 10)
    assert st == 0 and np.array_equal(back, w)


def test_order_shows_on_fp32_output(xs):
    """Ascending against reversed source order, fp32 output."""
    ft, v = xs
    want = R.model(v)
    assert not bool(torch.isnan(want).any())
    frac = R.differing_fraction(want, R.model(v, order=list(range(K))[::-1]))
    print(A.FT_IDS[ft], "order", frac)
    assert frac >= 0.10


def test_order_barely_shows_after_rounding_to_16_bits():
    v = R.sources(2, K, N)
    frac = R.differing_fraction(R.model(v, out_dtype=torch.bfloat16),
                                R.model(v, out_dtype=torch.bfloat16, order=list(range(K))[::-1]))
    assert frac < 0.01


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_per_add_rounding_shows(ft):
    v = R.sources(ft, K, N)
    dt = A.TORCH_FLOAT[ft]
    frac = R.differing_fraction(R.model(v, out_dtype=dt), R.model(v, out_dtype=dt, per_add=dt))
    print(A.FT_IDS[ft], "per-add", frac)
    assert frac >= 0.10


def test_start_from_zero_shows_on_negative_zero(xs):
    ft, v = xs
    x = v[0].clone()
    x[::5] = -0.0
    got, wrong = R.model([x]), R.model_from_zero([x])
    assert torch.equal(A.bits(got), A.bits(x.float()))
    differ = A.bits(got) != A.bits(wrong)
    assert bool(differ[::5].all()) and int(differ.sum()) == x[::5].numel()


def test_order_probe_separates_the_orders():
    init, xs3 = R.order_probe(2)
    want = R.model(xs3, init=init)
    # init first: 1 + 2^-24 ties to 1 twice, then - 1 = 0; any order the probe
    # holds that adds -1.0 earlier keeps a small term
    assert want.tolist()[0] == 0.0 and len(set(want.tolist())) >= 2
    rev = R.model(xs3[::-1], init=init)
    assert not torch.equal(A.bits(want), A.bits(rev))


def test_split_is_invisible_in_the_model():
    v = R.sources(2, 9, 4097, seed=90)
    part = R.model(v[:4])
    assert torch.equal(A.bits(R.model(v[4:], init=part)), A.bits(R.model(v)))
