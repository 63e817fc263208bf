"""CPU checks of tests/matmul_cases.py: the reference of the exact-sum GPU tests
(tests/test_gpu_matmul_exact.py) meets, on its own, the bitwise equality those
tests demand of the kernels."""
import numpy as np
import pytest
import torch

from tests import matmul_cases as MC
from tests.util import FT_NAME, TORCH_FLOAT

# every (rowWords, R) the GPU tests build an exact table at, and the types
SHAPES = sorted(set(MC.WORD_SHAPES + MC.PERIOD_SHAPES + [(rw, R) for rw, R, _ in MC.PREFIXES + MC.CAP_SHAPES]))
CASES = [(rw, R, ft, const) for rw, R in SHAPES for ft in (1, 2, 3) for const in (False, True)]
IDS = [f"{rw}x{R}-{FT_NAME[ft]}-{'const' if const else 'wide'}" for rw, R, ft, const in CASES]
M = 64


def make(rw, R, ft, const):
    a, e, W = MC.exact_table(ft, rw, R, 0, *((0, 0) if const else (None, None)))
    b, x = MC.exact_acts(ft, M, rw, e)
    return a, e, W, b, x


@pytest.mark.parametrize("rw,R,ft,const", CASES, ids=IDS)
def test_the_reference_is_exact(rw, R, ft, const):
    a, e, W, b, x = make(rw, R, ft, const)
    # the 2^24 condition, next to the shape
    assert R * rw <= MC.LARGEST_TABLE and (a != 0).all() and (b != 0).all()
    assert int(np.abs(a).max()) * int(np.abs(b).max()) * rw < 1 << 24
    assert np.abs(a).max() <= MC.A_MAX and np.abs(b).max() <= MC.b_max(rw) <= MC.B_MAX
    # W and x are numbers of the type: nothing was rounded
    assert W.dtype == x.dtype == TORCH_FLOAT[ft]
    assert np.array_equal(W.double().numpy(), np.ldexp(a.astype(np.float64), e[None, :]))
    assert np.array_equal(x.double().numpy(), np.ldexp(b.astype(np.float64), -e[None, :]))
    # the fp64 product is the int64 product
    want = b @ a.T
    assert np.array_equal((x.double() @ W.double().T).numpy(), want.astype(np.float64))
    assert torch.equal(MC.exact_product(b, a).double(), torch.from_numpy(want.astype(np.float64)))
    # ... and so is an fp32 sum over 256-word segments taken in a shuffled order
    order = np.random.default_rng(rw + R).permutation(rw // 256)
    xf, Wf = x.float(), W.float()
    acc = torch.zeros([M, R], dtype=torch.float32)
    for s in order:
        acc = acc + xf[:, 256 * s:256 * s + 256] @ Wf[:, 256 * s:256 * s + 256].T
    assert torch.equal(acc, MC.exact_product(b, a))


@pytest.mark.parametrize("ft", [1, 2, 3], ids=["fp16", "bf16", "fp32"])
def test_the_exponents_and_the_constant_table(ft):
    a, e, W = MC.exact_table(ft, 8192, 9)
    lo, hi = MC.E_RANGE[ft]
    assert e.min() == lo and e.max() == hi
    syms = np.unique(MC.symbols_of(MC.words_of(W, ft), ft))
    assert len(syms) >= {1: 80, 2: 200, 3: 200}[ft]  # (bf16: 207 distinct exponent bytes)
    a, e, W = MC.exact_table(ft, 8192, 9, 0, 0, 0)
    assert not e.any() and set(np.unique(a)) == ({1} if ft == 1 else {-1, 1})
    assert len(np.unique(MC.symbols_of(MC.words_of(W, ft), ft))) == 1  # one symbol of probability 1


def test_the_experts_of_a_grouped_call_share_their_exponents():
    t0, t1 = MC.exact_table(2, 768, 50, 0), MC.exact_table(2, 768, 50, 1)
    assert np.array_equal(t0[1], t1[1]) and not np.array_equal(t0[0], t1[0])


@pytest.mark.parametrize("ft", [1, 2, 3], ids=["fp16", "bf16", "fp32"])
def test_special_tables(ft):
    W = MC.special_table(ft)
    rw, R = MC.SPECIAL_SHAPE
    tiny = float(torch.finfo(TORCH_FLOAT[ft]).tiny)
    Wd = W.double()
    for j, k in enumerate(MC.SPECIAL_KS):
        col = Wd[:, k]
        den = (col != 0) & (col.abs() < tiny)
        assert den.any() and (col == 0).any() and (col.abs() == torch.finfo(TORCH_FLOAT[ft]).max).any(), k
        assert (col[den] > 0).any() and (col[den] < 0).any()
    # the columns lie in different lanes, chunk words and segments
    ks = MC.SPECIAL_KS + MC.MIRROR_KS
    assert len(set(ks)) == len(ks) and {k // 256 for k in MC.SPECIAL_KS} == {k // 256 for k in MC.MIRROR_KS} == {0, 1, 2}
    assert len({k % 256 // 8 for k in MC.SPECIAL_KS}) >= 8 and {0, 7} <= {k % 8 for k in MC.SPECIAL_KS}
    # a unit row picks the column, exactly; a denormal activation's products are fp32 numbers
    x = MC.unit_acts(ft, MC.SPECIAL_KS, rw)
    assert torch.equal(x.double() @ Wd.T, Wd[:, MC.SPECIAL_KS].T)
    xm = MC.unit_acts(ft, MC.MIRROR_KS, rw, MC.mirror_scales(ft))
    prod = xm.double() @ Wd.T
    assert torch.equal(prod.float().double(), prod) and bool((prod != 0).all())
    assert bool((xm.double().abs().max(1).values < tiny).all())
