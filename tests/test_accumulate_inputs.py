"""The input sets of the decode-and-accumulate tests hold what they claim
(tests/accumulate_cases.py): ties in both directions, overflow, exact
cancellation, -0 + -0, denormal inputs and results, inf - inf and NaN inputs.
Runs the CPU model and numpy only, none of the feature's code."""
import numpy as np
import pytest
import torch

from tests import accumulate_cases as A


def f(v, dtype):
    return torch.tensor([v], dtype=torch.float64).to(dtype)


def test_the_six_modes_and_the_size_edges():
    assert A.MODES == ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2))
    assert A.SIZES == (0, 1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 12345, 32767, 32768, 32769, 70001)
    assert A.acc_dtype(2, 2) == torch.float32 and A.acc_dtype(2, 1) == torch.bfloat16


def test_model_ties_in_bf16_and_fp16():
    bf, h = torch.bfloat16, torch.float16
    # bf16: ulp(1.0) = 2^-7; 1.0 + 2^-8 is a tie -> even 1.0, 1.0078125 + 2^-8 -> 1.015625
    assert float(A.model(f(1.0, bf), f(2.0 ** -8, bf), 1)) == 1.0
    assert float(A.model(f(1.0078125, bf), f(2.0 ** -8, bf), 1)) == 1.015625
    # fp16: ulp(1.0) = 2^-10
    assert float(A.model(f(1.0, h), f(2.0 ** -11, h), 1)) == 1.0
    assert float(A.model(f(1.0 + 2.0 ** -10, h), f(2.0 ** -11, h), 1)) == 1.0 + 2.0 ** -9
    # mode 2: the sum stays in fp32
    assert float(A.model(f(1.0, torch.float32), f(2.0 ** -8, bf), 2)) == 1.0 + 2.0 ** -8


def test_special_tables():
    for ft in (1, 2, 3, 4):
        s = A.specials(ft).double()
        assert s.numel() == 16 and len(set(A.SPECIAL_BITS[ft])) == 16
        dt = A.TORCH_FLOAT[ft]
        fi = torch.finfo(dt)
        assert float(s[0]) == 1.0 and float(s[1]) == 1.0 + fi.eps and float(s[2]) == -1.0
        assert float(s[4]) == 0.0 and not torch.signbit(s[4]) and float(s[5]) == 0.0 and torch.signbit(s[5])
        assert float(s[6]) == fi.max and float(s[7]) == -fi.max
        assert 0 < float(s[8]) < float(s[9]) < float(s[10]) == fi.tiny  # two denormals, the smallest normal
        assert float(s[11]) == float("inf") and float(s[12]) == -float("inf") and torch.isnan(s[13])
        assert float(s[14]) == fi.eps / 2
        assert torch.isinf(A.model(A.specials(ft)[6:7], A.specials(ft)[15:16], 1))  # max + max / 2 overflows


def _classes(x, acc, mode):
    """What the pairs (acc, x) exercise, by the model."""
    r = A.model(acc, x, mode)
    exact = acc.double() + x.double()  # exact for 16-bit and fp32 operands, finite or not
    fin = torch.isfinite(acc) & torch.isfinite(x)
    rd = r.double()
    inexact = fin & torch.isfinite(r) & (rd != exact)
    lo = torch.finfo(r.dtype).tiny
    return {
        "rounded down": bool((inexact & (rd.abs() < exact.abs())).any()),
        "rounded up": bool((inexact & (rd.abs() > exact.abs())).any()),
        "overflow to inf": bool((fin & torch.isinf(r)).any()),
        "cancellation to +0": bool((fin & (x != 0) & (r == 0) & ~torch.signbit(r)).any()),
        "-0 + -0": bool(((acc == 0) & torch.signbit(acc) & (x == 0) & torch.signbit(x) & torch.signbit(r)).any()),
        "denormal input": bool((fin & (x != 0) & (x.abs().double() < torch.finfo(x.dtype).tiny)).any()),
        "denormal result": bool((fin & (r != 0) & (r.abs() < lo)).any()),
        "inf - inf": bool((torch.isinf(acc) & torch.isinf(x) & torch.isnan(r)).any()),
        "NaN input": bool((torch.isnan(x) | torch.isnan(acc)).any()),
    }, r


def _ties(x, acc, mode):
    """Ties to even in both directions among the finite pairs: the exact sum
    lies midway between two neighbours of the result's type."""
    r = A.model(acc, x, mode)
    exact = acc.double() + x.double()
    fin = torch.isfinite(exact) & torch.isfinite(r) & (r.double() != exact)
    rb = A.bits(r)
    other = torch.where(r.double().abs() < exact.abs(), rb + 1, rb - 1).view(r.dtype)  # the neighbour across the sum
    fin &= torch.isfinite(other)
    tie = fin & ((r.double() - exact).abs() == (other.double() - exact).abs())
    assert bool(((rb[tie] & 1) == 0).all()), "a tie went to the odd neighbour"
    down = bool((tie & (r.double().abs() < exact.abs())).any())
    up = bool((tie & (r.double().abs() > exact.abs())).any())
    return down, up


@pytest.mark.parametrize("ft,mode", [(1, 1), (2, 1), (1, 2), (2, 2)], ids=["fp16-acc1", "bf16-acc1", "fp16-acc2",
                                                                          "bf16-acc2"])
def test_arithmetic16_set(ft, mode):
    xw, acc = A.arithmetic16(ft, mode)
    assert xw.size == 17 * 65536 == acc.numel() and acc.dtype == A.acc_dtype(ft, mode)
    # every pattern against every fixed value, then the random vector
    assert np.array_equal(xw[:65536], np.arange(65536, dtype=np.uint16)) and np.array_equal(xw[65536:131072], xw[:65536])
    fixed = A.fixed_accumulators(ft, mode)
    for i in range(16):
        assert A.same_bits(acc[i * 65536:(i + 1) * 65536], fixed[i].repeat(65536))
    assert bool(torch.isfinite(acc[16 * 65536:]).all())
    x = A.words_to_float(xw, ft)
    got, _ = _classes(x, acc, mode)
    want = set(got)
    if (ft, mode) == (1, 2):
        want.discard("overflow to inf")  # no finite fp16 value moves fp32's max
    assert {k for k in want if got[k]} == want, got
    assert _ties(x, acc, mode) == (True, True)


@pytest.mark.parametrize("ft", [3, 4], ids=["fp32", "fp64"])
def test_cross_specials_set(ft):
    x, acc = A.cross_specials(ft)
    assert x.numel() == 256 + 100000 == acc.numel()
    s = A.specials(ft)
    pairs = {(int(a), int(b)) for a, b in zip(A.bits(acc[:256]).tolist(), A.bits(x[:256]).tolist())}
    assert len(pairs) == 256 and pairs == {(int(a), int(b)) for a in A.bits(s).tolist() for b in A.bits(s).tolist()}
    r = A.model(acc, x, 1)
    one, nxt, half = s[0], s[1], s[14]
    # the ties at 1.0, both directions, by the model
    assert float(A.model(one, half, 1)) == 1.0
    assert float(A.model(nxt, half, 1)) == 1.0 + 2 * torch.finfo(s.dtype).eps
    fin = torch.isfinite(acc) & torch.isfinite(x)
    assert bool((fin & torch.isinf(r)).any())
    assert bool((fin & (x != 0) & (r == 0) & ~torch.signbit(r)).any())
    assert bool(((acc == 0) & torch.signbit(acc) & (x == 0) & torch.signbit(x) & torch.signbit(r)).any())
    tiny = torch.finfo(s.dtype).tiny
    assert bool((fin & (x != 0) & (x.abs() < tiny)).any()) and bool((fin & (r != 0) & (r.abs() < tiny)).any())
    assert bool((torch.isinf(acc) & torch.isinf(x) & torch.isnan(r)).any())
    assert bool(torch.isnan(x).any()) and bool(torch.isnan(acc).any())
    # the random pairs round: most sums are inexact in the type
    if ft == 3:
        exact = acc[256:].double() + x[256:].double()
        assert float((r[256:].double() != exact).float().mean()) > 0.25


def test_word_views_round_trip():
    for ft in (1, 2, 3, 4):
        w = A.member_words(ft, 257, seed=ft)
        assert np.array_equal(A.float_to_words(A.words_to_float(w, ft), ft), w)


def test_same_bits_tells_zero_signs_and_nans_apart():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert A.same_bits(a, a.clone())
    assert not A.same_bits(torch.tensor([-0.0, float("nan"), 1.0]), a)
    assert not A.same_bits(torch.tensor([0.0, 2.0, 1.0]), a)
    q = torch.tensor([0x7fc00001], dtype=torch.int32).view(torch.float32)
    assert A.same_bits(torch.cat([a[:1], q, a[2:]]), a)  # any NaN for a NaN
