"""The inputs and the expected result of the sparse decode-and-accumulate tests
(tests/sparse_accumulate_cases.py) checked on their own: numpy, torch and the
CPU oracle only, none of the feature's code.  The expected result must be the
dense model's everywhere except under a +0.0 word whose accumulator is -0.0
or a NaN, and the case list must really hold what the GPU test relies on."""
import numpy as np
import pytest
import torch

from tests import sparse_accumulate_cases as S
from tests.util import FT_NAME, SPARSE_LARGE_B


def dense_model(acc, words, ft, mode):
    return S.model(acc, S.words_to_float(words, ft), mode)


def differs_only_where_allowed(acc, words, ft, mode):
    """-> the number of positions where the sparse result differs from the
    dense model's; every one of them has a +0.0 word under a -0.0 or NaN
    accumulator."""
    want = S.expected(acc, words, ft, mode)
    dense = dense_model(acc, words, ft, mode)
    zero_word = torch.from_numpy(np.ascontiguousarray(words) == 0)
    neg_zero = (acc == 0) & torch.signbit(acc)
    allowed = zero_word & (neg_zero | torch.isnan(acc))
    # (a NaN result is some NaN: its bits are not compared)
    diff = (S.bits(want) != S.bits(dense)) & ~(torch.isnan(want) & torch.isnan(dense))
    assert not bool((diff & ~allowed).any())
    # under a zero word the accumulator keeps its very bits
    assert torch.equal(S.bits(want)[zero_word], S.bits(acc)[zero_word])
    return int(diff.sum())


@pytest.mark.parametrize("ft,mode", S.MODES, ids=S.MODE_IDS)
def test_expected_is_the_dense_model_but_for_skipped_zeros(ft, mode):
    differing = 0
    for k, (name, w) in enumerate(S.small_cases(ft) + S.large_cases(ft)):
        differing += differs_only_where_allowed(S.case_acc(ft, mode, w.size, seed=k), w, ft, mode)
    assert differing > 1000  # -0.0 accumulators under zero words: the deviation is exercised
    if ft <= 2:
        for words, acc in (S.patterns16_dense(ft, mode), S.patterns16_interleaved(ft, mode)):
            differs_only_where_allowed(acc, words, ft, mode)
    elif mode == 1:
        words, acc = S.cross_specials_interleaved(ft)
        assert differs_only_where_allowed(acc, words, ft, mode) > 0


@pytest.mark.parametrize("ft", [1, 2, 3, 4], ids=FT_NAME.get)
def test_the_case_list_holds_what_the_gpu_test_relies_on(ft):
    cases = S.small_cases(ft)
    assert len(cases) > 900
    sizes = {w.size for _, w in cases}
    assert set(range(201)) <= sizes
    for b in (256, 1024, 2048, 4096, 8192):
        assert {b + d for d in range(-2, 3)} <= sizes
    neg0_under_zero = neg0_under_nonzero = False
    tails = set()
    for k, (name, w) in enumerate(cases):
        a = S.case_acc(ft, 1, w.size, seed=k)
        neg0 = ((a == 0) & torch.signbit(a)).numpy()
        neg0_under_zero |= bool((neg0 & (w == 0)).any())
        neg0_under_nonzero |= bool((neg0 & (w != 0)).any())
        if w.size >= 2:
            tails.add((bool(w[-2] != 0), bool(w[-1] != 0)))
    assert neg0_under_zero and neg0_under_nonzero
    assert tails == {(False, False), (False, True), (True, False), (True, True)}
    assert any(w.size > 1024 and not w.any() for _, w in cases)  # an all-zero element
    assert any(w.size > 1024 and w.all() for _, w in cases)      # a zero-free element
    large = S.large_cases(ft)
    assert sorted(w.size for _, w in large) == [SPARSE_LARGE_B + d for d in range(-2, 3)]
    assert {(bool(w[-2] != 0), bool(w[-1] != 0)) for _, w in large} == tails


@pytest.mark.parametrize("ft,mode", [(1, 1), (2, 1), (1, 2), (2, 2)], ids=["fp16-acc1", "bf16-acc1", "fp16-acc2", "bf16-acc2"])
def test_the_16_bit_pattern_elements(ft, mode):
    words, acc = S.patterns16_dense(ft, mode)
    assert words.all() and words.size == acc.numel() == 16 * 65535
    assert set(np.unique(words).tolist()) == set(range(1, 1 << 16))
    words, acc = S.patterns16_interleaved(ft, mode)
    assert words.size == acc.numel() and not words[1::2].any() and words[0::2].all()
    under_zero = acc[1::2]
    assert bool(((under_zero == 0) & torch.signbit(under_zero)).any())
    assert bool(torch.isinf(under_zero).any()) and bool(torch.isnan(under_zero).any())
    tiny = torch.finfo(acc.dtype).tiny
    assert bool(((under_zero != 0) & (under_zero.abs() < tiny)).any())  # denormals
    # the signalling NaN is there, payload and all
    assert int(S.bits(S.acc_specials(ft, mode))[-1]) == S.SNAN_BITS[acc.dtype]
    assert bool(torch.isnan(S.acc_specials(ft, mode)[-1]))


def test_minus_zero_in_the_element_is_added():
    """-0.0 is a nonzero word: +0.0 + (-0.0) = +0.0 is computed, and -0.0 +
    (-0.0) stays -0.0; +0.0 in the element leaves -0.0 alone."""
    for ft in (1, 2, 3, 4):
        neg = S.float_to_words(torch.tensor([-0.0], dtype=S.TORCH_FLOAT[ft]), ft)[0]
        words = np.array([neg, neg, 0, 0], dtype=S.NP_WORD[ft])
        acc = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=S.TORCH_FLOAT[ft])
        want = S.expected(acc, words, ft, 1)
        assert torch.signbit(want).tolist() == [False, True, False, True]
        assert S.touched(words).tolist() == [True, True, False, False]


def test_the_oracle_round_trips_the_cases():
    """The archives the GPU test feeds come from the oracle's sparse
    compressor: it reproduces the words."""
    from oracle import oracle as O

    for ft in (2, 4):
        for name, w in S.small_cases(ft)[::37]:
            st, out = O.sparse_decompress(O.sparse_compress(w, ft, 10), ft, 10)
            assert st == 0 and np.array_equal(out, w), name
