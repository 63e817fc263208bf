"""CPU checks of the sparse-codec generators in tests/util.py and of the two
restatements of the sparse codec: they pin what tests/test_gpu_sparse_edges.py
feeds the kernels and compares them with.  The generators must be seeded and
reach every edge they claim (sizes around the 64-word step, the 1024-word
chunk, the 4096-word tile and the 262,144-word scan workgroup, each with the
four zero / nonzero combinations of the last two words); the C oracle and
tests/pyref.py (written from the reference's kernels, not from the oracle)
must agree byte for byte on every generated element and on the committed
fixtures; and the oracle's decoder must ignore what the reference leaves
uninitialised (the n-2 slot of the list, the bitmap's padding)."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import pyref
from tests.util import (FT_NAME, NP_WORD, SPARSE_BLOCK_EDGE, SPARSE_FAR_N, SPARSE_LARGE_B, SPARSE_SMALL_B,
                        SPARSE_SPECIAL_N, SPARSE_TAILS, sparse_edge_elements, sparse_edge_sizes,
                        sparse_far_element, sparse_special_patterns, sparse_special_words)

FTS = [1, 2, 3, 4]
ALL_ONES = {1: 0xFFFF, 2: 0xFFFF, 3: 0xFFFFFFFF, 4: 0xFFFFFFFFFFFFFFFF}

_ELEMENTS = {}


def elements(ft):
    """sparse_edge_elements(ft), generated once and left unchanged."""
    if ft not in _ELEMENTS:
        _ELEMENTS[ft] = sparse_edge_elements(ft)
    return _ELEMENTS[ft]


def tail_of(w):
    return (bool(w[-2] != 0), bool(w[-1] != 0))


def agree(ft, w, pb=10, checksum=False, what=""):
    """Oracle and pyref archives are identical and the oracle decodes them."""
    a = O.sparse_compress(w, ft, pb, checksum)
    p = pyref.sparse_compress(ft, w, pb, checksum)
    assert a.size == p.size and np.array_equal(a, p), f"oracle and pyref differ: {FT_NAME[ft]} {what} pb{pb}"
    st, dec = O.sparse_decompress(a, ft, pb, checksum)
    assert st == 0 and np.array_equal(dec, w), f"oracle roundtrip: {FT_NAME[ft]} {what} pb{pb}"
    return a


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_edge_elements_are_seeded_and_reach_every_edge(ft):
    els = elements(ft)
    again = sparse_edge_elements(ft)
    assert [e[:2] for e in els] == [e[:2] for e in again]
    assert all(a[2].dtype == NP_WORD[ft] and np.array_equal(a[2], b[2]) for a, b in zip(els, again))
    assert len({name for _, name, _ in els}) == len(els)
    small, large = sparse_edge_sizes()
    assert set(range(201)) <= set(small) and len(small) == len(set(small))
    by_n = {}
    for group, name, w in els:
        assert group == ("large" if w.size >= SPARSE_LARGE_B - 2 else "small"), name
        by_n.setdefault(w.size, []).append(w)
    assert set(by_n) == set(small) | set(large) | set(SPARSE_BLOCK_EDGE)
    # every size with all four tails; in particular B+1 with the gap slot
    # present and x[n-1] nonzero: n-1 = B is then the first word of a step,
    # chunk, tile or scan workgroup
    for n, ws in by_n.items():
        if n >= 2:
            assert {tail_of(w) for w in ws} == set(SPARSE_TAILS), n
    assert {int(w[0] != 0) for w in by_n[1]} == {0, 1} and len(by_n[0]) == 1
    for B in (64,) + SPARSE_SMALL_B + (SPARSE_LARGE_B,):
        for n in (B - 1, B, B + 1, B + 2):
            assert n in by_n, (B, n)
        assert any(tail_of(w) == (False, True) for w in by_n[B + 1]), B
    # the three fills all occur, among the large sizes too
    for sizes in (small, large):
        kinds = set()
        for n in sizes:
            if n >= 8:
                body = by_n[n][0][: n - 2]
                kinds.add("zero" if not body.any() else "dense" if body.all() else "half")
        assert kinds == {"zero", "half", "dense"}
    for n in by_n:
        if n >= 100 and n % 3 == 1:
            frac = float((by_n[n][0][: n - 2] == 0).mean())
            assert 0.3 < frac < 0.7, (n, frac)
    # list lengths on the dense codec's 4096-symbol block edge, and the list
    # that is the n-2 slot alone
    for n in SPARSE_BLOCK_EDGE:
        full = [w for w in by_n[n] if w.all()]
        empty = [w for w in by_n[n] if not w.any()]
        assert full and empty, n
        assert pyref.sparse_list(ft, full[0]).size == n
        assert pyref.sparse_list(ft, empty[0]).tolist() == [0]


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_special_words_hold_every_pattern(ft):
    v = sparse_special_words(ft)
    again = sparse_special_words(ft)
    assert set(v) == {"base", "negzero_n2", "negzero_n1"}
    pats = sparse_special_patterns(ft)
    for name, w in v.items():
        assert w.size == SPARSE_SPECIAL_N and w.dtype == NP_WORD[ft]
        np.testing.assert_array_equal(w, again[name])
        for pname, p in pats.items():
            assert int((w == p).sum()) >= 1, (name, pname)
        assert 0.2 < float((w == 0).mean()) < 0.5
    neg0 = pats["neg_zero"]
    assert neg0 != 0 and neg0.view(NP_WORD[ft]) == 1 << (8 * neg0.itemsize - 1)
    assert tail_of(v["base"]) == (True, True)
    assert v["negzero_n2"][-2] == neg0 and v["negzero_n2"][-1] != 0
    assert v["negzero_n1"][-2] == 0 and v["negzero_n1"][-1] == neg0
    if ft == 4:
        for pname in ("low_half_zero", "low_half_zero_denormal"):
            p = int(pats[pname])
            assert p & 0xFFFFFFFF == 0 and p >> 32 != 0
        for pname in ("high_half_zero", "high_half_zero_top_bit", "min_denormal"):
            p = int(pats[pname])
            assert p >> 32 == 0 and p & 0xFFFFFFFF != 0
    # -0.0 is a list member, not a zero: the list holds every -0.0
    lst = pyref.sparse_list(ft, v["negzero_n1"])
    assert int((lst == neg0).sum()) == int((v["negzero_n1"] == neg0).sum())
    assert lst[-1] == neg0 and lst[-2] == 0


def test_far_element_reaches_the_second_round_of_block_totals():
    w = sparse_far_element()
    assert w.size == SPARSE_FAR_N == 17302606 and w.dtype == np.uint16
    assert w[-2] == 0 and w[-1] != 0
    nz = np.flatnonzero(w)
    assert 0.009 < nz.size / w.size < 0.0101
    # scan workgroup g covers words [g * 262144, (g + 1) * 262144): a chunk of
    # workgroup g sums the totals of workgroups 0 .. g-1, 64 per round
    assert int(nz.max()) >= 65 * SPARSE_LARGE_B
    per_group = np.bincount(nz // SPARSE_LARGE_B, minlength=67)
    assert per_group.size == 67 and per_group[64] > 0 and per_group[65] > 0 and per_group[66] > 0
    assert np.array_equal(w[:100000], sparse_far_element()[:100000])


@pytest.mark.parametrize("pb", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_oracle_and_pyref_agree_on_the_small_group(ft, pb):
    for k, (group, name, w) in enumerate(elements(ft)):
        if group == "small":
            agree(ft, w, pb, what=name)
            if pb == 10 and k % 7 == 0:
                agree(ft, w, pb, checksum=True, what=name + " checksum")


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_oracle_and_pyref_agree_on_the_large_group(ft):
    for k, (group, name, w) in enumerate(elements(ft)):
        if group == "large":
            agree(ft, w, 10, checksum=k % 5 == 0, what=name)


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_oracle_and_pyref_agree_on_special_words(ft):
    for name, w in sparse_special_words(ft).items():
        for ck in (False, True):
            agree(ft, w, 10, checksum=ck, what=name)


def test_oracle_and_pyref_agree_on_the_far_element():
    w = sparse_far_element()
    agree(2, w, 10, what="far element")


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_pyref_decoder_inverts_small_archives(ft):
    for group, name, w in elements(ft):
        if w.size <= 70 or (w.size <= 1026 and name.endswith("t01")):
            a = pyref.sparse_compress(ft, w, 10)
            np.testing.assert_array_equal(pyref.sparse_decompress(ft, a, 10), w, err_msg=name)


def test_committed_sparse_fixtures_equal_pyref():
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz"))
    keys = [k for k in fx.files if k.startswith("s") and k.endswith("_pb10")]
    assert sorted(keys) == ["s2_nz_pb10", "s2_z_pb10", "s3_nz_pb10", "s3_z_pb10"]
    for k in keys:
        ft = int(k[1])
        w = fx[k.replace("_pb10", "_in")]
        np.testing.assert_array_equal(pyref.sparse_compress(ft, w, 10), fx[k], err_msg=k)
        np.testing.assert_array_equal(pyref.sparse_decompress(ft, fx[k], 10), w, err_msg=k)


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_oracle_ignores_the_dont_care_bits(ft):
    """Archives the reference may emit and this project's compressor never
    does: the n-2 slot of the list holds garbage, the bitmap's padding bytes
    and the bits of its last byte past n are set.  They differ from the plain
    archive exactly when such a slot, byte or bit exists, and decode to the
    same words."""
    sel = [(name, w) for group, name, w in elements(ft) if group == "small"]
    sel += [(name, w) for group, name, w in elements(ft) if group == "large" and name.endswith("zero_t01")]
    sel += list(sparse_special_words(ft).items())
    seen = 0
    for k, (name, w) in enumerate(sel):
        n = w.size
        ck = k % 4 == 0
        plain = pyref.sparse_compress(ft, w, 10, ck)
        a = pyref.sparse_compress(ft, w, 10, ck, gap_fill=ALL_ONES[ft], pad_fill=0xFF, pad_bits=True)
        has_gap = n >= 2 and w[n - 2] == 0
        has_pad = n % 128 != 0
        assert np.array_equal(a, plain) == (not has_gap and not has_pad), name
        prefix = 16 + pyref.round_up((n + 7) // 8, 16)
        assert np.array_equal(a[prefix:], plain[prefix:]) == (not has_gap), name
        seen += has_gap
        st, dec = O.sparse_decompress(a, ft, 10, ck)
        assert st == 0 and np.array_equal(dec, w), name
        if n <= 70:
            np.testing.assert_array_equal(pyref.sparse_decompress(ft, a, 10), w, err_msg=name)
    assert seen > 400
