"""CPU checks of what tests/test_gpu_sparse_range.py feeds the kernels
(tests/sparse_range_cases.py): every element is accepted by the CPU oracle and
round-trips, the reference-legal variants are accepted too, and on every
element and every range the rank identity of DESIGN.md 5.2c, restated in numpy
(model_range), gives x[first : first + count] from the bitmap and a slice of
the nonzero list -- with the slot before x[n-1] holding garbage.  Oracle and
pyref alone; no GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import pyref
from tests import sparse_range_cases as K
from tests.util import FT_NAME, NP_WORD, sparse_edge_elements, sparse_far_element

FTS = [1, 2, 3, 4]


def check_ranges(ft, x, ranges):
    """model_range on every range, with the n-2 slot of the list all ones."""
    lst = pyref.sparse_list(ft, x, gap_fill=K.ALL_ONES[ft])
    for first, count in ranges:
        got, lf, lc = K.model_range(x, lst, first, count)
        assert np.array_equal(got, x[first: first + count]), (FT_NAME[ft], x.size, first, count)


def roundtrips(ft, x, pb=10, checksum=False):
    a = O.sparse_compress(x, ft, pb, checksum)
    st, dec = O.sparse_decompress(a, ft, pb, checksum)
    assert st == 0 and np.array_equal(dec, x)


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_edge_elements_and_ranges(ft):
    els = {name: w for _, name, w in sparse_edge_elements(ft)}
    names = K.edge_names(K.EDGE_SMALL + K.EDGE_LARGE)
    assert len(names) == 1 + 2 + 4 * 14
    members = 0
    for name in names:
        x = els[name]
        ranges = K.edge_ranges(x.size)
        assert (0, x.size) in ranges and (0, 0) in ranges and (x.size, 0) in ranges
        check_ranges(ft, x, ranges)
        roundtrips(ft, x)
        members += len(ranges)
    assert members > 2000  # many members per archive


def test_edge_ranges_reach_every_point():
    r = K.edge_ranges(262145)
    firsts, ends = {a for a, _ in r}, {a + c for a, c in r}
    want = set(K.EDGE_POINTS) | {262143, 262144, 262145}
    assert firsts == want and ends == want
    assert K.edge_ranges(0) == [(0, 0)] and K.edge_ranges(1) == [(0, 0), (0, 1), (1, 0)]
    assert (64, 0) in K.edge_ranges(64) and (63, 1) in K.edge_ranges(64)


@pytest.mark.parametrize("ft", [2, 3], ids=FT_NAME.get)
def test_list_block_element(ft):
    x = K.list_block_element(ft)
    assert x.size == 3 * 4096 * 2 + 5 and x.dtype == NP_WORD[ft]
    ranges = K.list_block_ranges(x)
    rank = K.rank_table(x)
    assert sorted({int(rank[f]) for f, _ in ranges}) == [4095, 4096, 4097]
    assert sorted({c for _, c in ranges}) == [1, 2, 9000]
    check_ranges(ft, x, ranges)
    roundtrips(ft, x)


def test_workgroup_total_elements():
    x = K.wg_element()
    assert x.size == 2 * 262144 + 1102
    ranges = K.wg_ranges()
    for e in (262144, 524288):
        assert any(f < e < f + c for f, c in ranges) and any(f + c == e for f, c in ranges)
        assert any(f == e for f, c in ranges)
    check_ranges(2, x, ranges)
    roundtrips(2, x)
    far = sparse_far_element()
    fr = K.far_ranges()
    assert fr[0][0] + fr[0][1] <= 1024 and fr[1][0] < 64 * 262144 < fr[1][0] + fr[1][1]
    assert fr[2] == (far.size - 3, 3) and fr[3] == (far.size - 1025, 1025)
    check_ranges(2, far, fr)
    roundtrips(2, far)


@pytest.mark.parametrize("ft", [2, 4], ids=FT_NAME.get)
def test_quirk_archives_are_legal(ft):
    """The pyref archives with an all-ones n-2 slot, 0xFF padding bytes, the
    bits past n set and 0xFF in header bytes 4..15 (don't-care: the reference
    leaves them uninitialised): the oracle decodes them to x."""
    els = {name: w for _, name, w in sparse_edge_elements(ft)}
    seen = set()
    for name in K.edge_names(K.QUIRK_SIZES):
        x = els[name]
        seen.add(bool(x[-2] != 0))
        a = pyref.sparse_compress(ft, x, 10, gap_fill=K.ALL_ONES[ft], pad_fill=0xFF, pad_bits=True).copy()
        st, dec = O.sparse_decompress(a, ft, 10)
        assert st == 0 and np.array_equal(dec, x)
        a[4:16] = 0xFF
        st, dec = O.sparse_decompress(a, ft, 10)
        assert st == 0 and np.array_equal(dec, x)
        assert np.array_equal(pyref.sparse_decompress(ft, a, 10), x)
        check_ranges(ft, x, K.quirk_ranges(x.size))
    assert seen == {False, True}


def test_parameter_and_gather_inputs():
    els = {name: w for _, name, w in sparse_edge_elements(3)}
    x = els["n4097_dense_t01"]
    for pb in (9, 11):
        roundtrips(3, x, pb=pb)
    roundtrips(3, x, checksum=True)
    t = K.gather_table()
    assert t.shape == (4096, 1024) and 0.88 < float((t == 0).mean()) < 0.92
    rows = K.gather_rows()
    assert rows.size == 256 and 0 in rows and 4095 in rows and len(set(rows.tolist())) < 256
    flat = t.reshape(-1)
    roundtrips(2, flat)
    check_ranges(2, flat, [(int(r) * 1024, 1024) for r in rows[:16]])
