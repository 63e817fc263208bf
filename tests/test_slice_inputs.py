"""The batches of the grid-Y slice tests show a forgotten slice offset
(tests/slice_cases.py).  CPU only: the case table against the
properties that make a kernel which treats member i as member i - 65,535 (or
i - 131,070) compute something else, for every member count in the table."""
import numpy as np
import pytest
import torch

from tests import accumulate_cases as A
from tests import slice_cases as SC

FTS = (0, 1, 2, 3, 4)
DISTANCES = (SC.GRID_Y, 2 * SC.GRID_Y)


def test_the_counts_are_the_slice_edges():
    assert SC.GRID_Y == 65535
    assert SC.COUNTS == (65535, 65536, 65537) and SC.THREE_SLICES == 2 * 65535 + 1
    # the sparse reduce's rows, sources x members, straddle one slice
    assert SC.INNER_K * SC.INNER_COUNTS[0] == SC.GRID_Y + 1 and SC.INNER_COUNTS[1] == SC.INNER_COUNTS[0] + 1
    counts = SC.table_counts()
    assert set(counts) <= set(SC.ALL_COUNTS)
    assert set(SC.COUNTS) | {SC.THREE_SLICES} | set(SC.INNER_COUNTS) <= set(counts)
    # every family has a control (nothing sliced) beside its sliced cases
    for name in ("compress-three-kernel", "compress-single-pass", "decode", "accumulate", "reduce",
                 "sparse-compress", "sparse-decompress"):
        nbs = {row[-1] for row in SC.TABLES[name]}
        assert SC.CONTROL in nbs and max(nbs) > SC.GRID_Y, name
    # three slices: the dense and the sparse decode, and one compress (a
    # compress writes 572 KB of archive row per member)
    three = [name for name, t in SC.TABLES.items() for row in t if row[-1] == SC.THREE_SLICES]
    assert sorted(three) == ["compress-three-kernel", "decode", "sparse-decompress"]
    for t in SC.TABLES.values():
        assert len(set(SC.ids(t))) == len(t)


def test_the_period_divides_no_slice_distance():
    assert SC.K_DISTINCT == 7 and len(SC.SIZES) == 7 and len(set(SC.SIZES)) == 7
    for d in DISTANCES:
        assert d % SC.K_DISTINCT != 0
    assert SC.SIZES == (1, 33, 255, 1024, 1025, 4096, 4097)


def _contents(kind, ft):
    make = {"dense": SC.words, "sparse": SC.sparse_words, "rows": SC.row_words}[kind]
    return [make(ft, c) for c in range(SC.K_DISTINCT)]


@pytest.mark.parametrize("nb", SC.ALL_COUNTS)
def test_no_member_equals_the_member_a_slice_before(nb):
    """For every member i >= 65,535 (and >= 131,070): content, size, range and
    accumulator values all differ from those of member i - 65,535 (i -
    131,070)."""
    assert nb in SC.table_counts()
    sizes = np.array(SC.SIZES)
    firsts, counts = SC.member_ranges(nb)
    for d in DISTANCES:
        i = np.arange(d, nb)
        if i.size == 0:
            continue
        assert (SC.which(i) != SC.which(i - d)).all()
        assert (sizes[SC.which(i)] != sizes[SC.which(i - d)]).all()
        assert (SC.acc_which(i) != SC.acc_which(i - d)).all()
        assert (SC.acc_which(i) == SC.which(i + SC.ACC_SHIFT)).all()
        # a range decode: another archive, and nearly always another range of it
        # (the seven lists share ranges such as (0, 1)); where it is the same
        # range and not an empty one, its first word differs
        same = (firsts[i] == firsts[i - d]) & (counts[i] == counts[i - d])
        assert same.mean() < 0.1
        hit = i[same & (counts[i] > 0)]
        for ft in (0, 2):
            first_words = SC.padded([SC.words(ft, c) for c in range(SC.K_DISTINCT)])
            assert (first_words[SC.which(hit), firsts[hit]] != first_words[SC.which(hit - d), firsts[hit]]).all()
    for i in SC.named_members(nb):
        assert 0 <= i < nb
    named = SC.named_members(nb)
    assert nb - 1 in named and (nb <= SC.GRID_Y or {SC.GRID_Y - 1, SC.GRID_Y} <= set(named))


@pytest.mark.parametrize("kind,ft", [("dense", ft) for ft in FTS] + [("rows", 0), ("rows", 2)]
                         + [("sparse", 2), ("sparse", 3)])
def test_the_contents_differ_in_size_and_in_words(kind, ft):
    """Any two of the seven contents differ, also over the words both have
    (the shorter one is no prefix of the longer one), so that a table row, a
    histogram or a checksum taken from the wrong member is a wrong one."""
    ws = _contents(kind, ft)
    assert [w.size for w in ws] == ([SC.ROW] * 7 if kind == "rows" else list(SC.SIZES))
    for a in range(7):
        for b in range(a + 1, 7):
            m = min(ws[a].size, ws[b].size)
            assert not np.array_equal(ws[a][:m], ws[b][:m]), (a, b)
            if ft == 0:
                assert not np.array_equal(np.bincount(ws[a], minlength=256), np.bincount(ws[b], minlength=256))
    if kind == "sparse":
        assert not ws[SC.SPARSE_ALL_ZERO].any() and ws[SC.SPARSE_ZERO_FREE].all()
        share = [float((w == 0).mean()) for c, w in enumerate(ws) if SC.SIZES[c] >= 255]
        assert sum(0.8 < s < 0.97 for s in share) >= 3, share
    # the sources of a reduce: other words of the same sizes
    if kind != "rows":
        make = SC.words if kind == "dense" else SC.sparse_words
        for c in range(7):
            srcs = [make(ft, c, k) for k in range(SC.INNER_K)]
            assert all(s.size == SC.SIZES[c] for s in srcs)
            if SC.SIZES[c] > 1:
                assert all(not np.array_equal(srcs[0], s) for s in srcs[1:])


@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (3, 1)])
@pytest.mark.parametrize("sparse", [False, True])
def test_the_accumulator_values_differ(ft, mode, sparse):
    accs = [SC.acc_values(ft, mode, a, sparse) for a in range(7)]
    assert all(a.dtype == A.acc_dtype(ft, mode) and a.numel() == max(SC.SIZES) for a in accs)
    assert all(bool(torch.isfinite(a).all()) for a in accs)
    for a in range(7):
        for b in range(a + 1, 7):
            assert A.bits(accs[a])[0] != A.bits(accs[b])[0] or sparse  # (sparse: word 0 is -0.0 in all)
            assert not torch.equal(A.bits(accs[a])[:33], A.bits(accs[b])[:33])


def test_the_expected_rows_differ_and_hold_no_nan():
    """The expected rows are compared bit for bit; members a slice apart
    expect other sums."""
    for rows in (SC.accumulate_rows(2, 1), SC.accumulate_rows(2, 2), SC.accumulate_rows(3, 1),
                 SC.sparse_accumulate_rows(2, 1), SC.sparse_accumulate_rows(2, 2), SC.reduce_rows(2, SC.REDUCE_K),
                 SC.sparse_reduce_rows(2, SC.INNER_K)):
        assert [r.numel() for r in rows] in (list(SC.SIZES), list(SC.ALL_SIZES))
        assert not any(bool(torch.isnan(r).any()) for r in rows)
        for c in range(7):
            p = (c - 1) % 7  # 65,535 % 7 == 1: the member a slice before holds content c - 1
            m = min(rows[c].numel(), rows[p].numel())
            if m > 1:
                assert not torch.equal(A.bits(rows[c])[:m], A.bits(rows[p])[:m])
    assert SC.GRID_Y % 7 == 1 and (2 * SC.GRID_Y) % 7 == 2
    assert SC.which(SC.SHORT_MEMBER) == 1 and SC.SHORT_MEMBER == SC.GRID_Y
    assert SC.SHORT_MEMBER not in SC.empty_members(SC.THREE_SLICES)


def test_a_sum_without_the_init_or_a_source_is_another_sum():
    want = SC.reduce_rows(2, SC.REDUCE_K)
    short = SC.reduce_rows(2, SC.REDUCE_K - 1)
    assert all(not torch.equal(A.bits(a), A.bits(b)) for a, b in zip(want[2:], short[2:]))


@pytest.mark.parametrize("nb", SC.ALL_COUNTS)
def test_the_empty_members_lie_past_the_first_slice_and_differ_from_the_member_a_slice_before(nb):
    """The families with an empty member: every batch of at least 65,537
    members has one past 65,535 (of 131,071: one in each later slice), the
    control has one too, the member a slice (two slices) before an empty one
    is not empty, and with the empty members in place it still holds that no
    member equals the member a slice before it."""
    assert SC.EMPTY == 7 and SC.ALL_SIZES[SC.EMPTY] == 0 and SC.ALL_SIZES[:7] == SC.SIZES
    empty = SC.empty_members(nb)
    assert 3 in empty and all(0 <= e < nb for e in empty)
    assert set(empty) <= set(SC.named_members(nb))
    if nb >= SC.GRID_Y + 2:
        assert any(SC.GRID_Y <= e < 2 * SC.GRID_Y for e in empty)
    if nb > 2 * SC.GRID_Y:
        assert any(e >= 2 * SC.GRID_Y for e in empty)
    w = SC.member_contents(nb, empty=True)
    assert np.flatnonzero(w == SC.EMPTY).tolist() == sorted(empty)
    assert np.array_equal(np.delete(w, empty), np.delete(SC.member_contents(nb), empty))
    sizes = np.array(SC.ALL_SIZES)
    for d in DISTANCES:
        i = np.arange(d, nb)
        assert (w[i] != w[i - d]).all() and (sizes[w[i]] != sizes[w[i - d]]).all()


@pytest.mark.parametrize("ft", FTS)
def test_the_empty_content_has_no_words(ft):
    assert SC.words(ft, SC.EMPTY).size == 0 and SC.words(ft, SC.EMPTY).dtype == SC.words(ft, 0).dtype
    if ft:
        assert SC.sparse_words(ft, SC.EMPTY).size == 0
    for rows in (SC.accumulate_rows(2, 1), SC.sparse_accumulate_rows(2, 2)):
        assert len(rows) == SC.CONTENTS and rows[SC.EMPTY].numel() == 0
