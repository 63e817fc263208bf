"""The case tables of tests/gather_cases.py, checked on the host (numpy only;
none of the codec runs): the bound K on the blocks a row touches, by brute
force over every row start, and that every index list holds the edge kinds it
claims."""
import numpy as np
import pytest

from tests import gather_cases as G


@pytest.mark.parametrize("rw", G.ROW_WORDS)
def test_k_bounds_every_row_and_some_row_attains_it(rw):
    K = G.blocks_per_row(rw)
    # every start a row can have in any table: multiples of rw, modulo the block
    starts = (np.arange(G.BLK, dtype=np.int64) * rw) % G.BLK
    counts = -(-(starts + rw) // G.BLK)
    assert counts.max() == K and counts.min() >= 1
    # ... and some row of the test table attains it too
    mine = [G.row_blocks(r, rw)[1] for r in range(G.rows_of(rw))]
    assert max(mine) == K


def test_the_widths_cover_k_1_2_and_4():
    ks = {rw: G.blocks_per_row(rw) for rw in G.ROW_WORDS}
    assert ks == {1: 1, 7: 2, 8: 1, 64: 1, 257: 2, 1024: 1, 4096: 1, 4097: 2, 9000: 4}
    assert {1, 2, 4} <= set(ks.values())
    # a row that spans more blocks than a wave holds; a tail that is no whole row
    assert ks[9000] > 2 and G.N_TABLE % 9000 != 0 and G.N_TABLE % 1024 != 0
    assert G.N_BLOCKS == 18 and G.N_TABLE % G.BLK == 1234


@pytest.mark.parametrize("rw", G.ROW_WORDS)
def test_every_list_holds_what_it_claims(rw):
    R, K = G.rows_of(rw), G.blocks_per_row(rw)
    lists = G.index_lists(rw)
    assert {"first", "last", "edges", "twice", "len1", "len2", "len3", "random"} <= set(lists)
    assert ("neighbours" in lists) == (2 * rw <= G.BLK)
    claimed = set()
    for name, (idx, kinds) in lists.items():
        claimed |= kinds
        assert idx and all(0 <= r < R for r in idx), name
        for kind in kinds:
            if kind == "first":
                assert 0 in idx
            elif kind == "last":
                assert R - 1 in idx
            elif kind == "tail_block":
                assert any(G.in_tail_block(r, rw) for r in idx)
            elif kind == "ends_on_edge":
                assert any(G.ends_on_edge(r, rw) for r in idx)
            elif kind == "straddles":
                assert any(G.straddles(r, rw) for r in idx)
            elif kind == "edge_neighbours":
                for b in range(1, G.N_BLOCKS):
                    for word in (b * G.BLK - 1, b * G.BLK):
                        assert word // rw >= R or word // rw in idx
            elif kind == "twin_in_wave":
                assert K == 1 and any(idx[q] == idx[q + 1] for q in range(0, len(idx) - 1, 2))
            elif kind == "same_block_pair":
                assert any(a != b and G.row_blocks(a, rw) == G.row_blocks(b, rw) and G.row_blocks(a, rw)[1] == 1
                           for a, b in zip(idx, idx[1:]))
            elif kind == "idle_half":
                assert (len(idx) * K) % 2 == 1
            elif kind == "several_groups":
                assert len(idx) * K > 4 * G.TASKS_PER_WG and len(idx) == G.N_RANDOM
            else:
                raise AssertionError(kind)
    assert [len(lists[f"len{n}"][0]) for n in (1, 2, 3)] == [1, 2, 3]
    assert {"first", "last", "edge_neighbours", "several_groups"} <= claimed
    # a width that does not divide the block has rows on both sides of an edge
    if G.BLK % rw:
        assert "straddles" in claimed
    else:
        assert "ends_on_edge" in claimed
    if K == 1:
        assert "twin_in_wave" in claimed and "idle_half" in claimed


def test_some_width_has_a_row_in_the_tail_block():
    with_tail = [rw for rw in G.ROW_WORDS if "tail_block" in G.index_lists(rw)["last"][1]]
    assert {1, 7, 8, 64, 257, 1024, 4097} <= set(with_tail)
    # 4096 and 9000: the last whole row ends before the tail block
    assert 4096 not in with_tail and 9000 not in with_tail


def test_long_list_outruns_the_resident_workgroups():
    idx = G.long_list()
    assert len(idx) == G.LONG_COUNT and G.blocks_per_row(G.LONG_RW) == 1
    # 8,750 task groups: more than 256 CUs x 8 workgroups hold at once
    assert len(idx) // G.TASKS_PER_WG > 256 * 8
    assert 0 <= min(idx) and max(idx) < G.rows_of(G.LONG_RW)


@pytest.mark.parametrize("rw", G.ROW_WORDS)
@pytest.mark.parametrize("wide", [False, True])
def test_mixed_lists(rw, wide):
    R = G.rows_of(rw)
    idx, ok = G.mixed_list(rw, wide)
    assert len(idx) == len(ok)
    for v, good in zip(idx, ok):
        assert good == int(0 <= v and (v + 1) * rw <= G.N_TABLE) == int(0 <= v < R)
    bad = [v for v, good in zip(idx, ok) if not good]
    assert bad == G.failing_indices(rw, wide)
    assert {-1, R, R + 5} <= set(bad) and ((1 << 40) in bad) == wide == (G.INT64_MIN in bad)
    lim = (1 << 63) if wide else (1 << 31)
    assert all(-lim <= v < lim for v in idx)
    # every failing index sits between two good ones
    assert ok[0] == ok[-1] == 1 and all(ok[k - 1] and ok[k + 1] for k in range(len(ok)) if not ok[k])
