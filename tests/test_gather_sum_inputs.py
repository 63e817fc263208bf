"""The case tables and the model of tests/gather_sum_cases.py, checked on the
host (numpy and torch on the CPU; none of the codec runs): every bag list
holds the edge kinds it claims, and the model tells a wrong kernel -- another
order, a 16-bit running sum, a start from +0.0 -- from a right one."""
import numpy as np
import pytest
import torch

from tests import gather_cases as G
from tests import gather_sum_cases as S
from tests.util import TORCH_FLOAT


def test_the_widths_surround_the_tile():
    assert {S.TILE - 1, S.TILE, S.TILE + 1} <= set(S.ROW_WORDS)
    assert {1, 7, 8, 64, 257, 1024, 4097} <= set(S.ROW_WORDS)
    assert [S.tiles_of(rw) for rw in (1, S.TILE - 1, S.TILE, S.TILE + 1, 257, 1024, 4097)] == [1, 1, 1, 2, 3, 8, 33]
    assert S.N_TABLE == 17 * 4096 + 1234


@pytest.mark.parametrize("rw", S.ROW_WORDS)
def test_every_list_holds_what_it_claims(rw):
    R = G.rows_of(rw)
    lists = S.bag_lists(rw)
    assert {"lengths", "repeat", "misaligned", "edges", "ends", "odd", "empties"} == set(lists)
    claimed = set()
    for name, (bags, kinds) in lists.items():
        claimed |= kinds
        rows = [r for bag in bags for r in bag]
        assert all(0 <= r < R for r in rows), name
        idx, offsets = S.flatten(bags)
        assert len(offsets) == len(bags) + 1 and offsets[-1] == len(idx) == len(rows)
        for kind in kinds:
            if kind.startswith("len"):
                assert any(len(bag) == int(kind[3:]) for bag in bags), (name, kind)
            elif kind == "repeat":
                assert any(len(bag) > 2 and len(set(bag)) == 1 for bag in bags)
            elif kind == "misaligned":
                ok = False
                for bag in bags:
                    offs, blocks = S.row_offsets_and_blocks(bag, rw)
                    ok = ok or (len(offs) >= min(3, S.BLK // np.gcd(rw, S.BLK)) and len(blocks) >= 3)
                assert ok
            elif kind == "first":
                assert 0 in rows
            elif kind == "last":
                assert R - 1 in rows
            elif kind == "tail_block":
                assert any(G.in_tail_block(r, rw) for r in rows)
            elif kind == "ends_on_edge":
                assert any(G.ends_on_edge(r, rw) for r in rows)
            elif kind == "straddles":
                assert any(G.straddles(r, rw) for r in rows)
            elif kind == "edge_neighbours":
                pooled = bags[0]
                for b in range(1, G.N_BLOCKS):
                    for word in (b * G.BLK - 1, b * G.BLK):
                        assert word // rw >= R or word // rw in pooled
                assert any(len(bag) == 1 for bag in bags[1:])
            elif kind == "idle_half":
                assert (len(bags) * S.tiles_of(rw)) % 2 == 1
            elif kind == "empty_first":
                assert bags[0] == []
            elif kind == "empty_last":
                assert bags[-1] == []
            elif kind == "empty_adjacent":
                assert any(a == [] and b == [] for a, b in zip(bags, bags[1:]))
            else:
                raise AssertionError(kind)
    must = {"len0", "len1", "len2", "len3", "len17", "len700", "repeat", "misaligned", "edge_neighbours", "first",
            "last", "empty_first", "empty_last", "empty_adjacent"}
    assert must <= claimed
    # an odd task count exists wherever the tile count is odd
    assert ("idle_half" in claimed) == (S.tiles_of(rw) % 2 == 1)
    assert len(S.all_bags(rw)) == sum(len(bags) for bags, _ in lists.values())


def test_some_width_has_rows_on_each_side_of_an_edge_and_across_one():
    kinds = {rw: S.bag_lists(rw)["edges"][1] for rw in S.ROW_WORDS}
    assert any("ends_on_edge" in k for k in kinds.values()) and any("straddles" in k for k in kinds.values())
    assert any("tail_block" in S.bag_lists(rw)["ends"][1] for rw in S.ROW_WORDS)


def test_the_long_list_outnumbers_the_resident_workgroups():
    bags = S.long_bags()
    assert len(bags) == S.LONG_BAGS and {len(b) for b in bags} == {1, 2}
    groups = -(-len(bags) * S.tiles_of(S.LONG_RW) // S.TASKS_PER_WG)
    assert groups > 256 * 8 * 4  # several strides of 8 workgroups on each of 256 CUs
    R = G.rows_of(S.LONG_RW)
    assert all(0 <= r < R for b in bags for r in b)


def test_failing_bags_hold_every_bad_index_among_good_rows():
    for wide in (False, True):
        bags, ok = S.failing_bags(64, wide)
        R = G.rows_of(64)
        assert len(bags) == len(ok) and ok[0] == 1 and ok[-1] == 1
        bad = [r for bag in bags for r in bag if not 0 <= r < R]
        assert bad == G.failing_indices(64, wide)
        places = set()
        for bag, good in zip(bags, ok):
            assert good == int(all(0 <= r < R for r in bag))
            if not good:
                assert len(bag) == 4
                places.add([0 <= r < R for r in bag].index(False))
        assert {0, 1, 2} <= places and [] in bags


# ------------------------------------------------- discriminating power ----

def table(ft):
    return S.as_ints(S.table_words(ft)).view(TORCH_FLOAT[ft])


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_the_model_is_the_sequential_fp32_sum(ft):
    t = table(ft)
    rw = 64
    bags = S.bag_lists(rw)["lengths"][0]
    got = S.pooled(t, rw, bags, torch.float32)
    rows = t[: G.rows_of(rw) * rw].view(-1, rw)
    for b, bag in enumerate(bags):
        if not bag:
            assert torch.equal(S.bits(got[b]), torch.zeros(rw, dtype=torch.int32))
            continue
        acc = rows[bag[0]].float()
        for r in bag[1:]:
            acc = acc + rows[r].float()
        assert torch.equal(S.bits(got[b]), S.bits(acc)), b
    # one rounding to a 16-bit output
    if ft != 3:
        assert torch.equal(S.bits(S.pooled(t, rw, bags, TORCH_FLOAT[ft])), S.bits(got.to(TORCH_FLOAT[ft])))


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_wrong_kernels_change_words_of_a_17_row_bag(ft):
    """fp32 output, bag length 17, rowWords 64: the counts are computed here
    and must be nonzero."""
    t = table(ft)
    rw = 64
    bags = [b for b in S.bag_lists(rw)["lengths"][0] if len(b) == 17]
    assert len(bags) == 1
    right = S.pooled(t, rw, bags, torch.float32)
    assert not bool(torch.isnan(right).any())
    reverse = S.pooled(t, rw, bags, torch.float32, order=-1)
    n_reverse = int((S.bits(reverse) != S.bits(right)).sum())
    assert n_reverse > 0
    if ft != 3:
        narrow = S.pooled(t, rw, bags, torch.float32, acc_dtype=TORCH_FLOAT[ft])
        n_narrow = int((S.bits(narrow) != S.bits(right)).sum())
        assert n_narrow > rw // 2  # a 16-bit running sum loses bits in most words


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_a_start_from_zero_changes_every_negative_zero_of_a_one_row_bag(ft):
    neg0 = {1: -0x8000, 2: -0x8000, 3: -0x80000000}[ft]
    w = torch.zeros(4 * 64, dtype={1: torch.int16, 2: torch.int16, 3: torch.int32}[ft])
    w[64:128:2] = neg0
    t = w.view(TORCH_FLOAT[ft])
    for out_dtype in (torch.float32, TORCH_FLOAT[ft]):
        right = S.pooled(t, 64, [[1]], out_dtype)
        assert torch.equal(S.bits(right), S.bits(t[64:128].to(out_dtype)).view(1, 64))
        wrong = S.pooled(t, 64, [[1]], out_dtype, start_zero=True)
        changed = S.bits(wrong) != S.bits(right)
        assert torch.equal(changed.view(-1), w[64:128] == neg0) and int(changed.sum()) == 32


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_order_probe_sums_depend_on_the_order(ft):
    t, bags = S.order_probe(TORCH_FLOAT[ft])
    assert len(bags) == 24 and all(sorted(b) == [0, 1, 2, 3] for b in bags)
    sums = S.pooled(t, 8, bags, torch.float32)
    assert bool((sums == sums[:, :1]).all())  # every word of a bag alike
    seen = {float(v) for v in sums[:, 0]}
    assert seen == {0.0, 2.0 ** -24, 2.0 ** -23}
    rev = S.pooled(t, 8, bags, torch.float32, order=-1)
    assert int((S.bits(rev) != S.bits(sums)).sum()) > 0


def test_value_tables():
    for dt in (torch.float16, torch.bfloat16):
        t = S.all_patterns(dt)
        assert t.numel() == 2 * 65536
        first = S.bits(t[:65536]).to(torch.int32) & 0xffff
        assert torch.equal(first, torch.arange(65536, dtype=torch.int32))
        assert sorted((S.bits(t[65536:]).to(torch.int32) & 0xffff).tolist()) == list(range(65536))
        got = S.pooled(t, 64, S.pattern_pairs(), dt)
        assert got.shape == (1024, 64) and bool(torch.isnan(got.float()).any()) and bool(torch.isinf(got.float()).any())
    t, bags = S.fp32_specials()
    k = int(len(bags) ** 0.5)
    assert t.numel() == k * k * 8 and max(max(b) for b in bags) == k * k - 1
    got = S.pooled(t, 8, bags, torch.float32)
    assert bool(torch.isnan(got).any()) and bool(torch.isinf(got).any())
    assert bool((S.bits(got) == -0x80000000).any())  # -0.0 + -0.0
    assert bool(S.same(got, got).all())
