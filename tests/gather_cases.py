"""Case tables of the row gather with device-resident indices (DESIGN.md
5.2e): the table shape, the row widths, and for each width the index lists
with the edge kinds each list claims to hold.  numpy only; runs none of the
codec.  tests/test_gather_inputs.py checks the claims, tests/test_gpu_gather.py
runs the lists."""
import math

import numpy as np

BLK = 4096
N_TABLE = 17 * BLK + 1234  # 18 blocks (odd, partial tail)
N_BLOCKS = -(-N_TABLE // BLK)
ROW_WORDS = (1, 7, 8, 64, 257, 1024, 4096, 4097, 9000)
TASKS_PER_WG = 8  # 4 waves x 2 half-waves
N_RANDOM = 700
LONG_RW, LONG_COUNT = 8, 70000  # more task groups than resident workgroups

INT64_MIN = -(1 << 63)


def rows_of(rw, n=N_TABLE):
    return n // rw


def blocks_per_row(rw):
    """K: the most blocks a row of rw words touches."""
    return -(-(BLK - math.gcd(rw, BLK) + rw) // BLK)


def row_blocks(r, rw):
    """(first block, block count) of row r."""
    s = r * rw
    return s // BLK, -(-(s % BLK + rw) // BLK)


def ends_on_edge(r, rw):
    return ((r + 1) * rw) % BLK == 0


def straddles(r, rw):
    """Row r has words on both sides of a block edge."""
    return row_blocks(r, rw)[1] > 1


def in_tail_block(r, rw):
    """Row r's last word lies in the partial tail block."""
    return ((r + 1) * rw - 1) // BLK == N_BLOCKS - 1


def index_lists(rw):
    """name -> (list of row indices, set of edge kinds the list claims).
    Kinds: "first", "last", "ends_on_edge", "straddles", "edge_neighbours"
    (for every interior block edge the row holding the word before it and the
    row holding the word after it, where they are whole rows), "tail_block",
    "twin_in_wave" (one row at list positions 2q and 2q + 1 with K = 1: both
    halves of one wave decode the same block), "same_block_pair" (two distinct
    rows of one block adjacent in the list), "idle_half" (an odd task count),
    "several_groups" (more than one workgroup's pass of tasks)."""
    R = rows_of(rw)
    K = blocks_per_row(rw)
    lists = {}
    lists["first"] = ([0], {"first"})
    last_kinds = {"last"} | ({"tail_block"} if in_tail_block(R - 1, rw) else set())
    lists["last"] = ([R - 1], last_kinds)
    edge = []
    for b in range(1, N_BLOCKS):
        for word in (b * BLK - 1, b * BLK):
            if word // rw < R:
                edge.append(word // rw)
    kinds = {"edge_neighbours"}
    if any(ends_on_edge(r, rw) for r in edge):
        kinds.add("ends_on_edge")
    if any(straddles(r, rw) for r in edge):
        kinds.add("straddles")
    lists["edges"] = (edge, kinds)
    mid = R // 2
    lists["twice"] = ([mid, mid], {"twin_in_wave"} if K == 1 else set())
    if 2 * rw <= BLK:
        # two rows from the middle of a block
        r0 = (5 * BLK + BLK // 2) // rw
        lists["neighbours"] = ([r0, r0 + 1], {"same_block_pair"})
    rng = np.random.default_rng(1000 + rw)
    for n in (1, 2, 3):
        kinds = {"idle_half"} if (n * K) % 2 else set()
        lists[f"len{n}"] = (rng.integers(0, R, n).tolist(), kinds)
    lists["random"] = (rng.integers(0, R, N_RANDOM).tolist(), {"several_groups"})
    return lists


def long_list():
    rng = np.random.default_rng(77)
    return rng.integers(0, rows_of(LONG_RW), LONG_COUNT).tolist()


def failing_indices(rw, wide):
    """Indices that must fail, int64 only ones included when `wide`."""
    R = rows_of(rw)
    bad = [-1, R, R + 5]
    if wide:
        bad += [1 << 31, 1 << 40, INT64_MIN]
    return bad


def mixed_list(rw, wide):
    """(indices, expect ok): failing indices between good neighbours."""
    R = rows_of(rw)
    good = [0, R - 1, R // 2, R // 3, 1 % R, R - 1, 0]
    idx, ok = [], []
    for k, b in enumerate(failing_indices(rw, wide)):
        idx += [good[k % len(good)], b]
        ok += [1, 0]
    idx.append(good[-1])
    ok.append(1)
    return idx, ok
