"""The fused sparse reduce's plan (planSparseReduce, csrc/sparse_plan.h) on the
host, through tests/cpp/sparse_reduce_plan_check.cpp, which includes
sparse_plan.h only: the grids and the element count of every allocation at the
capacity edges, the call's scratch bytes, their bound by the sources of one
launch, and the C ABI's scratch query against the plan.  No HIP, no GPU."""
import os
import subprocess

import pytest

import dietgpu_fork_amd  # noqa: F401
from dietgpu_fork_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (0, 1, 1023, 1024, 1025, 262143, 262144, 262145, 15_000_000)
FIELDS = ("valid", "ns", "rows", "chunks", "cblocks", "grid_x", "dense_capacity", "list_stride", "list_bytes",
          "chunk_pre", "block_tot", "table_bytes", "partial_words", "dense_ptrs", "sizes", "dense_ok", "verdict",
          "first_n", "scratch_bytes", "num_passes")
WORD_BYTES = {1: 2, 2: 2, 3: 4}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sparse_reduce_plan") / "sparse_reduce_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "sparse_reduce_plan_check.cpp"), "-o", exe],
                   check=True, timeout=120)

    def run(word_bytes, nb, K, ns_max, max_cap, has_init=True):
        r = subprocess.run([exe] + [str(int(v)) for v in (word_bytes, nb, K, ns_max, max_cap, has_init)],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        f = [int(v) for v in r.stdout.split()]
        p = dict(zip(FIELDS, f))
        rest = f[len(FIELDS):]
        p["passes"] = [tuple(rest[4 * i: 4 * i + 4]) for i in range(len(rest) // 4)]
        return p

    return run


def up(a, b):
    return -(-a // b) * b


def granules(nbytes):
    return max(up(nbytes, 256), 256)


def expected(word_bytes, nb, K, ns_max, cap, has_init):
    """The plan restated: planReduce's even split, planSparseDecode's sizes for
    the widest pass's rows, every allocation a multiple of 256 bytes."""
    ns_max = min(ns_max, 4)
    passes = -(-K // ns_max)
    ns = -(-K // passes)
    rows = ns * nb
    chunks = max(1, -(-cap // 1024))
    cblocks, grid_x = -(-chunks // 256), -(-chunks // 4)
    stride = (up(cap, 16) + 16) * word_bytes
    table = (K * nb + nb + (nb if has_init else 0)) * 8 + nb * 4
    partial = nb * up(cap, 4) if passes > 1 else 0
    e = dict(valid=1, ns=ns, rows=rows, chunks=chunks, cblocks=cblocks, grid_x=grid_x, dense_capacity=cap + 1,
             list_stride=stride, list_bytes=rows * stride, chunk_pre=rows * chunks, block_tot=rows * cblocks,
             table_bytes=table, partial_words=partial, dense_ptrs=rows, sizes=rows, dense_ok=rows, verdict=2 * nb,
             first_n=nb, num_passes=passes)
    e["scratch_bytes"] = sum(granules(b) for b in (table, 4 * partial, 8 * rows, 4 * rows, rows, rows * stride,
                                                   4 * rows * chunks, 4 * rows * cblocks, 2 * nb, 4 * nb))
    return e


@pytest.mark.parametrize("cap", CAPS)
def test_grids_and_allocation_counts_at_the_capacity_edges(plan, cap):
    for word_bytes in (2, 4):
        for nb, K, has_init in ((1, 1, True), (1, 3, False), (1, 7, True), (5, 4, True), (401, 9, False), (3, 64, True)):
            got = plan(word_bytes, nb, K, 4, cap, has_init)
            want = expected(word_bytes, nb, K, 4, cap, has_init)
            assert {k: got[k] for k in want} == want, (word_bytes, nb, K, cap)
            assert [c for _, c, _, _ in got["passes"]][0] == got["ns"] and sum(c for _, c, _, _ in got["passes"]) == K


def test_named_values(plan):
    p = plan(2, 1, 3, 4, 15_000_000)
    assert (p["chunks"], p["cblocks"], p["grid_x"], p["rows"], p["num_passes"]) == (14649, 58, 3663, 3, 1)
    assert p["list_bytes"] == 3 * (15_000_000 + 16) * 2 and p["partial_words"] == 0
    p = plan(4, 1, 7, 4, 15_000_000)
    assert [c for _, c, _, _ in p["passes"]] == [4, 3] and p["rows"] == 4 and p["partial_words"] == 15_000_000
    assert p["list_bytes"] == 4 * (15_000_000 + 16) * 4
    # an empty capacity still counts one chunk and launches one workgroup per member
    p = plan(2, 2, 2, 4, 0)
    assert (p["chunks"], p["cblocks"], p["grid_x"], p["dense_capacity"], p["list_stride"]) == (1, 1, 1, 1, 32)


def test_scratch_is_bounded_by_the_sources_of_one_launch(plan):
    """Above NSmax sources the scratch no longer grows with K: the rows are
    those of the widest pass (at most NSmax sources), the partial is one fp32
    row per member; only the table of archive addresses (8 bytes each) knows
    K."""
    cap, nb = 262145, 3
    for ns_max in (1, 2, 3, 4):
        for word_bytes in (2, 4):
            full = plan(word_bytes, nb, ns_max, ns_max, cap)  # one pass of NSmax sources: no partial
            # (its empty partial takes one granule, the chained calls' a row per member)
            bound = full["scratch_bytes"] - granules(full["table_bytes"]) - granules(0) + granules(4 * nb * up(cap, 4))
            for K in range(ns_max + 1, 65):
                p = plan(word_bytes, nb, K, ns_max, cap)
                assert p["ns"] <= ns_max and p["rows"] <= full["rows"]
                rest = p["scratch_bytes"] - granules(p["table_bytes"])
                assert rest <= bound
                if p["ns"] == ns_max:
                    assert rest == bound
            a, b = plan(word_bytes, nb, 2 * ns_max, ns_max, cap), plan(word_bytes, nb, 16 * ns_max, ns_max, cap)
            assert b["scratch_bytes"] - a["scratch_bytes"] == (granules(b["table_bytes"]) - granules(a["table_bytes"]))
            assert b["table_bytes"] - a["table_bytes"] == 14 * ns_max * nb * 8


def test_k_range_and_instance_cap(plan):
    assert plan(2, 1, 0, 4, 100)["valid"] == 0 and plan(2, 1, 65, 4, 100)["valid"] == 0
    assert plan(2, 1, 4, 0, 100)["valid"] == 0
    # a cap above the largest instance means that instance
    assert plan(2, 1, 9, 8, 100)["passes"] == plan(2, 1, 9, 4, 100)["passes"]


@pytest.mark.parametrize("hook", [0, 1, 2, 3, 4, 9])
def test_the_c_abi_scratch_query_equals_the_plan(plan, hook):
    """dietgpu_float_reduce_sparse_scratch_bytes: the plan of a call with an
    init, under the current cap on the sources per launch."""
    L = N.lib()
    ns_max = hook if 1 <= hook < 4 else 4
    L.dietgpu_set_reduce_max_sources(hook)
    try:
        for ft in (1, 2, 3):
            for nb, K, cap in ((1, 1, 0), (1, 3, 15_000_000), (1, 7, 15_000_000), (5, 7, 262145), (401, 2, 700),
                               (2, 64, 1025)):
                got = L.dietgpu_float_reduce_sparse_scratch_bytes(ft, nb, K, cap)
                assert got == plan(WORD_BYTES[ft], nb, K, ns_max, cap, True)["scratch_bytes"], (ft, nb, K, cap)
    finally:
        L.dietgpu_set_reduce_max_sources(0)
