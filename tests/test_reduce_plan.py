"""The fused reduce's pass and grid rules (planReduce, planReduceGrid,
csrc/decode_plan.h) on the host, through tests/cpp/reduce_plan_check.cpp:
which sources go in which pass, which passes read and write the fp32 partial,
its bytes, and the grid of a pass.  No HIP, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 512  # 256 CUs x 2 resident workgroups (four sources at 10 probability bits)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reduce_plan") / "reduce_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "reduce_plan_check.cpp"), "-o", exe], check=True, timeout=120)

    def run(K, ns_max, partial_words=0, max_blocks=1, ny=1, slots=SLOTS):
        r = subprocess.run([exe] + [str(v) for v in (K, ns_max, partial_words, max_blocks, ny, slots)],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        f = [int(v) for v in r.stdout.split()]
        passes = [tuple(f[5 + 4 * i: 9 + 4 * i]) for i in range((len(f) - 5) // 4)]
        return {"valid": f[0], "num_passes": f[1], "partial_bytes": f[2], "grid_x": f[3], "chunks": f[4],
                "passes": passes}

    return run


def test_one_pass_needs_no_partial(plan):
    for K in (1, 2, 3, 4):
        p = plan(K, 4, partial_words=1000)
        assert p["valid"] == 1 and p["num_passes"] == 1 and p["partial_bytes"] == 0
        assert p["passes"] == [(0, K, 0, 0)]


def test_passes_cover_the_sources_in_order(plan):
    for ns_max in range(1, 9):
        for K in range(1, 65):
            p = plan(K, ns_max, partial_words=12)
            n = -(-K // ns_max)
            assert p["valid"] == 1 and p["num_passes"] == n == len(p["passes"])
            assert p["partial_bytes"] == (48 if n > 1 else 0)
            at = 0
            for i, (first, count, init, out) in enumerate(p["passes"]):
                assert first == at and 1 <= count <= ns_max
                # only the first pass reads the caller's init, only the last writes the caller's out
                assert init == (1 if i > 0 else 0) and out == (1 if i + 1 < n else 0)
                at += count
            assert at == K
            counts = [c for _, c, _, _ in p["passes"]]
            assert max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True)


def test_named_splits(plan):
    assert [c for _, c, _, _ in plan(7, 4)["passes"]] == [4, 3]
    assert [c for _, c, _, _ in plan(9, 4)["passes"]] == [3, 3, 3]
    assert [c for _, c, _, _ in plan(5, 4)["passes"]] == [3, 2]
    assert [c for _, c, _, _ in plan(64, 4)["passes"]] == [4] * 16


def test_k_range(plan):
    assert plan(0, 4)["valid"] == 0 and plan(65, 4)["valid"] == 0 and plan(4, 0)["valid"] == 0
    assert plan(64, 4)["valid"] == 1 and plan(1, 1)["valid"] == 1


def test_grid_follows_the_resident_slots(plan):
    # 1 x 8 Mi words: 2048 blocks, 256 chunks of 8: all side by side
    g = plan(3, 4, max_blocks=2048)
    assert (g["grid_x"], g["chunks"]) == (256, 1)
    # 256 x 512 Ki words: 16 chunks per member, 4096 in all on 512 slots: 8 per workgroup
    g = plan(3, 4, max_blocks=128, ny=256)
    assert (g["grid_x"], g["chunks"]) == (2, 8)
    # fewer slots, more chunks per workgroup, capped at 8
    g = plan(3, 4, max_blocks=2048, slots=64)
    assert (g["grid_x"], g["chunks"]) == (64, 4)
    g = plan(3, 4, max_blocks=65536, slots=64)
    assert (g["grid_x"], g["chunks"]) == (1024, 8)
    # an empty member still launches one workgroup; a slot count of 0 still launches
    assert plan(1, 4, max_blocks=0)["grid_x"] == 1
    assert plan(1, 4, max_blocks=16, slots=0)["grid_x"] >= 1
