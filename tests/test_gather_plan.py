"""k_gather's grid rule (planGather, csrc/decode_plan.h) on the host, through
tests/cpp/gather_plan_check.cpp: K tasks per index, 8 tasks per task group, and
min(resident slots, task groups) persistent workgroups.  No HIP, no GPU."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 2048  # 256 CUs x 8 resident workgroups


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_plan") / "gather_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "gather_plan_check.cpp"), "-o", exe], check=True, timeout=120)

    def run(*cases):
        args = [str(v) for c in cases for v in c]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows if len(cases) > 1 else rows[0]

    return run


def k_of(rw):
    return -(-(4096 - math.gcd(rw, 4096) + rw) // 4096)


def test_zero_tasks_launch_nothing(plan):
    assert plan((0, 64, SLOTS)) == (1, 1, 0, 0)
    assert plan((0, 9000, SLOTS)) == (1, 4, 0, 0)


def test_fewer_task_groups_than_slots(plan):
    # 1024 rows of 1024 words: K = 1, 128 groups of 8, all side by side
    assert plan((1024, 1024, SLOTS)) == (1, 1, 128, 128)
    # one index still launches one workgroup; 9 tasks need two
    assert plan((1, 64, SLOTS)) == (1, 1, 1, 1)
    assert plan((9, 64, SLOTS)) == (1, 1, 2, 2)
    # K = 4: 3 indices are 12 tasks
    assert plan((3, 9000, SLOTS)) == (1, 4, 2, 2)
    assert plan((SLOTS * 8, 8, SLOTS)) == (1, 1, SLOTS, SLOTS)


def test_more_task_groups_than_slots(plan):
    # one generation of resident workgroups strides over the groups
    assert plan((70000, 8, SLOTS)) == (1, 1, 8750, SLOTS)
    assert plan((SLOTS * 8 + 1, 8, SLOTS)) == (1, 1, SLOTS + 1, SLOTS)
    assert plan((70000, 257, 1792)) == (1, 2, 17500, 1792)
    # a slot count of 0 (never from the occupancy query) still launches
    assert plan((100, 8, 0)) == (1, 1, 13, 1)


def test_k_of_every_width(plan):
    widths = [1, 2, 7, 8, 64, 257, 1024, 4095, 4096, 4097, 8192, 9000, 12288, 12289, (1 << 32) - 1]
    rows = plan(*[(16, rw, SLOTS) for rw in widths])
    for rw, (valid, K, groups, grid) in zip(widths, rows):
        assert valid == 1 and K == k_of(rw), rw
        assert groups == -(-16 * K // 8) and grid == min(SLOTS, groups), rw


def test_overflow_and_zero_width_are_rejected(plan):
    # numIdx * K must stay below 2^32
    assert plan(((1 << 32) - 1, 8, SLOTS))[0] == 1
    assert plan(((1 << 31), 7, SLOTS))[0] == 0            # K = 2: exactly 2^32
    assert plan(((1 << 31) - 1, 7, SLOTS))[:2] == (1, 2)  # 2^32 - 2
    assert plan(((1 << 30), 9000, SLOTS))[0] == 0         # K = 4
    assert plan(((1 << 30) - 1, 9000, SLOTS))[0] == 1
    assert plan((4097, (1 << 32) - 1, SLOTS))[0] == 0     # K = 2^20 + 1
    assert plan((16, 0, SLOTS))[0] == 0
