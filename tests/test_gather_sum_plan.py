"""k_gatherSum's grid rule (planGatherSum, csrc/decode_plan.h) on the host,
through tests/cpp/gather_sum_plan_check.cpp: ceil(rowWords / 128) column tiles
per bag, a task per (bag, tile), 8 tasks per task group, and min(resident
slots, task groups) persistent workgroups.  No HIP, no GPU."""
import os
import subprocess

import pytest

from tests import gather_sum_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 2048  # 256 CUs x 8 resident workgroups
TILE = 128


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_sum_plan") / "gather_sum_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "gather_sum_plan_check.cpp"), "-o", exe], check=True,
                   timeout=120)

    def run(*cases):
        args = [str(v) for c in cases for v in c]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows if len(cases) > 1 else rows[0]

    return run


def test_the_tile_is_the_case_tables(plan):
    assert plan((1, 1, SLOTS))[1] == TILE == S.TILE


def test_tiles_per_row_at_every_width(plan):
    widths = list(S.ROW_WORDS) + [2, 511, 512, 513, 4096, 9000, (1 << 32) - 1]
    rows = plan(*[(16, rw, SLOTS) for rw in widths])
    for rw, (valid, tile, tiles, tasks, groups, grid) in zip(widths, rows):
        assert valid == 1 and tile == TILE, rw
        assert tiles == -(-rw // TILE) == (S.tiles_of(rw) if rw in S.ROW_WORDS else tiles), rw
        assert tasks == 16 * tiles and groups == -(-tasks // 8) and grid == min(SLOTS, groups), rw
    assert [r[2] for r in rows[:10]] == [1, 1, 1, 1, 1, 1, 2, 3, 8, 33]


def test_zero_bags_launch_nothing(plan):
    assert plan((0, 64, SLOTS)) == (1, TILE, 1, 0, 0, 0)
    assert plan((0, 4097, SLOTS)) == (1, TILE, 33, 0, 0, 0)


@pytest.mark.parametrize("rw,tiles", [(8, 1), (129, 2), (257, 3), (4097, 33)])
def test_tasks_and_grid_around_the_group_count(plan, rw, tiles):
    bags = 1000
    tasks = bags * tiles
    groups = -(-tasks // 8)
    for slots in (1, groups - 1, groups, groups + 1):
        assert plan((bags, rw, slots)) == (1, TILE, tiles, tasks, groups, min(slots, groups)), slots
    # a slot count of 0 (never from the occupancy query) still launches
    assert plan((bags, rw, 0))[5] == 1


def test_one_bag_and_the_long_list(plan):
    assert plan((1, 64, SLOTS)) == (1, TILE, 1, 1, 1, 1)
    assert plan((9, 64, SLOTS)) == (1, TILE, 1, 9, 2, 2)
    assert plan((3, 4097, SLOTS)) == (1, TILE, 33, 99, 13, 13)
    assert plan((S.LONG_BAGS, S.LONG_RW, SLOTS)) == (1, TILE, 1, 70000, 8750, SLOTS)


def test_the_task_bound_and_zero_width(plan):
    # numBags * tiles must stay below 2^32
    assert plan(((1 << 32) - 1, TILE, SLOTS))[:4] == (1, TILE, 1, (1 << 32) - 1)
    assert plan(((1 << 31), TILE + 1, SLOTS))[0] == 0            # 2 tiles: exactly 2^32
    assert plan(((1 << 31) - 1, TILE + 1, SLOTS))[:4] == (1, TILE, 2, (1 << 32) - 2)
    assert plan(((1 << 28), 4097, SLOTS))[0] == 0                # 33 tiles
    assert plan((130150524, 4097, SLOTS))[:4] == (1, TILE, 33, (1 << 32) - 4)
    assert plan((130150525, 4097, SLOTS))[0] == 0
    assert plan((128, (1 << 32) - 1, SLOTS))[0] == 0             # 2^25 tiles
    assert plan((127, (1 << 32) - 1, SLOTS))[0] == 1
    assert plan((16, 0, SLOTS))[0] == 0
    assert plan((0, 0, SLOTS))[0] == 0
