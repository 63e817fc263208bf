"""k_decode's grid rule (csrc/decode_plan.h) on the host: tests/cpp/
decode_plan_check.cpp checks DESIGN.md's literal cases (c2's P = 2, c3's
P = 8 over several generations, the capacityOnly and range grids) and sweeps
block counts, batch sizes, resident-slot counts and all four decode forms
against the three launch formulas the rule replaced.  No HIP, no GPU: only the
benchmark would otherwise notice a changed P."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_plan_matches_the_launch_formulas(tmp_path):
    exe = str(tmp_path / "decode_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "decode_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # 11 block counts x 7 batch sizes x 4 slot counts x 2 x 4 forms
    assert "2464 sweep cases, 0 failures" in r.stdout, r.stdout[-2000:]
