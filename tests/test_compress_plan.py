"""The compress rule (csrc/compress_plan.h) on the host: tests/cpp/
compress_plan_check.cpp checks DESIGN.md's literal cases (c2's four rounds of
64 XCD-aligned teams, the small batches the size rule sends to three kernels,
the team limit, the checksummed byte archive, the path hook), the routes the
GPU tests state as literals under every occupancy, and sweeps formats, batch
and element sizes, occupancies, checksum, caller histogram, caller-counted
rows, alignment and mode against the formulas of the drivers the rule
replaced.  No HIP, no GPU: only the benchmark would otherwise notice a changed
threshold."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compress_plan_matches_the_driver_formulas(tmp_path):
    exe = str(tmp_path / "compress_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "compress_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # 12 batch sizes x 12 element sizes x 16 occupancies x 2 alignments x 3
    # modes = 13,824 per format and flag set; fp16/bf16/fp32 and fp64 each take
    # 2 checksum x 7 row states = 14 sets, bytes 2 checksum x 2 histogram = 4
    assert "442368 sweep cases, 1105920 skipped, 512 refused for their item count, 0 failures" in r.stdout, \
        r.stdout[-2000:]
