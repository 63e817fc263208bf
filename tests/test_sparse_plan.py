"""The sparse drivers' host arithmetic (csrc/sparse_plan.h) on the host:
tests/cpp/sparse_plan_check.cpp restates the formulas that sparseCompressT,
sparseDecompressT and sparseRangeT held inline and sweeps them against
planSparseCompress, planSparseDecode and planSparseRange: every float type at
batch sizes 1 to 65,536 and sizes from 0 to 2^32 - 1 around the tile and chunk
edges; range calls of 1 to 300 members over repeated, unsorted archives, with
empty ranges, ends at and past 2^32 - 1, and the call that is refused as too
large beside the one that just fits.  Each range plan is also checked by brute
force (slots, running workgroup offsets, chunks counted, sizes).  No HIP, no
GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_plans_match_the_driver_formulas(tmp_path):
    exe = str(tmp_path / "sparse_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "sparse_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # 4 float types x 4 batch sizes x 12 sizes x (2 compress + 1 decode) = 576;
    # 300 mixed member lists, 10 ends x 4 settings, 3 around the too-large flag
    assert "919 sparse plan cases, 0 failures" in r.stdout, r.stdout[-2000:]
