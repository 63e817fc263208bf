"""The pinned staging ring's placement policy (StagingPlan, csrc/staging_plan.h)
on the host, through tests/cpp/staging_plan_check.cpp: where an upload of 64 KiB
to 2 MiB goes in the 8 MiB ring and which earlier uploads it waits for.  The
program drives the policy with modelled in-order streams and checks every
placement against a brute-force model that knows each use's region and whether
its copy has run.  No HIP, no GPU; tests/test_gpu_uploads.py runs the same
sequences through the real ring."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("staging_plan") / "staging_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dietgpu_fork_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "staging_plan_check.cpp"), "-o", exe], check=True, timeout=120)

    def run(case):
        r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    return run


def fields(line):
    return {k: int(v) for k, v in re.findall(r"([a-zA-Z0-9-]+) (\d+)", line)}


def test_the_policy_header_needs_no_hip():
    text = open(os.path.join(ROOT, "dietgpu_fork_amd", "csrc", "staging_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()


def test_rounding_wrap_and_limits(check):
    assert "rounding ok" in check("rounding")


def test_wrap_that_skips_a_pending_tail(check):
    """Seven 1 MiB uploads and a sync; a stall; H of 917,504 B in the tail at
    7 MiB; N1..N7 of 1 MiB from offset 0; N8 of 1,310,720 B wraps onto N1 and
    N2 while H, the oldest use, is pending in the tail that the wrap skipped.
    The policy must wait; the front-only rule the ring had before (the control
    inside the program) hands N8 the bytes of N1 and N2, and the model must
    say so."""
    out = check("skipped-tail")
    assert "skipped-tail ok" in out
    control = [ln for ln in out.splitlines() if ln.startswith("front-only control:")]
    assert len(control) == 2
    assert "[0, 1310720) overwrites pending use 8 [0, 1048576)" in control[0]
    assert "[0, 1310720) overwrites pending use 9 [1048576, 2097152)" in control[1]


def test_a_stalled_stream_does_not_hold_up_another(check):
    got = fields(check("two-streams"))
    assert got["uploads"] == 40 and got["waits"] == 0 and got["wraps"] >= 3


def test_nothing_waits_when_every_copy_has_run(check):
    got = fields(check("instant"))
    assert got["placements"] >= 10000 and got["waits"] == 0


@pytest.mark.parametrize("streams", [2, 3])
def test_random_uploads_stalls_and_drains(check, streams):
    """At least 10,000 placements of 65,540 B to 2 MiB (hundreds of exactly
    2 MiB) on streams that run, stall and catch up independently, with drains
    in between; every invariant of the program's header after each.  The run
    must have filled the ring with pending uses and waited, or it proved
    nothing."""
    got = fields(check(f"random{streams}"))
    assert got["streams"] == streams and got["placements"] >= 10000
    assert got["waits"] >= 100 and got["drains"] >= 10 and got["of-2MiB"] >= 100
    assert got["most-pending-bytes"] > 6 << 20
