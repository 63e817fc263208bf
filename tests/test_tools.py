"""The measuring tools: tools/ab.py (the same-box A/B driver and its rule),
tools/timing.py (the feature benchmarks' window loop and clocks) and
tools/variants.py (every variant still applies).  CPU tests but the last: the
A/B children and the clocks are fakes."""
import importlib.util
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(f"tools_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ab = _load("ab")
timing = _load("timing")


def _profile(name):
    return json.load(open(os.path.join(ROOT, "profiles", name)))


# ---- the rule reproduces the recorded verdicts ----

@pytest.mark.parametrize("name, call, figures, holds", [
    ("sparse_rails_ab.json", "", 306, 305),
    ("compress_plan_ab.json", "", 348, 343),
    ("decode_body_ab.json", "", 90, 90),
    ("decode_driver_ab.json", "five_round_call", 42, 42),
    ("decode_driver_ab.json", "three_round_call", 42, 38),
])
def test_judge_reproduces_recorded_verdicts(name, call, figures, holds):
    calls = ab.judge(_profile(name))
    assert all(c["disagree"] == [] for c in calls.values()), calls  # the nested calls too
    assert (calls[call]["figures"], calls[call]["holds"]) == (figures, holds)


def test_judge_names_what_does_not_hold_and_a_tie_holds():
    (name,) = ab.judge(_profile("sparse_rails_ab.json"))[""]["does_not_hold"]
    assert name.endswith("float32 b5 n10000000 compress_ms")
    doc = _profile("compress_plan_ab.json")
    (tie,) = [f for f in doc["figures"]
              if "5 x 15M fp32, 90 % zeros" in f["figure"] and f["figure"].endswith(" / kernels_ms / d:sparse")]
    v = ab.verdict(tie["parent"], tie["new"])
    assert (v["parent_median"], v["new_median"], v["parent_spread"]) == (35.8, 36.1, 0.3)
    assert 36.1 - 35.8 > 0.3 and v["holds"] and tie["within_spread"]  # binary floats would say no
    assert tie["figure"] not in ab.judge(doc)[""]["does_not_hold"]
    assert not ab.verdict([1.0, 1.1, 1.2], [1.4, 1.5, 1.3])["holds"]  # 0.3 > 0.2
    assert ab.verdict([1.0, 1.2], [1.3, 1.3])["holds"]  # even count: 1.3 - 1.1 = 0.2, a tie


def test_judge_command_line(capsys):
    assert ab.main(["judge", os.path.join(ROOT, "profiles", "decode_body_ab.json")]) == 0
    top = json.loads(capsys.readouterr().out.splitlines()[0])
    assert (top["figures"], top["holds"]) == (90, 90)


# ---- figure extraction ----

def test_bench_figures_of_the_committed_full_line():
    text = open(os.path.join(ROOT, "profiles", "r06e_bench.json")).read()
    line = ab.result_line("warning: noise\n{not json\n" + text + "\ntrailing words\n")
    figs = ab.bench_figures(line)
    names = list(figs)
    assert len(set(names)) == len(names) and "ms_per_step" in names
    assert list(ab.bench_figures(line)) == names
    for want in ("kernels / compress", "decode_hbm / decode_cold_ms",
                 "extras / c4: 5 x 15M fp32, 90 % zeros (sparse bitmap + dense codec) / kernels_ms / d:sparse"):
        assert want in figs, want
    rows = [n for n in names if " / rows / type=float32 batch=5 words=10000000 / " in n]
    assert [n.rsplit(" / ", 1)[1] for n in rows] == ["compress_ms", "decompress_ms"]
    assert all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in figs.values())
    assert not any("GBps" in n or n.endswith("ratio") for n in names)


def test_two_extras_of_one_config_raise():
    line = {"metric": "m", "ms_per_step": 1.0, "extras": [{"config": "a", "compress_ms": 1.0},
                                                          {"config": "a", "compress_ms": 2.0}]}
    with pytest.raises(ValueError, match="two figures named"):
        ab.bench_figures(line)
    with pytest.raises(ValueError, match="two figures named"):
        ab.feature_figures("tools/x_bench.py", [{"case": "full", "call_us": 1.0}, {"case": "full", "call_us": 2.0}])


def test_a_figure_of_one_set_only_is_reported():
    base = {"metric": "m", "ms_per_step": 0.2, "extras": [{"config": "a", "compress_ms": 1.0}]}
    more = {"metric": "m", "ms_per_step": 0.2, "extras": [{"config": "a", "compress_ms": 1.0},
                                                          {"config": "b", "compress_ms": 3.0}]}
    figures, summary = ab.compare({"parent": [ab.bench_figures(base)] * 3, "new": [ab.bench_figures(more)] * 3})
    assert [f["figure"] for f in figures] == ["ms_per_step", "extras / a / compress_ms"]
    assert summary["only_in"] == {"parent": [], "new": ["extras / b / compress_ms"]}
    assert (summary["figures"], summary["holds"], summary["does_not_hold"]) == (2, 2, [])


def test_feature_figures_of_the_committed_profiles():
    for name, count in (("accumulate", 12), ("sparse_accumulate", 21), ("range_decode", 14),
                        ("sparse_range_decode", 66), ("gather", 10)):
        lines = [json.loads(ln) for ln in open(os.path.join(ROOT, "profiles", f"{name}.json"))]
        figs = ab.feature_figures(f"tools/{name}_bench.py", lines)
        assert len(figs) == count and not any(n.endswith(("_min", "_max")) for n in figs), name


# ---- the run: order, stopping, the in-tree set ----

def _args(tmp_path, **kw):
    a = dict(sets=[str(tmp_path / "parent"), "default"], out=str(tmp_path / "out" / "ab.json"), rounds=3,
             bench_args=ab.BENCH_ARGS, also=[], tests="", dump=False, what="", logs=str(tmp_path / "logs"),
             bench_limit=400, also_limit=240, tests_limit=300)
    a.update(kw)
    return SimpleNamespace(**a)


def _sets(tmp_path):
    lib, parent = tmp_path / "_lib", tmp_path / "parent"
    for d, tag in ((lib, b"new"), (parent, b"parent")):
        d.mkdir()
        for f in ("libdietgpu_amd.so", "libdietgpu_torch.so", "libdietgpu_testhooks.so"):
            (d / f).write_bytes(tag + b" " + f.encode())
    (lib / "obj").mkdir()  # the objects' directory is no part of a set
    return lib, {f: (lib / f).read_bytes() for f in ab.set_files(lib)}


def _fake_child(lib, seen, fail_at=None):
    def child(argv, limit, out):
        which = (lib / "libdietgpu_amd.so").read_bytes().split()[0].decode()
        assert {(lib / f).read_bytes().split()[0].decode() for f in ab.set_files(lib)} == {which}  # the whole set
        seen.append((which, limit, argv))
        if len(seen) == fail_at:
            return 139
        if "--out" in argv:
            with open(argv[argv.index("--out") + 1], "w") as fh:
                fh.write(json.dumps({"case": "full", "stream_us": 10.0 + len(seen), "stream_us_min": 1.0,
                                     "device": "fake"}) + "\n")
        else:
            with open(out, "w") as fh:
                line = {"metric": "m", "ms_per_step": round(0.2 + len(seen) / 1000, 4)}
                fh.write("noise\n" + json.dumps(line) + "\n")
        return 0
    return child


def test_run_alternates_and_restores(tmp_path):
    lib, before = _sets(tmp_path)
    seen = []
    a = _args(tmp_path, also=["tools/sparse_range_bench.py"])
    assert ab.run(a, child=_fake_child(lib, seen), lib_dir=str(lib)) == 0
    assert [s[0] for s in seen] == ["new", "new", "parent", "parent"] * 3  # bench, then the --also script
    assert [s[1] for s in seen] == [400, 240] * 6
    assert all(s[2][:2] == [sys.executable, "-u"] for s in seen)
    assert {f: (lib / f).read_bytes() for f in ab.set_files(lib)} == before
    doc = json.load(open(a.out))
    assert list(doc) == ["what", "device", "command", "order", "rounds", "rule", "figures", "summary", "outputs_equal"]
    assert doc["rule"] == ab.RULE and "tie holds" in doc["rule"] and doc["rounds"] == 3 and doc["device"] == "fake"
    fig = {f["figure"]: f for f in doc["figures"]}
    assert list(fig) == ["ms_per_step", "sparse_range_bench / full / stream_us"]
    assert list(fig["ms_per_step"]) == ["figure", "unit", "parent", "new", "parent_median", "new_median",
                                        "parent_spread", "holds"]
    assert fig["ms_per_step"]["new"] == [0.201, 0.205, 0.209] and fig["ms_per_step"]["parent"] == [0.203, 0.207, 0.211]
    assert (fig["ms_per_step"]["unit"], fig["sparse_range_bench / full / stream_us"]["unit"]) == ("ms", "us")
    assert ab.judge(doc)[""]["disagree"] == []


def test_run_stops_at_the_first_failing_child(tmp_path):
    lib, before = _sets(tmp_path)
    seen = []
    a = _args(tmp_path)
    assert ab.run(a, child=_fake_child(lib, seen, fail_at=3), lib_dir=str(lib)) == 139  # round 2's first child
    assert [s[0] for s in seen] == ["new", "parent", "new"]
    assert not os.path.exists(a.out)
    assert {f: (lib / f).read_bytes() for f in ab.set_files(lib)} == before


def test_run_tests_and_dump_come_first(tmp_path):
    lib, before = _sets(tmp_path)
    seen = []

    def child(argv, limit, out):
        if "--dump-outputs" in argv:
            d = argv[argv.index("--dump-outputs") + 1]
            os.makedirs(d)
            with open(os.path.join(d, "sizes.npy"), "wb") as fh:
                fh.write((lib / "libdietgpu_amd.so").read_bytes().split()[0])  # differs between the sets
        return _fake_child(lib, seen)(argv, limit, out)

    a = _args(tmp_path, rounds=1, dump=True, tests="tests/test_gpu_parity.py")
    assert ab.run(a, child=child, lib_dir=str(lib)) == 0
    kinds = [("pytest" if "pytest" in s[2] else "dump" if "--dump-outputs" in s[2] else "bench", s[0]) for s in seen]
    assert kinds == [("pytest", "parent"), ("dump", "new"), ("dump", "parent"), ("bench", "new"), ("bench", "parent")]
    assert seen[0][1] == 300 and seen[0][2][-len(ab.PYTEST_ARGS):] == ab.PYTEST_ARGS
    assert json.load(open(a.out))["outputs_equal"] == ["sizes.npy"]
    assert {f: (lib / f).read_bytes() for f in ab.set_files(lib)} == before


def test_ab_keeps_off_the_gpu():
    src = open(os.path.join(ROOT, "tools", "ab.py")).read()
    assert "import torch" not in src and "dietgpu_fork_amd import" not in src and "os.exec" not in src
    r = subprocess.run([sys.executable, "-c", "import sys, ab; sys.exit('torch' in sys.modules)"],
                       cwd=os.path.join(ROOT, "tools"), timeout=60)
    assert r.returncode == 0


# ---- the timing loop with fake clocks ----

class _FakeGpu:
    """A clock that every call of a case advances by that case's cost."""

    def __init__(self):
        self.now = 0.0
        self.log = []

    def sync(self):
        pass

    def clock(self):
        return self.now

    def event(self):
        gpu = self

        class Event:
            def record(self):
                self.t = gpu.now

            def elapsed_time(self, other):
                return 1e3 * (other.t - self.t)  # ms
        return Event()


class _FakeProf:
    def __init__(self, launches_per_call=1):
        self.per_call = launches_per_call
        self.ms = self.n = 0

    def profile_reset(self):
        self.ms = self.n = 0

    def profile_query(self, family):
        return self.ms, self.n

    def launch(self, ms):
        self.ms += ms
        self.n += self.per_call


def _fake_cases(gpu, prof):
    window = {"n": -1}

    def case(name, seconds):
        def f():
            gpu.now += seconds * (1 + max(window["n"], 0))  # window w costs (1 + w) times the base
            prof.launch(1e3 * seconds / 2)
            gpu.log.append(name)
        return f
    return window, {"a": case("a", 1e-6), "b": case("b", 4e-6)}


def test_window_loop_drops_window_zero_alternates_and_summarises():
    gpu, prof = _FakeGpu(), _FakeProf()
    window, cases = _fake_cases(gpu, prof)

    def measure_case(name, f):
        if name == "a":
            window["n"] += 1
        return timing.measure(f, 2, gpu, stream=True, call=True, prof=prof, families=("decode",), check_launches=True)

    times = timing.run_windows(cases, measure_case, 3)
    assert gpu.log == ["a", "a", "b", "b"] * 4  # 3 windows and the warm-up, the cases alternating inside each
    assert {k: len(v) for k, v in times["a"].items()} == {"call": 3, "stream": 3, "kernel": 3}
    # window 0 (cost x1) is gone: the timed windows cost x2, x3, x4; us per call
    assert times["a"]["call"] == pytest.approx([2.0, 3.0, 4.0])
    assert times["b"]["stream"] == pytest.approx([8.0, 12.0, 16.0])
    assert times["b"]["kernel"] == pytest.approx([2.0, 2.0, 2.0])
    assert timing.summary(times["b"]["stream"], "stream_us") == {"stream_us": 12.0, "stream_us_min": 8.0,
                                                                "stream_us_max": 16.0}
    assert timing.summary([3.004, 1.0, 2.0, 10.0], "us") == {"us": 2.5, "us_min": 1.0, "us_max": 10.0}


def test_launch_count_assertion_fires():
    gpu, prof = _FakeGpu(), _FakeProf(launches_per_call=2)
    _, cases = _fake_cases(gpu, prof)
    with pytest.raises(AssertionError):
        timing.measure(cases["a"], 2, gpu, prof=prof, families=("decode",), check_launches=True)
    assert timing.measure(cases["a"], 2, gpu, prof=prof, families=("decode",)) == {"kernel": pytest.approx(0.5)}


def test_write_lines(tmp_path, capsys):
    lines = [{"case": "full", "call_us": 1.5}, {"case": "x", "call_us": 2.0}]
    timing.write_lines(lines, str(tmp_path / "sub" / "out.json"))
    assert [json.loads(ln) for ln in open(tmp_path / "sub" / "out.json")] == lines
    assert [json.loads(ln) for ln in capsys.readouterr().out.splitlines()] == lines


def test_ops_bench_times_every_launching_operator():
    """tools/ops_bench.py's case table names every torch operator but the
    four size operators, which launch nothing."""
    from dietgpu_fork_amd import ops

    sizes = {"max_float_compressed_output_size", "max_float_compressed_size", "max_any_compressed_output_size",
             "max_any_compressed_size"}
    assert {case.split()[0] for case in _load("ops_bench").CASES} == set(ops.OPS + ops.MORE_OPS + ops.REDUCE_OPS) - sizes


# ---- variants ----

def test_every_variant_applies():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "variants.py"), "--check"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "stale" not in r.stdout and r.stdout.count("applies") >= 40, r.stdout + r.stderr
    variants = _load("variants")
    for name, subs in variants.VARS.items():
        for f, _, _ in subs:
            assert os.path.exists(os.path.join(ROOT, "dietgpu_fork_amd", "csrc", f)), (name, f)
    assert "pskew" in variants.VARS  # tests/test_gpu_progress.py points at it


# ---- the harness on a real call ----

@pytest.mark.gpu
def test_harness_on_a_real_call():
    """float_compress_stride of one 4096-word bf16 element and its
    float_decompress_stride, alternating, 2 windows of 2 calls: every clock
    gives one finite positive value per timed window, and the profile scopes
    see one launch per call."""
    import math

    import torch

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to("cuda").view(1, 4096)
    ws = C.Workspace(16 << 20)
    arch2d, _ = C.float_compress_stride(x, ws=ws)
    out = torch.empty_like(x)
    cases = {"compress": (("encode",), lambda: C.float_compress_stride(x, ws=ws)),
             "decompress": (("decode",), lambda: C.float_decompress_stride(arch2d, 4096, torch.bfloat16, ws=ws,
                                                                           out=out))}
    gpu = timing.Gpu()

    def measure_case(name, case):
        families, f = case
        C.profile(False)
        t = timing.measure(f, 2, gpu, stream=True, call=True)
        C.profile(True)
        t.update(timing.measure(f, 2, gpu, prof=C, families=families, check_launches=True))
        return t

    try:
        with C.compress_path("three-kernel"):  # one k_encode launch per call, whatever the size rule says
            times = timing.run_windows(cases, measure_case, 2)
    finally:
        C.profile(False)
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))
    for name in cases:
        assert sorted(times[name]) == ["call", "kernel", "stream"]
        for clock, values in times[name].items():
            assert len(values) == 2 and all(math.isfinite(v) and v > 0 for v in values), (name, clock, values)
