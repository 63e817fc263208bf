"""Same-box A/B of two builds of the library: the parent's against the new one.

A refactor is accepted when every time it could have moved holds under

    median(new) - median(parent) <= max - min of the parent's runs

with the two builds alternating on one machine, every run a fresh process
(DESIGN.md section 6).  This is the one implementation of that procedure and
of that rule.

A *library set* is a directory holding what one build left in
dietgpu_fork_amd/_lib/ (the three libraries and api_roundtrip; they link to
each other, so they are swapped together).  `default` names the in-tree set.

    python tools/ab.py build REV [--name parent]
        where git is: export REV, build it with its own csrc/Makefile, copy its
        set to tools/ablibs/<name>/ (git-ignored).
    python tools/ab.py run PARENT_SET NEW_SET --out profiles/NAME.json
        [--rounds 5] [--bench-args "..."] [--also tools/X_bench.py]... [--dump]
        [--tests "tests/test_gpu_parity.py ..."]
        on the GPU machine: per round the new set, then the parent's, each
        swapped in whole for a fresh `bench.py` child and one child per --also
        script.  --tests runs the named GPU tests once per non-default set
        first; --dump adds one `bench.py --dump-outputs` run per set and
        compares the two directories byte for byte.
    python tools/ab.py with SET [--limit 240] -- COMMAND...
        one command as a child under SET (a variant's tests, a debug reader).
    python tools/ab.py judge FILE
        recompute the verdicts of an A/B file (the historical ones included).

Every child runs under `timeout -k 10 <limit>`, one at a time; the first that
exits non-zero ends the run with its status: nothing more is started and
nothing is retried.  The in-tree set is saved first and put back whatever
happens.  This script never touches the GPU itself (no torch, no package).
"""
import argparse
import filecmp
import json
import os
import shlex
import shutil
import subprocess
import sys
import tempfile
from decimal import Decimal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(REPO, "dietgpu_fork_amd", "_lib")
RULE = ("holds: median(new) - median(parent) <= max - min of the parent's runs, in decimal arithmetic "
        "on the values as written in this file, so a tie holds")
BENCH_ARGS = "--full --no-cpu-baseline --steps 20"
PYTEST_ARGS = ["-m", "gpu", "-x", "-q", "--timeout", "120", "--timeout-method", "thread"]


# ---- figures: one named time each ----

def result_line(text):
    """The last line of a bench run's stdout that parses as the {"metric": ...} object."""
    for ln in reversed(text.splitlines()):
        if ln.startswith("{"):
            try:
                d = json.loads(ln)
            except ValueError:
                continue
            if isinstance(d, dict) and "metric" in d:
                return d
    raise ValueError("no result line")


def _put(figs, name, value):
    if name in figs:
        raise ValueError(f"two figures named {name!r}")
    figs[name] = value


def bench_figures(line):
    """{name: ms} of a bench result line: ms_per_step and every numeric field
    whose key, or the key of a dict around it, ends in _ms, plus the headline's
    per-family `kernels`.  A list entry is named by its `config` (extras) or
    its type / batch / words (rows)."""
    figs = {}

    def walk(node, path, timed):
        if isinstance(node, dict):
            for k, v in node.items():
                walk(v, path + [k], timed or k == "ms_per_step" or k.endswith("_ms") or path + [k] == ["kernels"])
        elif isinstance(node, list):
            for i, e in enumerate(node):
                if isinstance(e, dict):
                    key = e["config"] if "config" in e else " ".join(
                        f"{k}={e[k]}" for k in ("type", "batch", "words") if k in e) or f"[{i}]"
                    walk(e, path + [key], timed)
        elif timed and isinstance(node, (int, float)) and not isinstance(node, bool):
            _put(figs, " / ".join(path), node)

    walk(line, [], False)
    return figs


def feature_figures(script, lines):
    """{name: us} of a feature benchmark's JSON lines: every median field
    (`us`, `*_us`), the line named by its `case`, or by its shape / dtype /
    zeros / zero_run / acc / variant."""
    figs = {}
    stem = os.path.basename(script).replace(".py", "")
    for ln in lines:
        ident = [ln["case"]] if "case" in ln else [
            f"{k}={ln[k]}" for k in ("shape", "dtype", "zeros", "zero_run", "acc", "variant") if k in ln]
        for k, v in ln.items():
            if k == "us" or k.endswith("_us"):
                _put(figs, f"{stem} / {' '.join(ident)} / {k}", v)
    return figs


# ---- the rule ----

def _dec(x):
    return Decimal(repr(x))  # the value as JSON writes it


def _median(values):
    s = sorted(_dec(v) for v in values)
    return s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2


def verdict(parent, new):
    """The medians, the parent's spread and whether the figure holds, exact in decimal."""
    pm, nm = _median(parent), _median(new)
    spread = max(map(_dec, parent)) - min(map(_dec, parent))
    return {"parent_median": float(pm), "new_median": float(nm), "parent_spread": float(spread),
            "holds": nm - pm <= spread}


def compare(runs):
    """runs: {"parent": [{name: value}, ...], "new": [...]}, one dict per run;
    (figures, summary) of the A/B file."""
    series = {role: {} for role in runs}
    for role, rs in runs.items():
        for r in rs:
            for name, v in r.items():
                series[role].setdefault(name, []).append(v)
    figures = [{"figure": name, "unit": "us" if name.endswith(("/ us", "_us")) else "ms", "parent": vals,
                "new": series["new"][name], **verdict(vals, series["new"][name])}
               for name, vals in series["parent"].items() if name in series["new"]]
    summary = {"figures": len(figures), "holds": sum(f["holds"] for f in figures),
               "does_not_hold": [f["figure"] for f in figures if not f["holds"]],
               "only_in": {role: [n for n in series[role] if n not in series[other]]
                           for role, other in (("parent", "new"), ("new", "parent"))}}
    return figures, summary


def judge(doc):
    """Recompute every verdict of an A/B file from its recorded runs:
    {call: {figures, holds, does_not_hold, disagree}}, the top level as ""
    and one entry per nested call.  Reads the historical spellings too."""
    out = {}

    def walk(node, path):
        figs = node.get("figures")
        if isinstance(figs, list) and figs and isinstance(figs[0], dict):
            now = [verdict(f["parent"], f["new"])["holds"] for f in figs]
            was = [f["holds"] if "holds" in f else f["within_spread"] for f in figs]
            out[path] = {"figures": len(figs), "holds": sum(now),
                         "does_not_hold": [f["figure"] for f, h in zip(figs, now) if not h],
                         "disagree": [f["figure"] for f, h, w in zip(figs, now, was) if h != w]}
        for k, v in node.items():
            if isinstance(v, dict):
                walk(v, f"{path}/{k}" if path else k)

    walk(doc, "")
    return out


# ---- library sets ----

def set_files(d):
    return sorted(f for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))


def swap_in(src, lib_dir):
    """Make lib_dir's files those of the set `src`, every one of them."""
    for f in set_files(lib_dir):
        os.remove(os.path.join(lib_dir, f))
    for f in set_files(src):
        shutil.copy2(os.path.join(src, f), os.path.join(lib_dir, f))


def resolve(name, saved, lib_dir):
    """A set's directory; `default` (or lib_dir itself) is the saved in-tree set."""
    d = os.path.abspath(name)
    if name == "default" or d == os.path.abspath(lib_dir):
        return saved
    if not os.path.isdir(d) or not set_files(d):
        raise SystemExit(f"ab: no library set in {name}")
    return d


def build(rev, name):
    jobs = min(16, os.cpu_count() or 8)
    tmp = tempfile.mkdtemp(prefix="ab_build_")
    try:
        tar = subprocess.Popen(["git", "-C", REPO, "archive", rev], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=tar.stdout)
        if tar.wait():
            raise SystemExit(f"git archive {rev} failed")
        subprocess.check_call(["make", "-s", f"-j{jobs}", "-C", os.path.join(tmp, "dietgpu_fork_amd", "csrc")])
        dst = os.path.join(REPO, "tools", "ablibs", name)
        os.makedirs(dst, exist_ok=True)
        swap_in(os.path.join(tmp, "dietgpu_fork_amd", "_lib"), dst)
        print("built", rev, "->", os.path.relpath(dst, REPO), set_files(dst))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- the run ----

def run_child(argv, limit, out):
    """One child to its end: stdout to `out`, stderr to out + ".err"; its exit status."""
    with open(out, "w") as fo, open(out + ".err", "w") as fe:
        return subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=fo, stderr=fe).returncode


def dirs_differ(a, b):
    """The files, by relative path, that are not byte for byte the same in both directories."""
    def files(d):
        return {os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs}
    fa, fb = files(a), files(b)
    return sorted((fa ^ fb) | {f for f in fa & fb
                               if not filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)})


def write_doc(doc, path):
    """The A/B file: one line per top-level field and per figure."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    figures = "[\n  " + ",\n  ".join(json.dumps(f) for f in doc["figures"]) + "\n ]"
    with open(path, "w") as fh:
        fh.write(",\n".join(f" {json.dumps(k)}: {figures if k == 'figures' else json.dumps(v)}"
                            for k, v in doc.items()).join(("{\n", "\n}\n")))


def run_with(set_dir, argv, limit, lib_dir=LIB_DIR):
    """One command under the set `set_dir`, its output passed through; its exit status."""
    saved = tempfile.mkdtemp(prefix="ab_default_")
    swap_in(lib_dir, saved)
    try:
        swap_in(resolve(set_dir, saved, lib_dir), lib_dir)
        return subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO).returncode
    finally:
        swap_in(saved, lib_dir)
        shutil.rmtree(saved, ignore_errors=True)


def run(a, child=run_child, lib_dir=LIB_DIR):
    """The A/B run; 0 with the file written, or the first failing child's status."""
    logs = os.path.abspath(a.logs or os.path.join("bench_out", os.path.basename(a.out).replace(".json", "")))
    os.makedirs(logs, exist_ok=True)
    py = [sys.executable, "-u"]
    bench = py + ["bench.py"] + shlex.split(a.bench_args)
    saved = tempfile.mkdtemp(prefix="ab_default_")
    swap_in(lib_dir, saved)
    order = ("new", "parent")
    runs = {role: [] for role in order}
    device = None

    def step(role, argv, limit, tag):
        swap_in(sets[role], lib_dir)
        out = os.path.join(logs, tag)
        print(f"ab: {tag} ({role})", flush=True)
        rc = child(argv, limit, out)
        if rc:
            print(f"ab: {tag} ({role}) exited {rc}; stopping, see {out}.err", file=sys.stderr)
        return rc, out

    try:
        sets = {role: resolve(s, saved, lib_dir) for role, s in zip(("parent", "new"), a.sets)}
        for role in order:
            if a.tests and sets[role] != saved:
                rc, _ = step(role, py + ["-m", "pytest"] + shlex.split(a.tests) + PYTEST_ARGS, a.tests_limit,
                             f"tests_{role}.log")
                if rc:
                    return rc
        outputs_equal = None
        if a.dump:
            for role in order:
                rc, _ = step(role, bench + ["--dump-outputs", os.path.join(logs, f"dump_{role}")], a.bench_limit,
                             f"dump_{role}.log")
                if rc:
                    return rc
            dumps = [os.path.join(logs, f"dump_{role}") for role in order]
            if not all(os.path.isdir(d) and os.listdir(d) for d in dumps):
                raise SystemExit("ab: a --dump run wrote no outputs")
            outputs_equal = dirs_differ(*dumps) or True
            if outputs_equal is True:  # equal: nothing to look at
                for d in dumps:
                    shutil.rmtree(d)
        for r in range(1, a.rounds + 1):
            for role in order:
                rc, out = step(role, bench, a.bench_limit, f"bench_{role}_{r}.log")
                if rc:
                    return rc
                figs = bench_figures(result_line(open(out).read()))
                for script in a.also:
                    lines_out = os.path.join(logs, f"{os.path.basename(script)}_{role}_{r}.json")
                    rc, _ = step(role, py + [script, "--out", lines_out], a.also_limit,
                                 f"{os.path.basename(script)}_{role}_{r}.log")
                    if rc:
                        return rc
                    lines = [json.loads(ln) for ln in open(lines_out)]
                    device = device or lines[0].get("device")
                    for name, v in feature_figures(script, lines).items():
                        _put(figs, name, v)
                runs[role].append(figs)
    finally:
        swap_in(saved, lib_dir)
        shutil.rmtree(saved, ignore_errors=True)

    figures, summary = compare(runs)
    doc = {"what": a.what or f"same-box A/B of the library sets {a.sets[0]} (parent) and {a.sets[1]} (new)",
           "device": device, "command": [" ".join(bench[2:])] + [f"{s} --out ..." for s in a.also],
           "order": f"new, parent, x{a.rounds}; every run a fresh process", "rounds": a.rounds, "rule": RULE,
           "figures": figures, "summary": summary, "outputs_equal": outputs_equal}
    write_doc(doc, a.out)
    print(json.dumps({**summary, "outputs_equal": outputs_equal}))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build")
    b.add_argument("rev")
    b.add_argument("--name", default="parent")
    r = sub.add_parser("run")
    r.add_argument("sets", nargs=2, metavar="SET", help="the parent's set, then the new one; `default` = in-tree")
    r.add_argument("--out", required=True)
    r.add_argument("--rounds", type=int, default=5)
    r.add_argument("--bench-args", default=BENCH_ARGS)
    r.add_argument("--also", action="append", default=[], metavar="tools/X_bench.py")
    r.add_argument("--tests", default="", help="GPU test files to run once per non-default set before any timing")
    r.add_argument("--dump", action="store_true")
    r.add_argument("--what", default="")
    r.add_argument("--logs", default="", help="directory of the children's output (default bench_out/<NAME>)")
    r.add_argument("--bench-limit", type=int, default=400, help="seconds per bench.py child")
    r.add_argument("--also-limit", type=int, default=240, help="seconds per --also child")
    r.add_argument("--tests-limit", type=int, default=300, help="seconds per --tests child")
    w = sub.add_parser("with")
    w.add_argument("set")
    w.add_argument("--limit", type=int, default=240, help="seconds")
    w.add_argument("command", nargs="+", help="after --")
    j = sub.add_parser("judge")
    j.add_argument("file")
    a = ap.parse_args(argv)
    if a.cmd == "build":
        build(a.rev, a.name)
        return 0
    if a.cmd == "run":
        return run(a)
    if a.cmd == "with":
        return run_with(a.set, a.command, a.limit)
    calls = judge(json.load(open(a.file)))
    for path, c in calls.items():
        print(json.dumps({"call": path or "(top level)", **c}))
    return int(any(c["disagree"] for c in calls.values()))


if __name__ == "__main__":
    sys.exit(main())
