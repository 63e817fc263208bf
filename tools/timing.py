"""The timing harness of the feature benchmarks (tools/*_bench.py).

One window loop: the cases alternate inside every window, so drift hits all of
them alike; window 0 is warm-up and is dropped; every value is the mean of a
window's `calls` calls.  A figure is then the median over the windows, with
the min and max across them.

Three clocks, all in microseconds per call, any of them together around one
run of the calls (`measure`):
  stream  two device events on the stream around the calls (launch gaps
          included)
  call    a host clock around the calls and a device synchronise
  kernel  the library's profile scopes summed over a tuple of kernel families
          (gaps excluded; the caller turns the profiler on), optionally with
          the assertion that every family saw one launch per call
Which clocks a benchmark takes, and whether the profiler is on while it takes
them, is the benchmark's choice: the committed profiles/*.json differ in it.

The loop takes the measurement as a callable and `measure` takes its clocks as
an object, so both run on the CPU with fakes (tests/test_tools.py).
"""
import json
import os
import statistics
import time


class Gpu:
    """The real clocks: torch's device events and synchronise, perf_counter."""

    def __init__(self):
        import torch
        self.cuda = torch.cuda

    def sync(self):
        self.cuda.synchronize()

    def event(self):
        return self.cuda.Event(enable_timing=True)

    clock = staticmethod(time.perf_counter)


def measure(f, calls, gpu, *, stream=False, call=False, prof=None, families=(), check_launches=False):
    """Run f `calls` times under the chosen clocks; {"stream" | "call" |
    "kernel": us per call}.  `prof` is the codec module (profile_reset,
    profile_query); with `families` it selects the kernel clock."""
    if families:
        prof.profile_reset()
    gpu.sync()
    if call:
        t0 = gpu.clock()
    if stream:
        e0, e1 = gpu.event(), gpu.event()
        e0.record()
    for _ in range(calls):
        f()
    if stream:
        e1.record()
    gpu.sync()
    out = {}
    if call:
        out["call"] = 1e6 * (gpu.clock() - t0) / calls
    if stream:
        out["stream"] = 1e3 * e0.elapsed_time(e1) / calls
    if families:
        ms = 0.0
        for fam in families:
            fam_ms, launches = prof.profile_query(fam)
            assert not check_launches or launches == calls, (fam, launches, calls)
            ms += fam_ms
        out["kernel"] = 1e3 * ms / calls
    return out


def run_windows(cases, measure_case, windows):
    """measure_case(name, case) -> {clock: value}, once per case per window,
    windows + 1 times; {name: {clock: [one value per timed window]}}."""
    times = {name: {} for name in cases}
    for w in range(windows + 1):  # window 0 is warm-up
        for name, case in cases.items():
            for clock, v in measure_case(name, case).items():
                if w:
                    times[name].setdefault(clock, []).append(v)
    return times


def summary(values, key):
    """{key: median, key_min, key_max} of one case's windows, rounded as the profiles are."""
    return {key: round(statistics.median(values), 2), key + "_min": round(min(values), 2),
            key + "_max": round(max(values), 2)}


def add_args(ap, out):
    ap.add_argument("--out", default=out)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)


def write_lines(lines, out):
    """Print each line and write them, one JSON object per line, to `out`."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        for ln in lines:
            print(json.dumps(ln))
            fh.write(json.dumps(ln) + "\n")
