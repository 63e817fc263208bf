"""What one torch.ops.dietgpu call costs on the host: every launching operator
on the shape of bench.py's own latency entry, 8 members of 4096 fp16 words and
a 64 MiB temp_mem, where the kernels take a few microseconds and the time is
the operator layer's (csrc/torch_ops.cpp: argument checks, the member columns,
the launch).  The clock is `call`: a host clock around a window's calls (200,
as in bench.py's entry) and one device synchronise.  The cases alternate
inside every window; a figure is the median over windows of the mean of a
window's calls, with the min and max across windows.  Prints one JSON line per
case and writes them to --out, where `tools/ab.py run ... --also
tools/ops_bench.py` picks up the call_us figures.  Reads nothing outside the
repository.

    usage: python tools/ops_bench.py [--out profiles/ops.json]
"""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, WORDS, ROW = 8, 4096, 64

# case (the operator, then what selects its path): (D = torch.ops.dietgpu, a = arguments()) -> one call
CASES = {
    "compress_data": lambda D, a: D.compress_data(True, a.xs, False, a.tmp),
    "compress_data_split_size": lambda D, a: D.compress_data_split_size(True, a.flat, a.split, False, a.tmp),
    "compress_data_simple": lambda D, a: D.compress_data_simple(True, a.xs, False),
    "decompress_data": lambda D, a: D.decompress_data(True, a.rows, a.out16, False, a.tmp),
    "decompress_data_split_size": lambda D, a: D.decompress_data_split_size(True, a.rows, a.out_flat, a.split, False,
                                                                          a.tmp),
    "decompress_data_simple": lambda D, a: D.decompress_data_simple(True, a.rows, False),
    "decompress_data_range": lambda D, a: D.decompress_data_range(True, a.rows, a.out16, a.first, a.tmp),
    "decompress_data_accumulate fp16": lambda D, a: D.decompress_data_accumulate(a.rows, a.out16, a.tmp),
    "decompress_data_accumulate fp32": lambda D, a: D.decompress_data_accumulate(a.rows32, a.out32, a.tmp),  # peeks
    "gather_rows": lambda D, a: D.gather_rows(True, a.table, ROW, a.idx, a.out_rows, a.tmp),
    "reduce_data fp16": lambda D, a: D.reduce_data(a.rows + a.rows, 2, a.out16, None, a.tmp),
    "reduce_data fp32": lambda D, a: D.reduce_data(a.rows32 + a.rows32, 2, a.out32, None, a.tmp),  # peeks
}


def arguments(D, torch, dev="cuda"):
    f16, f32 = torch.float16, torch.float32
    a = SimpleNamespace(xs=[torch.randn(WORDS, device=dev).to(f16) for _ in range(N)],
                        tmp=torch.empty([64 << 20], dtype=torch.uint8, device=dev),
                        split=torch.full([N], WORDS, dtype=torch.int32), first=torch.zeros(N, dtype=torch.int64),
                        idx=torch.arange(N, device=dev, dtype=torch.int32))
    a.flat = torch.cat(a.xs)
    a.rows = D.compress_data_simple(True, a.xs, False)
    a.rows32 = D.compress_data_simple(True, [x.to(f32) for x in a.xs], False)
    a.table = D.compress_data_simple(True, [a.flat], False)[0]  # [N * WORDS / ROW, ROW]
    a.out16, a.out32 = ([torch.zeros(WORDS, dtype=t, device=dev) for _ in range(N)] for t in (f16, f32))
    a.out_flat, a.out_rows = torch.empty_like(a.flat), a.flat.new_empty([N, ROW])
    return a


def main():
    import timing  # (tools/timing.py, next to this script)

    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/ops.json")
    ap.set_defaults(calls=200)
    o = ap.parse_args()

    import torch

    import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)

    D, gpu = torch.ops.dietgpu, timing.Gpu()
    a = arguments(D, torch)
    times = timing.run_windows(CASES, lambda name, f: timing.measure(lambda: f(D, a), o.calls, gpu, call=True),
                               o.windows)
    timing.write_lines([{"case": name, **timing.summary(t["call"], "call_us"), "windows": o.windows,
                         "calls_per_window": o.calls, "device": torch.cuda.get_device_name(0)}
                        for name, t in times.items()], o.out)


if __name__ == "__main__":
    main()
