"""What a row gather with device-resident indices costs: the
element and rows of tools/range_decode_bench.py -- one 64 MiB bf16 element,
1024 random rows of 1024 words -- through gather_rows_device (k_gather, the
indices already on the device), through the existing gather_rows (host
indices, one batched range decode) and against the full float_decompress; and
gather_rows_device on 16,384 rows of 64 and of 256 words, the embedding-sized
case.

Kernel times come from the library's event hook (profile_query of the
"decode_gather" / "decode_range" / "decode" families), call times from a host
clock around the call and a device synchronise.  Each figure is the median
over windows of the mean of a window's calls; the cases alternate inside every
window, so drift hits all of them alike.  Prints one JSON line per case and
writes them to --out.

    usage: python tools/gather_bench.py [--out profiles/gather.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/gather.json")
    ap.add_argument("--mib", type=int, default=64)
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    bf16 = torch.bfloat16
    n = a.mib * (1 << 20) // 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, generator=g).to(bf16).to(dev)
    ws = C.Workspace(256 << 20)
    arch2d, sizes = C.float_compress_stride(x.view(1, n), ws=ws)
    archive = arch2d[0, : int(sizes[0])]
    full_out = torch.empty([1, n], dtype=bf16, device=dev)

    cases = {"full": ("decode", lambda: C.float_decompress_stride(arch2d, n, bf16, ws=ws, out=full_out))}
    checks = []

    def device_case(row_words, n_rows, seed):
        rows = np.random.default_rng(seed).integers(0, n // row_words, n_rows)
        idx = torch.from_numpy(rows).to(dev)
        out = torch.empty([n_rows, row_words], dtype=bf16, device=dev)
        ok = torch.empty([n_rows], dtype=torch.uint8, device=dev)
        cases[f"gather_device_{n_rows}_rows_of_{row_words}"] = ("decode_gather", lambda: C.gather_rows_device(
            archive, row_words, idx, bf16, out=out, out_status=ok, ws=ws))
        checks.append((out, ok, row_words, idx))
        return rows

    rows = device_case(1024, 1024, 1).tolist()  # range_decode_bench.py's rows
    host_out = torch.empty([1024, 1024], dtype=bf16, device=dev)
    cases["gather_host_1024_rows_of_1024"] = ("decode_range", lambda: C.gather_rows(
        archive, 1024, rows, bf16, out=host_out, ws=ws))
    device_case(64, 16384, 2)
    device_case(256, 16384, 3)

    # correctness at the sizes timed
    for name, (_, f) in cases.items():
        f()
    torch.cuda.synchronize()
    xi = x.view(torch.int16)
    assert torch.equal(full_out.view(torch.int16).view(-1), xi)
    assert torch.equal(host_out.view(torch.int16), xi.view(-1, 1024)[rows])
    for out, ok, row_words, idx in checks:
        assert bool(ok.all())
        assert torch.equal(out.view(torch.int16), xi.view(-1, row_words)[idx])

    # kernel and call time of the same calls, the profiler on
    gpu = timing.Gpu()
    C.profile(True)
    times = timing.run_windows(cases, lambda name, case: timing.measure(
        case[1], a.calls, gpu, call=True, prof=C, families=(case[0],), check_launches=True), a.windows)
    C.profile(False)

    lines = []
    base = statistics.median(times["full"]["kernel"])
    for name, (family, _) in cases.items():
        t = times[name]
        lines.append({"case": name, "family": family, "element_mib": a.mib, "dtype": "bf16",
                      **timing.summary(t["kernel"], "kernel_us"), **timing.summary(t["call"], "call_us"),
                      "kernel_vs_full": round(statistics.median(t["kernel"]) / base, 4), "windows": a.windows,
                      "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
