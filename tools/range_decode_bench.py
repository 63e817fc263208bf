"""What a range decode costs: ranges of 1 .. 1024 blocks
starting mid-archive, and a 1024-row gather, of one 64 MiB bf16 element,
against the full float_decompress of that element.

Kernel times come from the library's event hook (profile_query of the
"decode_range" / "decode" families), call times from a host clock around the
call and a device synchronise.  Each figure is the median over windows of the
mean of a window's calls; the cases alternate inside every window, so drift
hits all of them alike.  Prints one JSON line per case and writes them to
--out.

    usage: python tools/range_decode_bench.py [--out profiles/range_decode.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

BLK = 4096


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/range_decode.json")
    ap.add_argument("--mib", type=int, default=64)
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    n = a.mib * (1 << 20) // 2
    row_words, n_rows = 1024, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, generator=g).to(torch.bfloat16).to(dev)
    ws = C.Workspace(256 << 20)
    arch2d, sizes = C.float_compress_stride(x.view(1, n), ws=ws)
    archive = arch2d[0, : int(sizes[0])]
    full_out = torch.empty([1, n], dtype=torch.bfloat16, device=dev)
    mid = (n // BLK // 2) * BLK
    rows = np.random.default_rng(1).integers(0, n // row_words, n_rows).tolist()
    gather_out = torch.empty([n_rows, row_words], dtype=torch.bfloat16, device=dev)

    cases = {"full": ("decode", lambda: C.float_decompress_stride(arch2d, n, torch.bfloat16, ws=ws, out=full_out))}
    for blocks in (1, 8, 64, 512, 1024):
        cnt = blocks * BLK
        out = torch.empty([cnt], dtype=torch.bfloat16, device=dev)
        cases[f"range_{blocks}_blocks"] = ("decode_range", lambda cnt=cnt, out=out: C.float_decompress_range(
            [archive], [mid], [cnt], [out], dtype=torch.bfloat16, ws=ws))
    cases[f"gather_{n_rows}_rows_of_{row_words}"] = ("decode_range", lambda: C.gather_rows(
        archive, row_words, rows, torch.bfloat16, out=gather_out, ws=ws))

    # correctness at the sizes timed
    for name, (_, f) in cases.items():
        f()
    torch.cuda.synchronize()
    xi = x.view(torch.int16)
    assert torch.equal(full_out.view(torch.int16).view(-1), xi)
    assert torch.equal(gather_out.view(torch.int16), xi.view(-1, row_words)[rows])

    # kernel and call time of the same calls, the profiler on
    gpu = timing.Gpu()
    C.profile(True)
    times = timing.run_windows(cases, lambda name, case: timing.measure(
        case[1], a.calls, gpu, call=True, prof=C, families=(case[0],), check_launches=True), a.windows)
    C.profile(False)

    lines = []
    base = statistics.median(times["full"]["kernel"])
    for name, t in times.items():
        lines.append({"case": name, "element_mib": a.mib, "dtype": "bf16", **timing.summary(t["kernel"], "kernel_us"),
                      "call_us": round(statistics.median(t["call"]), 2),
                      "kernel_vs_full": round(statistics.median(t["kernel"]) / base, 4), "windows": a.windows,
                      "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
