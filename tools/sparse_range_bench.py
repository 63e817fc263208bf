"""What a range decode of a sparse archive costs: ranges of
1 Ki, 64 Ki and 1 Mi words near the start, at the middle and near the end of
one 15 M-word fp32 element, and a 1024-row gather from a [15 K, 1024] table,
against the full sparse_decompress of the same element (at 50 % and at 90 %
zeros) on the same device in the same run.

Three figures per case: `stream_us`, the time of a window's calls between two
events on the stream (launch gaps included, the profiling hook off);
`kernel_us`, the library's event hook summed over the call's kernel families
("sparse" plus "decode" or "decode_range"; gaps excluded); `call_us`, a host
clock around the calls and a device synchronise.  Each is the median over the
windows of the mean of a window's calls; all cases alternate inside every
window, so drift hits them alike.  Prints one JSON line per case and writes
them to --out.

    usage: python tools/sparse_range_bench.py [--out profiles/sparse_range_decode.json]
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
    timing.add_args(ap, "profiles/sparse_range_decode.json")
    ap.add_argument("--rows", type=int, default=15 * 1024)
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    row_words, n_rows = 1024, 1024
    n = a.rows * row_words
    ws = C.Workspace(512 << 20)
    g = torch.Generator().manual_seed(0)
    dense = torch.randn(n, generator=g)
    keep = torch.rand(n, generator=g)
    cases, checks = {}, []
    for zeros in (50, 90):
        x = torch.where(keep < zeros / 100.0, torch.zeros(()), dense).to(dev)
        comp, sizes = C.sparse_compress([x], ws=ws)
        torch.cuda.synchronize()
        archive = comp[0, : int(sizes[0])]
        xi = x.view(torch.int32)
        full_out = torch.empty([n], dtype=torch.float32, device=dev)
        cases[f"full_z{zeros}"] = (("sparse", "decode"), lambda archive=archive, full_out=full_out: C.sparse_decompress(
            [archive], [full_out], ws=ws))
        checks.append((full_out, xi))
        for cnt_name, cnt in (("1Ki", 1 << 10), ("64Ki", 1 << 16), ("1Mi", 1 << 20)):
            for where, first in (("start", 1000), ("middle", n // 2 + 1000), ("end", n - cnt - 1000)):
                out = torch.empty([cnt], dtype=torch.float32, device=dev)
                cases[f"range_{cnt_name}_{where}_z{zeros}"] = (
                    ("sparse", "decode_range"), lambda archive=archive, first=first, cnt=cnt, out=out:
                    C.sparse_decompress_range([archive], [first], [cnt], [out], ws=ws))
                checks.append((out, xi[first: first + cnt]))
        rows = np.random.default_rng(1).integers(0, a.rows, n_rows)
        gather_out = torch.empty([n_rows, row_words], dtype=torch.float32, device=dev)
        cases[f"gather_{n_rows}_rows_z{zeros}"] = (("sparse", "decode_range"), lambda archive=archive, rows=rows,
                                                   gather_out=gather_out: C.gather_rows(
            archive, row_words, rows, torch.float32, out=gather_out, ws=ws, sparse=True))
        checks.append((gather_out, xi.view(-1, row_words)[torch.from_numpy(rows).to(dev)]))

    # correctness at the sizes timed
    for _, f in cases.values():
        f()
    torch.cuda.synchronize()
    for got, want in checks:
        assert torch.equal(got.view(torch.int32).reshape(-1), want.reshape(-1))

    gpu = timing.Gpu()

    def measure_case(name, case):
        families, f = case
        C.profile(False)  # stream and call time of the same calls, the profiler off
        t = timing.measure(f, a.calls, gpu, stream=True, call=True)
        C.profile(True)  # kernel time of a second run of the calls
        t.update(timing.measure(f, a.calls, gpu, prof=C, families=families))
        return t

    times = timing.run_windows(cases, measure_case, a.windows)
    C.profile(False)

    lines = []
    for name, t in times.items():
        base = times["full_z" + name.rsplit("_z", 1)[1]]
        lines.append({"case": name, "element_words": n, "dtype": "fp32", **timing.summary(t["stream"], "stream_us"),
                      "kernel_us": round(statistics.median(t["kernel"]), 2),
                      "call_us": round(statistics.median(t["call"]), 2),
                      "stream_vs_full": round(statistics.median(t["stream"]) / statistics.median(base["stream"]), 4),
                      "windows": a.windows, "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
