"""What pooling rows of a compressed table costs: the fused
gather_rows_sum (k_gatherSum, one launch, no temporary) against the path a
user had before it on the same device -- gather_rows_device into a
[numIdx, row_words] temporary, index_add_ of its fp32 copy into a zeroed fp32
[B, row_words] buffer, and (16-bit tables) a cast to the output type.  All
cases run in one process, the two paths alternating inside every window.

Tables of 2^20 rows of 128 words, bf16 and fp32; pooling factors 1, 8, 32 and
128; 4,096 and 65,536 bags; uniform random indices.  Both paths are timed with
device events around a window's calls (launch gaps included: the baseline is
several launches), the cases alternating inside every window; each figure is
the median over the windows with their min and max, which is the spread to
read a difference against.  Beside the times, the bytes each path writes and
re-reads outside the archive: B * pooling * row_words * w written and read
again by the baseline (twice that where the fp32 copy is another buffer),
B * row_words * w written by the fused call.  Prints one JSON line per case
and writes them to --out.

    usage: python tools/gather_sum_bench.py [--out profiles/gather_sum_bench.json]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

POOLING = (1, 8, 32, 128)
BAGS = (4096, 65536)


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/gather_sum_bench.json")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--row-words", type=int, default=128)
    ap.add_argument("--dtypes", default="bf16,fp32")
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    rw, R = a.row_words, a.rows
    ws = C.Workspace(256 << 20)
    gpu = timing.Gpu()
    lines = []
    for name in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]
        g = torch.Generator().manual_seed(0)
        x = torch.randn(R * rw, generator=g).to(dt).to(dev)
        arch2d, sizes = C.float_compress_stride(x.view(1, -1), ws=ws)
        archive = arch2d[0, : int(sizes[0])]
        w = x.element_size()
        cases, meta = {}, {}
        for B in BAGS:
            for pool in POOLING:
                m = B * pool
                rng = np.random.default_rng(B + pool)
                idx = torch.from_numpy(rng.integers(0, R, m)).to(dev)
                offsets = torch.arange(0, m + 1, pool, dtype=torch.int64, device=dev)
                bag_of = torch.arange(B, device=dev).repeat_interleave(pool)
                out = torch.empty([B, rw], dtype=dt, device=dev)
                ok = torch.empty([B], dtype=torch.uint8, device=dev)
                tmp = torch.empty([m, rw], dtype=dt, device=dev)
                tmp_ok = torch.empty([m], dtype=torch.uint8, device=dev)
                acc = torch.empty([B, rw], dtype=torch.float32, device=dev)
                # (an fp32 table's sums are the fp32 buffer itself: no cast)
                base_out = torch.empty([B, rw], dtype=dt, device=dev) if dt != torch.float32 else acc

                def fused(idx=idx, offsets=offsets, out=out, ok=ok):
                    C.gather_rows_sum(archive, rw, idx, offsets, dt, out=out, out_status=ok, ws=ws)

                def baseline(idx=idx, bag_of=bag_of, tmp=tmp, tmp_ok=tmp_ok, acc=acc, base_out=base_out):
                    C.gather_rows_device(archive, rw, idx, dt, out=tmp, out_status=tmp_ok, ws=ws)
                    acc.zero_()
                    acc.index_add_(0, bag_of, tmp.float())
                    if base_out is not acc:
                        base_out.copy_(acc)

                # correctness at the sizes timed: the fused rows against a
                # sequential fp32 sum of the gathered rows (index_add_'s own
                # order is not fixed: it is compared with a tolerance)
                fused()
                baseline()
                torch.cuda.synchronize()
                assert bool(ok.all()) and bool(tmp_ok.all())
                seq = tmp.view(B, pool, rw)[:, 0].float()
                for k in range(1, pool):
                    seq = seq + tmp.view(B, pool, rw)[:, k].float()
                assert torch.equal(seq.to(dt), out), (name, B, pool)
                assert torch.allclose(base_out.float(), out.float(), rtol=2e-2, atol=1e-3), (name, B, pool)
                key = f"{name}_bags{B}_pool{pool}"
                calls = a.calls if m <= (1 << 20) else max(2, a.calls // 8)
                cases[key + "_fused"] = (fused, calls)
                cases[key + "_baseline"] = (baseline, calls)
                moved = {"fused": B * rw * w,
                         "baseline": m * rw * w * 2 + (m * rw * 4 * 2 if dt != torch.float32 else 0)
                         + B * rw * 4 * 3 + (B * rw * (4 + w) if dt != torch.float32 else 0)}
                for path in ("fused", "baseline"):
                    meta[f"{key}_{path}"] = {"dtype": name, "bags": B, "pooling": pool, "path": path,
                                             "bytes_outside_archive": moved[path], "calls_per_window": calls}
        times = timing.run_windows(cases, lambda _, case: timing.measure(case[0], case[1], gpu, stream=True),
                                   a.windows)
        for key in cases:
            line = {"case": key, **meta[key], **timing.summary(times[key]["stream"], "stream_us"),
                    "windows": a.windows, "rows": R, "row_words": rw, "archive_bytes": int(sizes[0]),
                    "device": torch.cuda.get_device_name(0)}
            if key.endswith("_fused"):
                base = statistics.median(times[key[:-6] + "_baseline"]["stream"])
                line["fused_vs_baseline"] = round(statistics.median(times[key]["stream"]) / base, 4)
            lines.append(line)
        del cases, x, arch2d, archive
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
