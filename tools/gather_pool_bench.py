"""What embedding_bag's other forms cost on a compressed table (DESIGN.md
5.2n): the fused gather_rows_pool (k_gatherPool, one launch, no temporary) in
weighted sum, mean and max, against the path a user had before it --
gather_rows_device into a [numIdx, row_words] temporary, then torch's
reduction over it in the table's own type (mean, amax) or its multiply by the
fp32 weights and sum -- and against gather_rows_sum on the same
routing, which prices the weight and the select over the plain sum.

Tables of 2^20 rows of 128 words, bf16 and fp32; 4,096 and 65,536 bags;
pooling 1, 8, 32 and 128; uniform random indices, bags of one length.  Device
events around a window's calls, the candidates alternating inside every window;
each figure is the median over the windows with their min and max, the spread
a difference is read against.  Every candidate is compared with an fp64
reduction of the gathered rows before anything is timed.  Prints one JSON line
per case and writes them to --out.

    usage: python tools/gather_pool_bench.py [--out profiles/gather_pool_bench.json]
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
BAGS = (65536, 4096)
MODES = ("wsum", "mean", "max")


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/gather_pool_bench.json")
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
        for B in BAGS:
            for pool in POOLING:
                m = B * pool
                rng = np.random.default_rng(B + pool)
                idx = torch.from_numpy(rng.integers(0, R, m)).to(dev)
                offsets = torch.arange(0, m + 1, pool, dtype=torch.int64, device=dev)
                wts = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(dev)
                out = {k: torch.empty([B, rw], dtype=dt, device=dev) for k in MODES + ("sum",)}
                two = {k: torch.empty([B, rw], dtype=dt, device=dev) for k in MODES}
                ok = torch.empty([B], dtype=torch.uint8, device=dev)
                tmp = torch.empty([m, rw], dtype=dt, device=dev)
                tmp_ok = torch.empty([m], dtype=torch.uint8, device=dev)

                def fused(mode):
                    kw = dict(per_sample_weights=wts) if mode == "wsum" else dict(mode=mode)
                    C.gather_rows_pool(archive, rw, idx, offsets, dt, out=out[mode], out_status=ok, ws=ws, **kw)

                def plain_sum():
                    C.gather_rows_sum(archive, rw, idx, offsets, dt, out=out["sum"], out_status=ok, ws=ws)

                def two_step(mode):
                    C.gather_rows_device(archive, rw, idx, dt, out=tmp, out_status=tmp_ok, ws=ws)
                    # what a user would write: only the weighted sum needs fp32 rows
                    # (the multiply promotes them); torch's mean of a 16-bit
                    # tensor accumulates in fp32 itself and amax is exact
                    rows = tmp.view(B, pool, rw)
                    if mode == "wsum":
                        two[mode].copy_((rows * wts.view(B, pool, 1)).sum(1))
                    elif mode == "mean":
                        torch.mean(rows, 1, out=two[mode])
                    else:
                        torch.amax(rows, 1, out=two[mode])

                # correctness at the sizes timed, before any timing
                C.gather_rows_device(archive, rw, idx, dt, out=tmp, out_status=tmp_ok, ws=ws)
                rows64 = tmp.view(B, pool, rw)[: 512].double()
                want = {"wsum": (rows64 * wts.view(B, pool, 1)[: 512].double()).sum(1), "mean": rows64.mean(1),
                        "max": rows64.amax(1)}
                plain_sum()
                for mode in MODES:
                    fused(mode)
                    two_step(mode)
                    torch.cuda.synchronize()
                    assert bool(ok.all()) and bool(tmp_ok.all())
                    for got in (out[mode], two[mode]):
                        assert torch.allclose(got[: 512].double(), want[mode], rtol=2e-2, atol=1e-2), (name, B, pool, mode)
                assert torch.allclose(out["sum"][: 512].double(), rows64.sum(1), rtol=2e-2, atol=1e-2)
                del rows64, want

                key = f"{name}_bags{B}_pool{pool}"
                calls = a.calls if m <= (1 << 20) else max(2, a.calls // 8)
                cases = {f"{key}_sum": (plain_sum, calls)}
                for mode in MODES:
                    cases[f"{key}_{mode}_fused"] = (lambda mode=mode: fused(mode), calls)
                    cases[f"{key}_{mode}_twostep"] = (lambda mode=mode: two_step(mode), calls)
                times = timing.run_windows(cases, lambda _, case: timing.measure(case[0], case[1], gpu, stream=True),
                                           a.windows)
                med = {k: statistics.median(v["stream"]) for k, v in times.items()}
                for k in cases:
                    line = {"case": k, "dtype": name, "bags": B, "pooling": pool, "calls_per_window": calls,
                            **timing.summary(times[k]["stream"], "stream_us"), "windows": a.windows, "rows": R,
                            "row_words": rw, "device": torch.cuda.get_device_name(0)}
                    if k.endswith("_fused"):
                        line["fused_vs_twostep"] = round(med[k] / med[k[:-6] + "_twostep"], 4)
                        line["fused_vs_plain_sum"] = round(med[k] / med[f"{key}_sum"], 4)
                    lines.append(line)
                timing.write_lines(lines, a.out)  # (kept up to date: a run cut short leaves what it measured)
                del cases, out, two, tmp
        del x, arch2d, archive
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
