"""What the fused sparse reduce saves: one sparse_reduce call
(k_sparseReduce: K sparse archives expanded side by side, the running sum in
registers) against the per-peer loop it replaces in dist.reduce_archives --
acc = own.float(), one sparse_decompress_accumulate call per peer around an
fp32 accumulator in HBM, acc.to(dtype).  Shapes: 1 x 15 M words, bf16 and
fp32, K = 3 and K = 7, with 90 % zeros at random word positions, 90 % zeros as
whole 1000-word rows, and 50 % zeros at random positions; a workspace that
holds the plan.

Times are device events around a window's calls; each figure is the median
over windows of the mean of a window's calls, with the min and max across
windows; the variants alternate inside every window, so drift hits all alike.
Both results of one call on the same inputs are compared bit for bit first.
"worthwhile": the fused median lies below the loop's by more than the spread
between windows (the routing rule).  --candidates adds the fused call with its
launches capped at 3 and at 2 sources (the kernel's source-limit candidates)
to every window.  Prints one JSON line per case and variant and writes them to
--out.  Reads nothing outside the repository.

    usage: python tools/sparse_reduce_bench.py [--candidates] [--only N] [--out profiles/sparse_reduce.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

N15M = 15_000_000
# (words, dtype, K, fraction of zeros, run: zeros fall on whole runs of this many words)
CASES = tuple((N15M, dtype, K, zeros, run)
              for dtype in (torch.bfloat16, torch.float32) for K in (3, 7)
              for zeros, run in ((0.9, 1), (0.9, 1000), (0.5, 1)))


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/sparse_reduce.json")
    ap.add_argument("--only", type=int, default=None, help="run only case number N")
    ap.add_argument("--candidates", action="store_true",
                    help="also time the fused call capped at 3 and at 2 sources per launch")
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    gpu = timing.Gpu()
    lines = []
    for ci, (n, dtype, K, zeros, run) in enumerate(CASES):
        if a.only is not None and a.only != ci:
            continue
        ft = C.FLOAT_TYPE[dtype]
        wb = torch.empty(0, dtype=dtype).element_size()
        need = C.sparse_reduce_scratch_bytes(ft, 1, K, n)
        ws = C.Workspace(need + (64 << 20))  # the plan, and the compressor's own scratch
        g = torch.Generator(device=dev).manual_seed(K + run)
        own = torch.randn(n, generator=g, device=dev).to(dtype)
        sources, comp_bytes, nnz = [], 0, 0
        for k in range(K):
            x = torch.randn(n, generator=g, device=dev).to(dtype)
            x[x == 0] = 1  # (the zeros are the mask's)
            x.view(n // run, run)[torch.rand(n // run, generator=g, device=dev) < zeros] = 0
            arch2d, sizes = C.sparse_compress([x], ft=ft, ws=ws)
            size = int(sizes[0])
            sources.append([arch2d[0, :size].clone()])
            comp_bytes += size
            nnz += int((x != 0).sum())
            del x, arch2d
        out = torch.empty_like(own)
        acc = torch.empty(n, dtype=torch.float32, device=dev)
        result = {}

        def fused():
            C.sparse_reduce(sources, [out], inits=[own], ft=ft, ws=ws)

        def loop():
            acc.copy_(own)  # own.float()
            for row in sources:
                C.sparse_decompress_accumulate(row, [acc], ft=ft, ws=ws)
            result["loop"] = acc.to(dtype)

        # the two ways agree bit for bit on the same inputs
        fused()
        loop()
        torch.cuda.synchronize()
        it = torch.int16 if wb == 2 else torch.int32
        assert torch.equal(out.view(it), result["loop"].view(it)), "fused and per-peer results differ"
        assert ws.max_usage() <= ws.buf.numel(), "the workspace does not hold the plan"

        def capped(ns):  # the fused call with at most ns sources per launch (the NSmax candidates)
            def f():
                C.set_reduce_max_sources(ns)
                fused()
                C.set_reduce_max_sources(0)
            return f

        variants = {"fused": fused, "loop": loop}
        if a.candidates:
            variants.update({f"fused_ns{ns}": capped(ns) for ns in (3, 2)})
        times = {k: v["stream"] for k, v in timing.run_windows(
            variants, lambda name, f: timing.measure(f, a.calls, gpu, stream=True), a.windows).items()}
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(max(times[k]) - min(times[k]) for k in ("fused", "loop"))
        u = n * wb          # own, and out
        f32 = n * 4         # the loop's accumulator
        lst = nnz * wb      # the nonzero lists (scratch rows: written by the dense decode, read by the expansion)
        lines_per = 128 // 4
        for name in variants:
            lines.append({
                "shape": "1x15M", "dtype": str(dtype).split(".")[-1], "K": K, "zeros": zeros, "zero_run": run,
                "variant": name, **timing.summary(times[name], "us"), "vs_loop": round(med[name] / med["loop"], 4),
                "ratio": round(comp_bytes / (K * u), 4), "nonzeros": nnz,
                # bytes the algorithm moves.  Both: per source the archive and its list written and read
                # (C + 2 L).  fused: own and out once (K above the kernel's source limit: an fp32 partial
                # written and read between passes, not counted).  loop: own -> acc, per peer the accumulator's
                # words under set bits read and written (its 128 B lines: `lines_per` words each, far more),
                # acc -> out
                "bytes": comp_bytes + 2 * lst + 2 * u + ((2 * f32 + 2 * 4 * nnz) if name == "loop" else 0),
                "acc_line_share": round(1 - zeros ** (lines_per if run == 1 else 1), 4),
                "worthwhile": bool(med["loop"] - med["fused"] > spread) if name == "fused" else None,
                "scratch_bytes": need, "windows": a.windows, "calls_per_window": a.calls,
                "device": torch.cuda.get_device_name(0)})
        del own, out, acc, sources, result, ws
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
