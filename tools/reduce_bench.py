"""What the fused multi-archive reduce saves: one
float_reduce call (k_reduce: K archives decoded side by side, the running sum
in registers) against the per-peer loop it replaces in dist.reduce_archives --
own.to(float32), one float_decompress_accumulate call per peer around an fp32
accumulator in HBM, acc.to(dtype).  Cases: bf16, K = 7 on 1 x 8 Mi words (a
shard of a 64 Mi-word all-reduce over 8 ranks); K = 3 and K = 7 on the c2
shape (256 x 524,288 bf16 words); fp32, K = 7, on 1 x 8 Mi words.

Times are device events around a window's calls; each figure is the median
over windows of the mean of a window's calls, with the min and max across
windows; the two variants alternate inside every window, so drift hits both
alike.  Both results of one call on the same inputs are compared bit for bit
first.  "worthwhile": the fused median lies below the loop's by more than the
spread between windows (the routing rule).  --candidates adds the fused call
with its launches capped at 3 and at 2 sources (the kernel's source-limit
candidates) to every window.  Prints one JSON line per case and variant and
writes them to --out.  Reads nothing outside the repository.

    usage: python tools/reduce_bench.py [--candidates] [--only N] [--out profiles/reduce.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

CASES = (("1x8Mi", torch.bfloat16, 1, 8 << 20, 7),
         ("c2_256x524288", torch.bfloat16, 256, 524288, 3),
         ("c2_256x524288", torch.bfloat16, 256, 524288, 7),
         ("1x8Mi", torch.float32, 1, 8 << 20, 7))


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/reduce.json")
    ap.add_argument("--only", type=int, default=None, help="run only case number N")
    ap.add_argument("--candidates", action="store_true",
                    help="also time the fused call capped at 3 and at 2 sources per launch")
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    gpu = timing.Gpu()
    ws = C.Workspace(512 << 20)
    lines = []
    for ci, (shape, dtype, nb, n, K) in enumerate(CASES):
        if a.only is not None and a.only != ci:
            continue
        ft = C.FLOAT_TYPE[dtype]
        wb = torch.empty(0, dtype=dtype).element_size()
        g = torch.Generator().manual_seed(nb + K)
        own = torch.randn(nb * n, generator=g).to(dtype).to(dev).view(nb, n)
        sources, comp_bytes = [], 0
        for k in range(K):
            x = torch.randn(nb * n, generator=g).to(dtype).to(dev).view(nb, n)
            arch2d, sizes = C.float_compress_stride(x, ws=ws)
            sizes_h = sizes.cpu().tolist()
            sources.append([arch2d[i, : sizes_h[i]] for i in range(nb)])
            comp_bytes += sum(sizes_h)
            del x
        out = torch.empty_like(own)
        outs, owns = [out[i] for i in range(nb)], [own[i] for i in range(nb)]
        acc = torch.empty(nb, n, dtype=torch.float32, device=dev)
        accs = [acc[i] for i in range(nb)]
        result = {}

        def fused():
            C.float_reduce(sources, outs, inits=owns, ft=ft, ws=ws)

        def loop():
            acc.copy_(own)  # own.to(float32)
            for row in sources:
                C.float_decompress_accumulate(row, accs, ft=ft, ws=ws)
            result["loop"] = acc.to(dtype)

        # the two ways agree bit for bit on the same inputs
        fused()
        loop()
        torch.cuda.synchronize()
        it = torch.int16 if wb == 2 else torch.int32
        assert torch.equal(out.view(it), result["loop"].view(it)), "fused and per-peer results differ"

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
        u = nb * n * wb       # own, and out
        f32 = nb * n * 4      # the loop's accumulator
        for name in variants:
            lines.append({
                "shape": shape, "dtype": str(dtype).split(".")[-1], "K": K, "variant": name,
                **timing.summary(times[name], "us"), "vs_loop": round(med[name] / med["loop"], 4),
                "ratio": round(comp_bytes / (K * u), 4),
                # bytes the algorithm moves.  fused: own, the archives, out (K above the kernel's
                # source limit: an fp32 partial written and read between passes, not counted).
                # loop: own -> acc, K x (archive + acc read and written), acc -> out
                "bytes": comp_bytes + 2 * u + ((2 + 2 * K) * f32 if name == "loop" else 0),
                "worthwhile": bool(med["loop"] - med["fused"] > spread) if name == "fused" else None,
                "windows": a.windows, "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
        del own, out, acc, sources, outs, owns, accs, result
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
