"""What decode-and-accumulate saves: the fused call
(float_decompress_accumulate, k_decode's accumulate form) against what a
caller did before it -- float_decompress_pointer into a temporary, then
acc.add_(tmp), or acc.add_(tmp.float()) for an fp32 accumulator -- and the
plain decode for scale.  Cases: the c2 shape (256 x 524,288 bf16 words) and
one 64 MiB bf16 element, each with a bf16 (ACC 1) and an fp32 (ACC 2)
accumulator.

Times are device events around a window's calls; each figure is the median
over windows of the mean of a window's calls, with the min and max across
windows; the variants alternate inside every window, so drift hits all of
them alike.  The fused and the unfused result of one call on the same inputs
are compared bit for bit first.  Prints one JSON line per case and writes them
to --out.  Reads nothing outside the repository.

    usage: python tools/accumulate_bench.py [--out profiles/accumulate.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/accumulate.json")
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    gpu = timing.Gpu()
    ws = C.Workspace(256 << 20)
    lines = []
    for shape, (nb, n) in (("c2_256x524288", (256, 524288)), ("1x64MiB", (1, 32 << 20))):
        g = torch.Generator().manual_seed(nb)
        x = torch.randn(nb * n, generator=g).to(torch.bfloat16).to(dev).view(nb, n)
        arch2d, sizes = C.float_compress_stride(x, ws=ws)
        sizes_h = sizes.cpu().tolist()
        archives = [arch2d[i, : sizes_h[i]] for i in range(nb)]
        comp_bytes = sum(sizes_h)
        tmp = torch.empty_like(x)
        tmps = [tmp[i] for i in range(nb)]
        for mode, acc_dtype in ((1, torch.bfloat16), (2, torch.float32)):
            acc = torch.randn(nb, n, generator=torch.Generator().manual_seed(7)).to(acc_dtype).to(dev)
            accs = [acc[i] for i in range(nb)]

            def fused():
                C.float_decompress_accumulate(archives, accs, ft=2, ws=ws)

            def unfused():
                C.float_decompress_pointer(archives, tmps, ft=2, ws=ws)
                acc.add_(tmp if mode == 1 else tmp.float())

            def decode():
                C.float_decompress_pointer(archives, tmps, ft=2, ws=ws)

            # the two ways agree bit for bit on the same inputs
            start = acc.clone()
            fused()
            got = acc.clone()
            acc.copy_(start)
            unfused()
            torch.cuda.synchronize()
            it = torch.int16 if mode == 1 else torch.int32
            assert torch.equal(got.view(it), acc.view(it)), "fused and unfused results differ"
            acc.copy_(start)

            variants = {"fused": fused, "unfused": unfused, "decode": decode}
            times = {k: v["stream"] for k, v in timing.run_windows(
                variants, lambda name, f: timing.measure(f, a.calls, gpu, stream=True), a.windows).items()}
            u = nb * n * 2
            ub = nb * n * acc.element_size()
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) - min(v) for k, v in times.items() if k != "decode")
            for name in variants:
                lines.append({
                    "shape": shape, "dtype": "bf16", "acc": {1: "bf16", 2: "fp32"}[mode], "variant": name,
                    **timing.summary(times[name], "us"), "vs_unfused": round(med[name] / med["unfused"], 4),
                    "ratio": round(comp_bytes / u, 4),
                    # bytes the algorithm moves: archive C, decoded U, accumulator U' (unfused: the
                    # temporary is written and read, and tmp.float() writes and add_ reads a second one)
                    "bytes": {"fused": comp_bytes + 2 * ub,
                              "unfused": comp_bytes + 2 * u + 2 * ub + (2 * ub if mode == 2 else 0),
                              "decode": comp_bytes + u}[name],
                    "worthwhile": bool(med["unfused"] - med["fused"] > spread) if name == "fused" else None,
                    "windows": a.windows, "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
            del acc, accs
        del x, arch2d, tmp, tmps, archives
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
