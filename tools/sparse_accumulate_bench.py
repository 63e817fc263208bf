"""What the sparse decode-and-accumulate saves: the fused call
(sparse_decompress_accumulate, k_sparseExpand's accumulate form) against what
a caller did before it -- sparse_decompress into a temporary, then
acc.add_(tmp), or acc.add_(tmp.float()) for an fp32 accumulator -- and the
plain sparse_decompress for scale.  Shapes: the sparse points of the README,
1 x 15 M and 5 x 15 M fp32 at 90 % zeros, 5 x 15 M fp32 at 50 % zeros, and
5 x 15 M bf16 at 90 % zeros into bf16 and into fp32 accumulators, the zeros
at uniformly random word positions; and 5 x 15 M fp32 and bf16 into fp32 with
90 % of the 1000-word rows zero as a whole.

Times are device events around a window's calls; each figure is the median
over windows of the mean of a window's calls, with the min and max across
windows; the variants alternate inside every window, so drift hits all of
them alike.  The fused and the unfused result of one call on the same inputs
are compared bit for bit first (the accumulators hold no -0.0 and no NaN, so
skipping a zero word and adding +0.0 agree).  Prints one JSON line per
variant and writes them to --out.  Reads nothing outside the repository.

    usage: python tools/sparse_accumulate_bench.py [--out profiles/sparse_accumulate.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

N15M = 15 * 1000 * 1000
# (shape name, elements, words each, dtype, fraction of zeros, accumulator dtypes, run): zeros fall
# on runs of `run` consecutive words, 1 = word by word
SHAPES = (
    ("1x15M", 1, N15M, torch.float32, 0.9, (torch.float32,), 1),
    ("5x15M", 5, N15M, torch.float32, 0.9, (torch.float32,), 1),
    ("5x15M", 5, N15M, torch.float32, 0.5, (torch.float32,), 1),
    ("5x15M", 5, N15M, torch.bfloat16, 0.9, (torch.bfloat16, torch.float32), 1),
    # structured sparsity (untouched rows of an embedding or expert gradient): whole 1000-word rows zero
    ("5x15M rows of 1000", 5, N15M, torch.float32, 0.9, (torch.float32,), 1000),
    ("5x15M rows of 1000", 5, N15M, torch.bfloat16, 0.9, (torch.float32,), 1000),
)
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/sparse_accumulate.json")
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    gpu = timing.Gpu()
    ws = C.Workspace(2 << 30)
    lines = []
    for shape, nb, n, dtype, zeros, acc_dtypes, run in SHAPES:
        g = torch.Generator(device=dev).manual_seed(nb)
        x = torch.randn(nb, n, generator=g, device=dev).to(dtype)
        x[x == 0] = 1  # (bf16 rounds no N(0,1) draw to zero in practice; the zeros are the mask's)
        x.view(nb, n // run, run)[torch.rand(nb, n // run, generator=g, device=dev) < zeros] = 0
        nnz = int((x != 0).sum())
        ft = C.FLOAT_TYPE[dtype]
        arch2d, sizes = C.sparse_compress([x[i] for i in range(nb)], ft=ft, ws=ws)
        sizes_h = sizes.cpu().tolist()
        archives = [arch2d[i, : sizes_h[i]] for i in range(nb)]
        comp_bytes = sum(sizes_h)
        tmp = torch.empty_like(x)
        tmps = [tmp[i] for i in range(nb)]
        for acc_dtype in acc_dtypes:
            wide = acc_dtype != dtype
            acc = torch.randn(nb, n, generator=torch.Generator().manual_seed(7)).to(acc_dtype)
            acc[acc == 0] = 1  # no -0.0, so that the two variants agree bit for bit
            acc = acc.to(dev)
            accs = [acc[i] for i in range(nb)]

            def fused():
                C.sparse_decompress_accumulate(archives, accs, ft=ft, ws=ws)

            def unfused():
                C.sparse_decompress(archives, tmps, ft=ft, ws=ws)
                acc.add_(tmp.float() if wide else tmp)

            def decode():
                C.sparse_decompress(archives, tmps, ft=ft, ws=ws)

            start = acc.clone()
            fused()
            got = acc.clone()
            acc.copy_(start)
            unfused()
            torch.cuda.synchronize()
            it = {2: torch.int16, 4: torch.int32}[acc.element_size()]
            assert torch.equal(got.view(it), acc.view(it)), "fused and unfused results differ"
            acc.copy_(start)
            del got

            variants = {"fused": fused, "unfused": unfused, "decode": decode}
            times = {k: v["stream"] for k, v in timing.run_windows(
                variants, lambda name, f: timing.measure(f, a.calls, gpu, stream=True), a.windows).items()}
            wb, ab = x.element_size(), acc.element_size()
            u = nb * n * wb           # the decoded elements
            ub = nb * n * ab          # the accumulators
            lst = nnz * wb            # the nonzero lists (scratch rows: written by the dense decode, read by the expansion)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) - min(v) for k, v in times.items() if k != "decode")
            for name in variants:
                lines.append({
                    "shape": shape, "dtype": NAME[dtype], "zeros": zeros, "zero_run": run, "acc": NAME[acc_dtype],
                    "variant": name,
                    **timing.summary(times[name], "us"), "vs_unfused": round(med[name] / med["unfused"], 4),
                    "ratio": round(comp_bytes / u, 4), "nonzero": round(nnz / (nb * n), 4),
                    # bytes the algorithm moves: archive C (its bitmap is read twice: counted, then
                    # expanded), list L written and read; fused: the accumulator words under nonzero
                    # words read and written; unfused: the temporary U written and read, the accumulator
                    # U' read and written, and for an fp32 accumulator tmp.float() writes and add_ reads U'
                    "bytes": {"fused": comp_bytes + 2 * lst + 2 * nnz * ab,
                              "unfused": comp_bytes + 2 * lst + 2 * u + 2 * ub + (2 * ub if wide else 0),
                              "decode": comp_bytes + 2 * lst + u}[name],
                    "worthwhile": bool(med["unfused"] - med["fused"] > spread) if name == "fused" else None,
                    "windows": a.windows, "calls_per_window": a.calls, "device": torch.cuda.get_device_name(0)})
            del acc, accs, start
        del x, arch2d, tmp, tmps, archives
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
