"""What a matmul on a compressed weight table costs, bf16,
R x row_words in {4096 x 4096, 14336 x 4096, 8192 x 8192}, M in {1, 4, 8, 16,
32, 64}, four candidates alternating inside every window on one device:

  (a) fused     codec.matmul_rows: k_matmulRows + k_matmulFinish per 4 rows of
                x, no decoded matrix in memory
  (b) two-step  float_decompress into a preallocated [R, row_words] temporary,
                then torch.matmul(x, W.T): the path a user had before
  (c) dense     torch.matmul alone on an uncompressed W: for information, the
                price of keeping the weights compressed
  (d) tile      codec.matmul_tile: k_matmulTile +
                k_matmulFinish, every row of x in one pass through the matrix
                pipe

Device events around a window's calls; each figure is the median over the
windows with their min and max, which is the spread to read a difference
against.  The results are compared first, with the tolerance of
tests/test_gpu_matmul_rows.py (the two-step and dense products, rounded to
bf16 by torch, against the fp64 product within bf16's rounding on top).
Prints one JSON line per case and writes them to --out
(profiles/matmul_rows_bench.json holds the run before (d) existed,
profiles/matmul_tile_bench.json the one with it).

    usage: python tools/matmul_rows_bench.py [--out profiles/matmul_tile_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

SHAPES = ((4096, 4096), (14336, 4096), (8192, 8192))
MS = (1, 4, 8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/matmul_tile_bench.json")
    ap.add_argument("--shapes", default=",".join(f"{r}x{k}" for r, k in SHAPES))
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev, dt = "cuda", torch.bfloat16
    ws = C.Workspace(64 << 20)
    gpu = timing.Gpu()
    lines = []
    for shape in a.shapes.split(","):
        R, rw = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(R + rw)
        W = torch.randn([R, rw], generator=g).to(dt).to(dev)
        arch2d, sizes = C.float_compress_stride(W.view(1, -1), ws=ws)
        archive = arch2d[0, : int(sizes[0])]
        tmp = torch.empty_like(W)
        cases, meta = {}, {}
        for M in MS:
            x = torch.randn([M, rw], generator=g).to(dt).to(dev)
            out, out4 = (torch.empty([M, R], dtype=torch.float32, device=dev) for _ in range(2))
            ok = torch.empty([1], dtype=torch.uint8, device=dev)
            y2, y3 = (torch.empty([M, R], dtype=dt, device=dev) for _ in range(2))

            def fused(x=x, out=out, ok=ok):
                C.matmul_rows(archive, rw, x, dt, out=out, out_status=ok, ws=ws)

            def two_step(x=x, y=y2):
                C.float_decompress_pointer([archive], [tmp.view(-1)], ws=ws)
                torch.matmul(x, tmp.T, out=y)

            def dense(x=x, y=y3):
                torch.matmul(x, W.T, out=y)

            def tile(x=x, out=out4, ok=ok):
                C.matmul_tile(archive, rw, x, dt, out=out, out_status=ok, ws=ws)

            fused(), two_step(), dense(), tile()
            torch.cuda.synchronize()
            assert int(ok) == 1 and torch.equal(tmp.view(torch.int16), W.view(torch.int16))
            xd, Wd = x.double(), W.double()
            ref, mag = xd @ Wd.T, xd.abs() @ Wd.abs().T
            bound = rw * 2.0 ** -23 * mag
            for y in (out, out4):
                assert bool(((y.double() - ref).abs() <= bound).all()), (shape, M)
            for y in (y2, y3):  # torch's own order and bf16 rounding on top
                assert bool(((y.double() - ref).abs() <= 2 * bound + 2.0 ** -8 * ref.abs()).all()), (shape, M)
            for path, f in (("fused", fused), ("two_step", two_step), ("dense", dense), ("tile", tile)):
                key = f"bf16_{shape}_M{M}_{path}"
                cases[key] = (f, a.calls)
                meta[key] = {"dtype": "bf16", "rows": R, "row_words": rw, "M": M, "path": path,
                             "calls_per_window": a.calls}
        times = timing.run_windows(cases, lambda _, case: timing.measure(case[0], case[1], gpu, stream=True),
                                   a.windows)
        for key in cases:
            line = {"case": key, **meta[key], **timing.summary(times[key]["stream"], "stream_us"),
                    "windows": a.windows, "archive_bytes": int(sizes[0]), "dense_bytes": R * rw * 2,
                    "device": torch.cuda.get_device_name(0)}
            stem, path = key.rsplit("_", 1) if not key.endswith("_two_step") else (key[:-9], "two_step")
            if path in ("fused", "tile"):
                base = statistics.median(times[stem + "_two_step"]["stream"])
                line[path + "_vs_two_step"] = round(statistics.median(times[key]["stream"]) / base, 4)
            lines.append(line)
        del cases, W, arch2d, archive, tmp
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
