"""What a matmul on a sparse weight archive costs through the matrix pipe
(DESIGN.md 5.2o), on 5.2m's four tables: bf16, N(0, 1) magnitude-pruned to 50 %
and 90 % zeros, R x row_words in {4096 x 4096, 8192 x 8192}, M in {4, 8, 16,
64}, four candidates alternating inside every window on one device:

  (a) sparse_tile  codec.matmul_sparse_tile: one pass over the decoded list,
                   k_sparseMatmulTile + k_sparseMatmulTileFinish
  (b) sparse       codec.matmul_sparse: one pass per eight rows of x
  (c) two_step     sparse_decompress into a reused [R, row_words] temporary,
                   then torch.matmul(x, W.T)
  (d) dense_tile   codec.matmul_tile on a DENSE archive of the same matrix

Built like tools/sparse_matmul_bench.py on tools/timing.py: device events
around a window's calls, the median over the windows with their min and max,
every candidate compared with the fp64 product first.  Every sparse_tile line
carries its ratio to the other three, and `beats_sparse`: whether its median
lies below matmul_sparse's by more than the spread (max - min) of
matmul_sparse's windows (5.2j's rule).

    usage: python tools/sparse_matmul_tile_bench.py [--out profiles/sparse_matmul_tile_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

SHAPES = ((4096, 4096), (8192, 8192))
ZEROS = (0.5, 0.9)
MS = (4, 8, 16, 64)
PATHS = ("sparse_tile", "sparse", "two_step", "dense_tile")


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/sparse_matmul_tile_bench.json")
    ap.add_argument("--shapes", default=",".join(f"{r}x{k}" for r, k in SHAPES))
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev, dt = "cuda", torch.bfloat16
    ws = C.Workspace(1 << 30)
    gpu = timing.Gpu()
    lines = []
    for shape in a.shapes.split(","):
        R, rw = (int(v) for v in shape.split("x"))
        for zeros in ZEROS:
            g = torch.Generator().manual_seed(R + rw)
            W = torch.randn([R, rw], generator=g).to(dev)
            W[W.abs() <= W.abs().flatten().kthvalue(int(zeros * R * rw)).values] = 0
            W = W.to(dt)
            sp2d, sp_size = C.sparse_compress([W.view(-1)], ws=ws)
            sparse = sp2d[0, : int(sp_size[0])]
            de2d, de_size = C.float_compress_stride(W.view(1, -1), ws=ws)
            dense_arc = de2d[0, : int(de_size[0])]
            nnz = C._sparse_sizes(sparse)[1]
            tmp = torch.empty_like(W)
            cases, meta = {}, {}
            for M in MS:
                x = torch.randn([M, rw], generator=g).to(dt).to(dev)
                outs = [torch.empty([M, R], dtype=torch.float32, device=dev) for _ in range(3)]
                oks = [torch.empty([1], dtype=torch.uint8, device=dev) for _ in range(3)]
                y = torch.empty([M, R], dtype=dt, device=dev)

                def f_sparse_tile(x=x, out=outs[0], ok=oks[0]):
                    C.matmul_sparse_tile(sparse, rw, x, dt, out=out, out_status=ok, ws=ws, nnz_bound=nnz)

                def f_sparse(x=x, out=outs[1], ok=oks[1]):
                    C.matmul_sparse(sparse, rw, x, dt, out=out, out_status=ok, ws=ws, nnz_bound=nnz)

                def f_two_step(x=x, y=y):
                    C.sparse_decompress([sparse], [tmp.view(-1)], ws=ws)
                    torch.matmul(x, tmp.T, out=y)

                def f_dense_tile(x=x, out=outs[2], ok=oks[2]):
                    C.matmul_tile(dense_arc, rw, x, dt, out=out, out_status=ok, ws=ws)

                fs = dict(zip(PATHS, (f_sparse_tile, f_sparse, f_two_step, f_dense_tile)))
                for f in fs.values():
                    f()
                torch.cuda.synchronize()
                assert all(int(ok) == 1 for ok in oks) and torch.equal(tmp.view(torch.int16), W.view(torch.int16))
                xd, Wd = x.double(), W.double()
                ref, bound = xd @ Wd.T, rw * 2.0 ** -23 * (xd.abs() @ Wd.abs().T)
                for out in outs:
                    assert bool(((out.double() - ref).abs() <= bound).all()), (shape, zeros, M)
                # torch's own order and bf16 rounding on top
                assert bool(((y.double() - ref).abs() <= 2 * bound + 2.0 ** -8 * ref.abs()).all()), (shape, M)
                for path, f in fs.items():
                    key = f"bf16_{shape}_z{int(100 * zeros)}_M{M}_{path}"
                    cases[key] = (f, a.calls)
                    meta[key] = {"dtype": "bf16", "rows": R, "row_words": rw, "zeros": zeros, "M": M, "path": path,
                                 "calls_per_window": a.calls}
            times = timing.run_windows(cases, lambda _, case: timing.measure(case[0], case[1], gpu, stream=True),
                                       a.windows)
            for key in cases:
                line = {"case": key, **meta[key], **timing.summary(times[key]["stream"], "stream_us"),
                        "windows": a.windows, "sparse_archive_bytes": int(sp_size[0]),
                        "dense_archive_bytes": int(de_size[0]), "raw_bytes": R * rw * 2, "list_words": nnz,
                        "device": torch.cuda.get_device_name(0)}
                if meta[key]["path"] == "sparse_tile":
                    stem, mine = key[: -len("sparse_tile")], statistics.median(times[key]["stream"])
                    for other in PATHS[1:]:
                        line["sparse_tile_vs_" + other] = round(
                            mine / statistics.median(times[stem + other]["stream"]), 4)
                    old = times[stem + "sparse"]["stream"]
                    line["beats_sparse"] = bool(statistics.median(old) - mine > max(old) - min(old))
                lines.append(line)
            del cases, W, sp2d, sparse, de2d, dense_arc, tmp
            torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)
    lost = [ln["case"] for ln in lines if ln["M"] == 64 and ln.get("beats_sparse") is False]
    assert not lost, f"at M = 64 matmul_sparse_tile must beat matmul_sparse beyond its spread: {lost}"


if __name__ == "__main__":
    main()
