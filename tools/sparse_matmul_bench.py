"""What a matmul on a sparse weight archive costs, bf16,
N(0, 1) magnitude-pruned to 50 % and 90 % zeros, R x row_words in {4096 x 4096,
8192 x 8192}, M in {1, 4, 16, 64}, four candidates alternating inside every
window on one device:

  (a) sparse    codec.matmul_sparse: the list decoded once, k_sparseMatmul +
                k_sparseMatmulFinish, no expanded matrix in memory
  (b) two-step  sparse_decompress into a reused [R, row_words] temporary, then
                torch.matmul(x, W.T): the path a user had before
  (c) dense-arc codec.matmul_rows (M <= 4) / codec.matmul_tile on a DENSE
                archive of the same pruned matrix
  (d) dense     torch.matmul alone on the uncompressed W: for information

Built like tools/matmul_rows_bench.py on tools/timing.py: device events around
a window's calls, the median over the windows with their min and max, every
candidate compared with the fp64 product first (that script's tolerances).
Each line carries the bytes of the sparse and of the dense archive.

    usage: python tools/sparse_matmul_bench.py [--out profiles/sparse_matmul_bench.json]
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
MS = (1, 4, 16, 64)
PATHS = ("sparse", "two_step", "dense_archive", "dense")


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/sparse_matmul_bench.json")
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
                out1, out3 = (torch.empty([M, R], dtype=torch.float32, device=dev) for _ in range(2))
                ok1, ok3 = (torch.empty([1], dtype=torch.uint8, device=dev) for _ in range(2))
                y2, y4 = (torch.empty([M, R], dtype=dt, device=dev) for _ in range(2))

                def f_sparse(x=x, out=out1, ok=ok1):
                    C.matmul_sparse(sparse, rw, x, dt, out=out, out_status=ok, ws=ws, nnz_bound=nnz)

                def f_two_step(x=x, y=y2):
                    C.sparse_decompress([sparse], [tmp.view(-1)], ws=ws)
                    torch.matmul(x, tmp.T, out=y)

                def f_dense_archive(x=x, out=out3, ok=ok3, M=M):
                    (C.matmul_rows if M <= 4 else C.matmul_tile)(dense_arc, rw, x, dt, out=out, out_status=ok, ws=ws)

                def f_dense(x=x, y=y4):
                    torch.matmul(x, W.T, out=y)

                fs = dict(zip(PATHS, (f_sparse, f_two_step, f_dense_archive, f_dense)))
                for f in fs.values():
                    f()
                torch.cuda.synchronize()
                assert int(ok1) == 1 and int(ok3) == 1 and torch.equal(tmp.view(torch.int16), W.view(torch.int16))
                xd, Wd = x.double(), W.double()
                ref, bound = xd @ Wd.T, rw * 2.0 ** -23 * (xd.abs() @ Wd.abs().T)
                for y in (out1, out3):
                    assert bool(((y.double() - ref).abs() <= bound).all()), (shape, zeros, M)
                for y in (y2, y4):  # torch's own order and bf16 rounding on top
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
                if meta[key]["path"] == "sparse":
                    stem = key[: -len("sparse")]
                    for other in PATHS[1:3]:
                        base = statistics.median(times[stem + other]["stream"])
                        line["sparse_vs_" + other] = round(statistics.median(times[key]["stream"]) / base, 4)
                lines.append(line)
            del cases, W, sp2d, sparse, de2d, dense_arc, tmp
            torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
