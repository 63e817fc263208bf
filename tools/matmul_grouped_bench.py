"""What a mixture-of-experts layer on compressed expert tables costs (DESIGN.md
5.2l), bf16, E = 64 experts of R x row_words in {2048 x 4096, 4096 x 4096},
three routings (active experts x rows each: 8 x 1, 8 x 8, 32 x 4), three
candidates alternating inside every window on one device:

  (a) grouped   codec.matmul_grouped: one call, the routing read on the device
  (b) loop      codec.matmul_tile per active expert, the routing known to the
                host in advance (which flatters it: a real caller reads it back)
  (c) two-step  per active expert, float_decompress into one reused temporary,
                then torch.matmul

Device events around a window's calls; each figure is the median over the
windows with their min and max, which is the spread to read a difference
against.  The results are compared with the fp64 product first, with the
tolerance of tests/test_gpu_matmul_rows.py.  Prints one JSON line per case and
writes them to --out.

    usage: python tools/matmul_grouped_bench.py [--out profiles/matmul_grouped_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timing  # noqa: E402  (tools/timing.py, next to this script)

SHAPES = ((2048, 4096), (4096, 4096))
ROUTINGS = ((8, 1), (8, 8), (32, 4))
E = 64


def main():
    ap = argparse.ArgumentParser()
    timing.add_args(ap, "profiles/matmul_grouped_bench.json")
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
        # four distinct tables, dealt round-robin to the 64 experts (each expert its own archive copy)
        Ws = [torch.randn([R, rw], generator=g).to(dt).to(dev) for _ in range(4)]
        archives = []
        for e in range(E):
            arch2d, sizes = C.float_compress_stride(Ws[e % 4].view(1, -1), ws=ws)
            archives.append(arch2d[0, : int(sizes[0])].clone())
        ptrs = C.archive_ptrs(archives)
        tmp = torch.empty_like(Ws[0])
        cases, meta = {}, {}
        for active, rows in ROUTINGS:
            T = active * rows
            chosen = [(e * E) // active for e in range(active)]  # spread over the experts
            counts = [rows if e in chosen else 0 for e in range(E)]
            offs = torch.tensor([0] + [sum(counts[: e + 1]) for e in range(E)], dtype=torch.int64, device=dev)
            x = torch.randn([T, rw], generator=g).to(dt).to(dev)
            out_a, out_b = (torch.zeros([T, R], dtype=torch.float32, device=dev) for _ in range(2))
            out_c = torch.zeros([T, R], dtype=dt, device=dev)
            ok, ok1 = torch.empty([E], dtype=torch.uint8, device=dev), torch.empty([1], dtype=torch.uint8, device=dev)

            def grouped(x=x, offs=offs, out=out_a):
                C.matmul_grouped(ptrs, rw, x, offs, dt, out=out, out_status=ok, ws=ws)

            def loop(x=x, out=out_b, chosen=chosen, rows=rows):
                for i, e in enumerate(chosen):
                    C.matmul_tile(archives[e], rw, x[i * rows:(i + 1) * rows], dt, out=out[i * rows:(i + 1) * rows],
                                  out_status=ok1, ws=ws)

            def two_step(x=x, out=out_c, chosen=chosen, rows=rows):
                for i, e in enumerate(chosen):
                    C.float_decompress_pointer([archives[e]], [tmp.view(-1)], ws=ws)
                    torch.matmul(x[i * rows:(i + 1) * rows], tmp.T, out=out[i * rows:(i + 1) * rows])

            grouped(), loop(), two_step()
            torch.cuda.synchronize()
            assert bool(ok.all()) and torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
            for i, e in enumerate(chosen):
                xd, Wd = x[i * rows:(i + 1) * rows].double(), Ws[e % 4].double()
                ref, bound = xd @ Wd.T, rw * 2.0 ** -23 * (xd.abs() @ Wd.abs().T)
                assert bool(((out_a[i * rows:(i + 1) * rows].double() - ref).abs() <= bound).all()), (shape, e)
                err_c = (out_c[i * rows:(i + 1) * rows].double() - ref).abs()
                assert bool((err_c <= 2 * bound + 2.0 ** -8 * ref.abs()).all()), (shape, e)
            for path, f in (("grouped", grouped), ("loop", loop), ("two_step", two_step)):
                key = f"bf16_{shape}_{active}x{rows}_{path}"
                cases[key] = (f, a.calls)
                meta[key] = {"dtype": "bf16", "experts": E, "rows": R, "row_words": rw, "active": active,
                             "rows_each": rows, "path": path, "calls_per_window": a.calls}
        times = timing.run_windows(cases, lambda _, case: timing.measure(case[0], case[1], gpu, stream=True),
                                   a.windows)
        for key in cases:
            line = {"case": key, **meta[key], **timing.summary(times[key]["stream"], "stream_us"),
                    "windows": a.windows, "device": torch.cuda.get_device_name(0)}
            if meta[key]["path"] == "grouped":
                stem = key[: -len("grouped")]
                for other in ("loop", "two_step"):
                    base = statistics.median(times[stem + other]["stream"])
                    line["grouped_vs_" + other] = round(statistics.median(times[key]["stream"]) / base, 4)
            lines.append(line)
        del cases, Ws, archives, ptrs, tmp
        torch.cuda.empty_cache()
    timing.write_lines(lines, a.out)


if __name__ == "__main__":
    main()
