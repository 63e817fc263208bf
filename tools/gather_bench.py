"""What a row gather with device-resident indices costs: the
element and rows of tools/range_decode_bench.py -- one 64 MiB bf16 element,
1024 random rows of 1024 words -- through gather_rows_device (k_gather, the
indices already on the device), through the existing gather_rows (host
indices, one batched range decode) and against the full float_decompress; and
gather_rows_device on 16,384 rows of 64 and of 256 words, the embedding-sized
case.

Kernel times come from the library's event hook (profile_query of the
"decode_gather" / "decode_range" / "decode" families), call times from a host
clock around the call and a device synchronise.  Each figure is the median
over windows of the mean of a window's calls; the cases alternate inside every
window, so drift hits all of them alike.  Prints one JSON line per case and
writes them to --out.

    usage: python tools/gather_bench.py [--out profiles/gather.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gather.json")
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()

    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec as C

    dev = "cuda"
    bf16 = torch.bfloat16
    n = a.mib * (1 << 20) // 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, generator=g).to(bf16).to(dev)
    ws = C.Workspace(256 << 20)
    arch2d, sizes = C.float_compress_stride(x.view(1, n), ws=ws)
    archive = arch2d[0, : int(sizes[0])]
    full_out = torch.empty([1, n], dtype=bf16, device=dev)

    cases = {"full": ("decode", lambda: C.float_decompress_stride(arch2d, n, bf16, ws=ws, out=full_out))}
    checks = []

    def device_case(row_words, n_rows, seed):
        rows = np.random.default_rng(seed).integers(0, n // row_words, n_rows)
        idx = torch.from_numpy(rows).to(dev)
        out = torch.empty([n_rows, row_words], dtype=bf16, device=dev)
        ok = torch.empty([n_rows], dtype=torch.uint8, device=dev)
        cases[f"gather_device_{n_rows}_rows_of_{row_words}"] = ("decode_gather", lambda: C.gather_rows_device(
            archive, row_words, idx, bf16, out=out, out_status=ok, ws=ws))
        checks.append((out, ok, row_words, idx))
        return rows

    rows = device_case(1024, 1024, 1).tolist()  # range_decode_bench.py's rows
    host_out = torch.empty([1024, 1024], dtype=bf16, device=dev)
    cases["gather_host_1024_rows_of_1024"] = ("decode_range", lambda: C.gather_rows(
        archive, 1024, rows, bf16, out=host_out, ws=ws))
    device_case(64, 16384, 2)
    device_case(256, 16384, 3)

    # correctness at the sizes timed
    for name, (_, f) in cases.items():
        f()
    torch.cuda.synchronize()
    xi = x.view(torch.int16)
    assert torch.equal(full_out.view(torch.int16).view(-1), xi)
    assert torch.equal(host_out.view(torch.int16), xi.view(-1, 1024)[rows])
    for out, ok, row_words, idx in checks:
        assert bool(ok.all())
        assert torch.equal(out.view(torch.int16), xi.view(-1, row_words)[idx])

    C.profile(True)
    kern = {k: [] for k in cases}
    call = {k: [] for k in cases}
    for w in range(a.windows + 1):  # window 0 is warm-up
        for name, (family, f) in cases.items():
            C.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms, launches = C.profile_query(family)
            assert launches == a.calls, (name, launches)
            if w:
                kern[name].append(1e3 * ms / a.calls)
                call[name].append(1e6 * dt / a.calls)
    C.profile(False)

    lines = []
    base = statistics.median(kern["full"])
    for name, (family, _) in cases.items():
        k = statistics.median(kern[name])
        lines.append({"case": name, "family": family, "element_mib": a.mib, "dtype": "bf16",
                      "kernel_us": round(k, 2), "kernel_us_min": round(min(kern[name]), 2),
                      "kernel_us_max": round(max(kern[name]), 2),
                      "call_us": round(statistics.median(call[name]), 2),
                      "call_us_min": round(min(call[name]), 2), "call_us_max": round(max(call[name]), 2),
                      "kernel_vs_full": round(k / base, 4), "windows": a.windows, "calls_per_window": a.calls,
                      "device": torch.cuda.get_device_name(0)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            print(json.dumps(ln))
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
