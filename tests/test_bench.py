"""bench.py's command line: a plain run prints the headline line alone,
--full adds the per-kernel figures, --dump-outputs writes the last timed
step's outputs as .npy arrays (checked against the CPU oracle on the GPU,
and for masking / determinism on CPU tensors)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, WORDS = 3, 4097  # more than one tensor, an odd size: a few ms per step
DUMPED = ("compressed_sizes", "decoded_sizes", "decode_status", "archive_checksums", "decoded_checksums",
          "archive_head", "archive_sample", "decoded_sample")
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "ratio")
FULL_ONLY_KEYS = ("kernels", "roofline", "cpu_baseline", "decode_hbm", "extras")


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def _fake_outputs(fill):
    """CPU stand-ins for the step's buffers: 5 archives of 40 columns, the
    bytes past each archive's size set to `fill` (the compressor leaves them
    unwritten)."""
    g = torch.Generator().manual_seed(7)
    nb, cols, n = 5, 40, 33
    sizes = torch.tensor([40, 1, 17, 39, 8], dtype=torch.int32)
    comp = torch.randint(0, 256, (nb, cols), generator=g, dtype=torch.uint8)
    out = torch.randn(nb, n, generator=g).to(torch.bfloat16)
    ref = comp.clone()
    for i in range(nb):
        comp[i, int(sizes[i]):] = fill
        ref[i, int(sizes[i]):] = 0
    ok = torch.ones(nb, dtype=torch.uint8)
    osz = torch.full((nb,), n, dtype=torch.int32)
    return comp, sizes, out, ok, osz, ref


def test_dump_outputs_masks_unwritten_bytes_and_is_deterministic(tmp_path):
    got = []
    for k, fill in enumerate((0xAA, 0x55)):
        comp, sizes, out, ok, osz, ref = _fake_outputs(fill)
        d = tmp_path / f"d{k}"
        bench._dump_outputs(str(d), 0, 1, comp, sizes, out, ok, osz, sample=64)
        assert sorted(os.listdir(d)) == sorted(f"{n}.npy" for n in DUMPED)
        got.append({n: np.load(d / f"{n}.npy") for n in DUMPED})
    a, b = got
    for n in DUMPED:
        assert a[n].dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
    np.testing.assert_array_equal(a["compressed_sizes"], sizes.numpy())
    np.testing.assert_array_equal(a["archive_checksums"], ref.numpy().astype(np.int64).sum(axis=1))
    np.testing.assert_array_equal(a["decoded_checksums"],
                                  out.view(torch.int16).numpy().astype(np.int64).sum(axis=1))
    np.testing.assert_array_equal(a["archive_head"], ref.numpy())  # 40 columns < the head's cap
    assert a["archive_sample"].shape == a["decoded_sample"].shape == (64,)
    assert set(a["archive_sample"]) <= set(ref.numpy().ravel().astype(np.float32))
    assert set(a["decoded_sample"]) <= set(out.float().numpy().ravel())


def test_dump_outputs_names_the_rank_in_a_multi_gpu_run(tmp_path):
    comp, sizes, out, ok, osz, _ = _fake_outputs(0)
    bench._dump_outputs(str(tmp_path), 1, 2, comp, sizes, out, ok, osz, sample=8)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}.rank1.npy" for n in DUMPED)


def _run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(NB), "--words", str(WORDS), "--settle-ms", "1", *extra],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_the_oracles_archives(tmp_path):
    from oracle import oracle as O

    line = _run_bench("--dump-outputs", str(tmp_path))
    for k in HEADLINE_KEYS:
        assert k in line, k
    for k in FULL_ONLY_KEYS:
        assert k not in line, k
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (printed to 0.01 GB/s and 0.1 us)
    assert line["value"] == pytest.approx(NB * WORDS * 2 / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-2, abs=0.011)

    got = {n: np.load(tmp_path / f"{n}.npy") for n in DUMPED}
    # the bench's c2 input: N(0,1) fp32 from seed 0 on the device, truncated to bf16
    g = torch.Generator(device="cuda").manual_seed(0)
    x32 = torch.randn(NB, WORDS, generator=g, device="cuda", dtype=torch.float32)
    x = (x32.view(torch.int32) >> 16).to(torch.int16).cpu()
    refs = [O.float_compress(x[i].numpy().view(np.uint16), 2) for i in range(NB)]
    np.testing.assert_array_equal(got["compressed_sizes"], [r.size for r in refs])
    np.testing.assert_array_equal(got["archive_checksums"], [int(r.astype(np.int64).sum()) for r in refs])
    for i, r in enumerate(refs):
        m = min(r.size, got["archive_head"].shape[1])
        np.testing.assert_array_equal(got["archive_head"][i, :m], r[:m])
        assert not got["archive_head"][i, m:].any()
    assert line["ratio"] == pytest.approx(sum(r.size for r in refs) / (NB * WORDS * 2), abs=1e-5)
    np.testing.assert_array_equal(got["decode_status"], np.ones(NB))
    np.testing.assert_array_equal(got["decoded_sizes"], np.full(NB, WORDS))
    np.testing.assert_array_equal(got["decoded_checksums"], x.to(torch.int64).sum(dim=1).numpy())
    assert set(got["decoded_sample"]) <= set(x.view(torch.bfloat16).float().numpy().ravel())


@pytest.mark.gpu
def test_full_run_adds_the_kernel_figures():
    line = _run_bench("--full", "--no-extras", "--no-cpu-baseline")
    for k in HEADLINE_KEYS + ("kernels", "roofline", "decode_hbm"):
        assert k in line, k
    assert line["steps"] == 3 and line["kernels"] and line["roofline"]["peak"] == bench.HBM_PEAK_GBPS
