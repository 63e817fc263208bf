"""Argument checks of the sparse decode-and-accumulate that fire before any
device is touched, so they run without a GPU: codec.sparse_decompress_accumulate
and the C ABI's dietgpu_float_decompress_sparse_accumulate (csrc/capi.cpp).
Every rejection is matched on its message and leaves the caller's tensors as
they were.  tests/test_gpu_sparse_accumulate.py holds what needs a device."""
import os

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dietgpu_float_decompress_sparse_accumulate"


def arch():
    return torch.arange(64, dtype=torch.uint8)


def acc(dtype=torch.float32, n=16):
    return torch.arange(n, dtype=torch.float64).to(dtype)


# name -> (archives, accumulators, ft, message)
REJECTS = {
    "more-archives": (lambda: ([arch(), arch()], [acc()], None), "one entry per member"),
    "more-accumulators": (lambda: ([arch()], [acc(), acc()], None), "one entry per member"),
    "empty": (lambda: ([], [], None), "sparse_decompress_accumulate: empty batch"),
    "mixed-dtypes": (lambda: ([arch(), arch()], [acc(), acc(torch.float16)], None),
                     "sparse_decompress_accumulate: the accumulators must share a dtype"),
    "integer-accumulator": (lambda: ([arch()], [acc(torch.int32)], None),
                            "sparse_decompress_accumulate: unsupported accumulator dtype"),
    "byte-accumulator": (lambda: ([arch()], [acc(torch.uint8)], None),
                         "sparse_decompress_accumulate: unsupported accumulator dtype"),
    "strided-accumulator": (lambda: ([arch()], [acc(n=32)[::2]], None),
                            "sparse_decompress_accumulate: the accumulators must be contiguous"),
    "fp32-into-fp16": (lambda: ([arch()], [acc(torch.float16)], 3), "accumulator type 1 does not go with float type 3"),
    "fp64-into-fp32": (lambda: ([arch()], [acc(torch.float32)], 4), "accumulator type 3 does not go with float type 4"),
    "fp16-into-bf16": (lambda: ([arch()], [acc(torch.bfloat16)], 1), "accumulator type 2 does not go with float type 1"),
    "bf16-into-fp64": (lambda: ([arch()], [acc(torch.float64)], 2), "accumulator type 4 does not go with float type 2"),
    "fp32-into-fp64": (lambda: ([arch()], [acc(torch.float64)], 3), "accumulator type 4 does not go with float type 3"),
}


@pytest.mark.parametrize("case", REJECTS)
def test_wrapper_rejects_before_the_device(case):
    make, msg = REJECTS[case]
    ins, accs, ft = make()
    keep = [t.clone() for t in ins + accs]
    with pytest.raises(ValueError, match=msg):
        C.sparse_decompress_accumulate(ins, accs, ft=ft)
    assert all(torch.equal(a, b) for a, b in zip(ins + accs, keep))


def test_the_dense_wrapper_keeps_its_messages():
    """The two wrappers share their checks; each names itself."""
    with pytest.raises(ValueError, match="float_decompress_accumulate: empty batch"):
        C.float_decompress_accumulate([], [])
    with pytest.raises(ValueError, match="^sparse_decompress_accumulate: empty batch"):
        C.sparse_decompress_accumulate([], [])


# (float_type, acc_type) pairs the C ABI refuses; it checks them, and the
# prob bits, before it looks at the stack or any pointer
BAD_PAIRS = [(1, 2), (1, 4), (2, 1), (2, 4), (3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 3), (2, 0), (2, 5), (3, -1)]
GOOD_PAIRS = [(1, 1), (2, 2), (3, 3), (4, 4), (1, 3), (2, 3)]


def capi(ft, pb, acc_type):
    rc = getattr(N.lib(), NAME)(None, ft, pb, 1, None, None, None, acc_type, None, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


@pytest.mark.parametrize("ft,acc_type", BAD_PAIRS)
def test_c_abi_rejects_a_bad_pair(ft, acc_type):
    rc, msg = capi(ft, 10, acc_type)
    assert rc == N.DIETGPU_ERR_INVALID
    assert f"acc_type {acc_type} does not go with float_type {ft}" in msg


@pytest.mark.parametrize("ft", [0, 5, -1])
def test_c_abi_rejects_a_bad_float_type(ft):
    rc, msg = capi(ft, 10, 3)
    assert rc == N.DIETGPU_ERR_INVALID and "float_type must be 1..4" in msg


@pytest.mark.parametrize("pb", [0, 8, 12])
def test_c_abi_rejects_prob_bits(pb):
    rc, msg = capi(2, pb, 3)
    assert rc == N.DIETGPU_ERR_INVALID and f"unhandled pdf precision {pb}" in msg


@pytest.mark.parametrize("ft,acc_type", GOOD_PAIRS)
def test_c_abi_passes_a_good_pair_on_to_the_next_check(ft, acc_type):
    rc, msg = capi(ft, 10, acc_type)
    assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg


def test_entry_points_are_declared():
    assert hasattr(N.lib(), NAME) and NAME in N.EXPORTED
    # the argument order of dietgpu_float_decompress_accumulate
    assert getattr(N.lib(), NAME).argtypes == N.lib().dietgpu_float_decompress_accumulate.argtypes
    hdr = open(os.path.join(ROOT, "include", "dietgpu_c.h")).read()
    assert NAME in hdr
    cpp = open(os.path.join(ROOT, "include", "dietgpu", "GpuFloatCodec.h")).read()
    block = cpp.split("// Sparse decode-and-accumulate")[1].split("stream);")[0]
    assert "void floatDecompressSparseAccumulate(" in block and "-0.0" in block  # the deviation is stated
    hooks = open(os.path.join(ROOT, "include", "dietgpu_testhooks.h")).read()
    assert "dietgpu_test_sparse_accumulate_config" in hooks


def test_the_collectives_codec_has_the_three_methods_and_info():
    from dietgpu_fork_amd import dist as D

    for cls in (D.GpuFloatCodec, D.GpuSparseFloatCodec):
        for m in ("compress", "decompress", "accumulate", "info"):
            assert callable(getattr(cls, m))
    # a dense header is what GpuFloatCodec.info reads
    with pytest.raises(RuntimeError, match="not a dense float archive"):
        D.GpuFloatCodec().info(torch.zeros(64, dtype=torch.uint8))
    # a sparse header {n, 0, 0, 0}, an empty bitmap's 16 bytes, a dense bf16 header
    import numpy as np

    h = np.zeros(16 + 16 + 32, dtype=np.uint8)
    h[0:4] = np.frombuffer(np.uint32(100).tobytes(), dtype=np.uint8)
    h[32:36] = np.frombuffer(np.uint32(0xf00f0001).tobytes(), dtype=np.uint8)
    h[40] = 2
    assert D.GpuSparseFloatCodec().info(torch.from_numpy(h)) == (100, torch.bfloat16)
