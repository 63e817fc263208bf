"""Argument checks of the row gather with device-resident indices that fire
before any device is touched, so they run without a GPU: the C ABI's
dietgpu_ans_gather_rows / dietgpu_float_gather_rows (csrc/capi.cpp),
torch.ops.dietgpu.gather_rows (csrc/torch_ops.cpp) and the Python wrapper
codec.gather_rows_device.  Every rejection is matched to its own message and
leaves the caller's tensors as they were.  tests/test_gpu_gather.py holds the
rejections that need device tensors."""
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMA = ("dietgpu::gather_rows(bool compress_as_float, Tensor t_in, int row_words, Tensor t_idx, Tensor t_out, "
          "Tensor? temp_mem=None, Tensor? out_status=None) -> int")


def test_the_operator_and_its_schema():
    assert str(D.gather_rows.default._schema) == SCHEMA
    assert ops.gather_rows is D.gather_rows
    # the twelve operators before it keep their list
    assert len(ops.OPS) == 12 and "gather_rows" not in ops.OPS and ops.MORE_OPS == ("gather_rows",)


def test_c_abi_is_declared():
    N.lib()
    assert "dietgpu_ans_gather_rows" in N.EXPORTED and "dietgpu_float_gather_rows" in N.EXPORTED


# ---------------------------------------------------------------- C ABI ----
# The flattened config and the row shape are checked before the stack or any
# pointer is looked at: every pointer here is null.

def float_call(ft=2, pb=10, rw=64, n=4, stride=64):
    rc = N.lib().dietgpu_float_gather_rows(None, ft, pb, None, rw, n, None, 0, None, stride, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


def ans_call(pb=10, rw=64, n=4, stride=64):
    rc = N.lib().dietgpu_ans_gather_rows(None, pb, None, rw, n, None, 1, None, stride, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


@pytest.mark.parametrize("call", [float_call, ans_call])
@pytest.mark.parametrize("pb", [0, 8, 12])
def test_c_abi_rejects_prob_bits(call, pb):
    rc, msg = call(pb=pb)
    assert rc == N.DIETGPU_ERR_INVALID and f"unhandled pdf precision {pb}" in msg


@pytest.mark.parametrize("call", [float_call, ans_call])
def test_c_abi_rejects_row_words_0(call):
    rc, msg = call(rw=0, stride=0)
    assert rc == N.DIETGPU_ERR_INVALID and "rowWords must be at least 1" in msg


@pytest.mark.parametrize("call", [float_call, ans_call])
@pytest.mark.parametrize("rw,stride", [(64, 63), (64, 0), (1, 0), (9000, 4096)])
def test_c_abi_rejects_a_stride_below_the_row(call, rw, stride):
    rc, msg = call(rw=rw, stride=stride)
    assert rc == N.DIETGPU_ERR_INVALID
    assert f"outRowStrideWords ({stride}) must be at least rowWords ({rw})" in msg


@pytest.mark.parametrize("ft", [0, 5, -1, 16])
def test_c_abi_rejects_a_float_type_out_of_range(ft):
    rc, msg = float_call(ft=ft)
    assert rc == N.DIETGPU_ERR_INVALID and "float_type must be 1..4" in msg


@pytest.mark.parametrize("call", [float_call, ans_call])
def test_c_abi_passes_good_arguments_on_to_the_next_check(call):
    for kw in ({}, {"pb": 9}, {"pb": 11}, {"rw": 1, "stride": 1}, {"rw": 64, "stride": 67}, {"n": 0}):
        rc, msg = call(**kw)
        assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg, kw
    if call is float_call:
        for ft in (1, 2, 3, 4):
            rc, msg = call(ft=ft)
            assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg


# ------------------------------------------------------------- operator ----
# CPU tensors throughout: the checks below come before any device check.

def arch():
    return torch.arange(64, dtype=torch.uint8)


def idx(dtype=torch.int64, shape=(4,)):
    return torch.zeros(shape, dtype=dtype)


def out(dtype=torch.bfloat16, shape=(4, 64)):
    return torch.full(shape, 3, dtype=dtype)


# name -> (as float, row_words, t_idx, t_out, message)
OP_REJECTS = {
    "row-words-0": (True, 0, idx, lambda: out(shape=(4, 0)), "row_words must be at least 1"),
    "row-words-negative": (True, -3, idx, out, "row_words must be at least 1"),
    "float-idx": (True, 64, lambda: idx(torch.float32), out, "t_idx must be int32 or int64"),
    "int16-idx": (True, 64, lambda: idx(torch.int16), out, "t_idx must be int32 or int64"),
    "bool-idx": (False, 64, lambda: idx(torch.bool), lambda: out(torch.uint8), "t_idx must be int32 or int64"),
    "cpu-idx-int64": (True, 64, idx, out, "t_idx must be a contiguous GPU tensor"),
    "cpu-idx-int32": (False, 64, lambda: idx(torch.int32), lambda: out(torch.uint8),
                      "t_idx must be a contiguous GPU tensor"),
    "int-out-in-float-mode": (True, 64, idx, lambda: out(torch.int16),
                              "float outputs must be float16, bfloat16, float32 or float64"),
    "byte-out-in-float-mode": (True, 64, idx, lambda: out(torch.uint8),
                               "float outputs must be float16, bfloat16, float32 or float64"),
    "float-out-in-byte-mode": (False, 64, idx, out, "t_out must be uint8 in byte mode"),
    "out-too-few-rows": (True, 64, idx, lambda: out(shape=(3, 64)), r"t_out must have the shape \[\*t_idx.shape, row_words\]"),
    "out-other-width": (True, 64, idx, lambda: out(shape=(4, 65)), r"t_out must have the shape"),
    "out-flat": (True, 64, idx, lambda: out(shape=(256,)), r"t_out must have the shape"),
    "out-extra-dim": (True, 64, idx, lambda: out(shape=(1, 4, 64)), r"t_out must have the shape"),
    "idx-2d-out-2d": (True, 64, lambda: idx(shape=(2, 2)), out, r"t_out must have the shape"),
    "out-last-dim-strided": (True, 64, idx, lambda: out(shape=(4, 128))[:, ::2],
                             "last dimension must be contiguous"),
    "out-rows-at-two-strides": (True, 64, lambda: idx(shape=(2, 2)), lambda: out(shape=(2, 3, 64))[:, :2],
                                "rows must lie at a constant stride"),
    "out-rows-overlap": (True, 64, idx, lambda: out(shape=(64,)).as_strided((4, 64), (0, 1)),
                         "rows must not overlap"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    as_float, rw, make_idx, make_out, msg = OP_REJECTS[case]
    a, i, o = arch(), make_idx(), make_out()
    keep = [t.clone() for t in (a, i, o)]
    with pytest.raises(RuntimeError, match=msg):
        D.gather_rows(as_float, a, rw, i, o)
    assert all(torch.equal(x, y) for x, y in zip((a, i, o), keep))


def test_python_wrapper_rejects_before_the_device():
    from dietgpu_fork_amd import codec as C

    a = arch()
    with pytest.raises(ValueError, match="idx must be a contiguous CUDA int32 or int64 tensor"):
        C.gather_rows_device(a, 64, idx(), torch.bfloat16)
    with pytest.raises(ValueError, match="idx must be a contiguous CUDA int32 or int64 tensor"):
        C.gather_rows_device(a, 64, [0, 1], torch.bfloat16)
    with pytest.raises(ValueError, match="idx must be a contiguous CUDA int32 or int64 tensor"):
        C.gather_rows_device(a, 64, idx(torch.float32), torch.bfloat16)
