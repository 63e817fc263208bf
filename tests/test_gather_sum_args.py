"""Argument checks of the pooled row gather that fire before
any device is touched, so they run without a GPU: the C ABI's
dietgpu_float_gather_rows_sum (csrc/capi.cpp), torch.ops.dietgpu.gather_rows_sum
(csrc/torch_ops.cpp) and the Python wrapper codec.gather_rows_sum.  Every
rejection is matched to its own message and leaves the caller's tensors as they
were.  tests/test_gpu_gather_sum.py holds the rejections that need device
tensors (and the C++ entry point's, through the test hook)."""
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMA = ("dietgpu::gather_rows_sum(Tensor t_in, int row_words, Tensor t_idx, Tensor t_offsets, Tensor t_out, "
          "Tensor? temp_mem=None, Tensor? out_status=None) -> int")


def test_the_operator_and_its_schema():
    assert str(D.gather_rows_sum.default._schema) == SCHEMA
    assert ops.POOL_OPS == ("gather_rows_sum",) and ops.gather_rows_sum is D.gather_rows_sum
    # the operators before it keep their lists
    assert len(ops.OPS) == 12 and ops.MORE_OPS == ("gather_rows",) and ops.REDUCE_OPS == ("reduce_data",)


def test_c_abi_is_declared():
    N.lib()
    assert "dietgpu_float_gather_rows_sum" in N.EXPORTED and hasattr(N.lib(), "dietgpu_float_gather_rows_sum")


# ---------------------------------------------------------------- C ABI ----
# The flattened config and the shape are checked before the stack or any
# pointer is looked at: every pointer here is null.

def c_call(ft=2, pb=10, rw=64, bags=4, n=9, out32=0, stride=64):
    rc = N.lib().dietgpu_float_gather_rows_sum(None, ft, pb, None, rw, bags, n, None, None, 1, None, out32, stride,
                                               None, None)
    return rc, N.lib().dietgpu_last_error().decode()


@pytest.mark.parametrize("pb", [0, 8, 12])
def test_c_abi_rejects_prob_bits(pb):
    rc, msg = c_call(pb=pb)
    assert rc == N.DIETGPU_ERR_INVALID and f"unhandled pdf precision {pb}" in msg


def test_c_abi_rejects_row_words_0():
    rc, msg = c_call(rw=0, stride=0)
    assert rc == N.DIETGPU_ERR_INVALID and "rowWords must be at least 1" in msg


@pytest.mark.parametrize("rw,stride", [(64, 63), (64, 0), (1, 0), (4097, 4096)])
def test_c_abi_rejects_a_stride_below_the_row(rw, stride):
    rc, msg = c_call(rw=rw, stride=stride)
    assert rc == N.DIETGPU_ERR_INVALID
    assert f"outRowStrideWords ({stride}) must be at least rowWords ({rw})" in msg


@pytest.mark.parametrize("ft", [0, 5, -1, 16])
def test_c_abi_rejects_a_float_type_out_of_range(ft):
    # (0 would be a byte archive: there is no byte form of this call)
    rc, msg = c_call(ft=ft)
    assert rc == N.DIETGPU_ERR_INVALID and "float_type must be 1..4" in msg


def test_c_abi_rejects_fp64_archives():
    for out32 in (0, 1):
        rc, msg = c_call(ft=4, out32=out32)
        assert rc == N.DIETGPU_ERR_INVALID
        assert "a pooled row gather takes fp16, bf16 or fp32 archives (float type 1..3), not 4" in msg


def test_c_abi_rejects_a_16_bit_out_of_an_fp32_archive():
    rc, msg = c_call(ft=3, out32=0)
    assert rc == N.DIETGPU_ERR_INVALID and "the pooled rows of an fp32 archive are fp32" in msg


def test_c_abi_passes_good_arguments_on_to_the_next_check():
    for kw in ({}, {"pb": 9}, {"pb": 11}, {"rw": 1, "stride": 1}, {"stride": 67}, {"bags": 0}, {"n": 0},
               {"ft": 1}, {"ft": 1, "out32": 1}, {"out32": 1}, {"ft": 3, "out32": 1}):
        rc, msg = c_call(**kw)
        assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg, kw


# ------------------------------------------------- the C++ entry point ----
# floatGatherRowsSum's own refusals -- a config with useChecksum set, which no
# layer above can express, and the types the C ABI refuses itself -- through
# the test hook, over an empty stack: they come before any pointer is looked at.

def hook_call(ft, checksum, out32, rw=64, bags=2, n=3):
    T = N.testlib()
    stack = N.Stack(0)
    rc = T.dietgpu_test_gather_sum_config(stack.h, ft, checksum, None, rw, bags, n, None, None, None, out32, None,
                                          None)
    return rc, T.dietgpu_test_last_error().decode()


def test_the_hook_is_declared():
    N.testlib()
    assert "dietgpu_test_gather_sum_config" in N.TEST_EXPORTED


@pytest.mark.parametrize("ft,out32", [(1, 0), (1, 1), (2, 0), (2, 1), (3, 1)])
def test_entry_point_rejects_a_checksum_config(ft, out32):
    rc, msg = hook_call(ft, 1, out32)
    assert rc == N.DIETGPU_ERR_INVALID
    assert "a pooled row gather cannot verify a checksum (the decoded words are never stored)" in msg


def test_entry_point_rejects_types_shapes_and_task_counts():
    for args, want in (((4, 0, 1), "takes fp16, bf16 or fp32 archives (float type 1..3), not 4"),
                       ((3, 0, 0), "the pooled rows of an fp32 archive are fp32"),
                       ((2, 0, 0, 0), "rowWords must be at least 1"),
                       ((2, 0, 0, 129, 1 << 31), "too many bags: numBags (2147483648) times the 2 column tiles"),
                       ((2, 0, 0, 64, 2), "must not be null")):  # a good call reaches the pointer check
        rc, msg = hook_call(*args)
        assert rc == N.DIETGPU_ERR_INVALID and want in msg, (args, msg)
    # no bags: nothing to do, before any pointer is looked at
    assert hook_call(2, 0, 0, 64, 0, 0)[0] == N.DIETGPU_OK


# ------------------------------------------------------------- operator ----
# CPU tensors throughout: the checks below come before any device check.

def arch():
    return torch.arange(64, dtype=torch.uint8)


def idx(dtype=torch.int64, n=9):
    return torch.zeros([n], dtype=dtype)


def offs(dtype=torch.int64, n=5):
    return torch.zeros([n], dtype=dtype)


def out(dtype=torch.bfloat16, shape=(4, 64)):
    return torch.full(shape, 3, dtype=dtype)


# name -> (row_words, t_idx, t_offsets, t_out, message)
OP_REJECTS = {
    "row-words-0": (0, idx, offs, lambda: out(shape=(4, 0)), "row_words must be at least 1"),
    "row-words-negative": (-3, idx, offs, out, "row_words must be at least 1"),
    "float-idx": (64, lambda: idx(torch.float32), lambda: offs(torch.float32), out, "t_idx must be int32 or int64"),
    "int16-idx": (64, lambda: idx(torch.int16), lambda: offs(torch.int16), out, "t_idx must be int32 or int64"),
    "idx-64-offsets-32": (64, idx, lambda: offs(torch.int32), out, "t_offsets must have t_idx's dtype"),
    "idx-32-offsets-64": (64, lambda: idx(torch.int32), offs, out, "t_offsets must have t_idx's dtype"),
    "no-offsets": (64, idx, lambda: offs(n=0), lambda: out(shape=(0, 64)), "t_offsets with B \\+ 1 >= 1 entries"),
    "offsets-2d": (64, idx, lambda: offs().reshape(5, 1), out, "t_idx and t_offsets must be 1-d"),
    "idx-2d": (64, lambda: idx().reshape(3, 3), offs, out, "t_idx and t_offsets must be 1-d"),
    "fp64-out": (64, idx, offs, lambda: out(torch.float64), "t_out must be float16, bfloat16 or float32"),
    "byte-out": (64, idx, offs, lambda: out(torch.uint8), "t_out must be float16, bfloat16 or float32"),
    "int-out": (64, idx, offs, lambda: out(torch.int16), "t_out must be float16, bfloat16 or float32"),
    "out-too-few-rows": (64, idx, offs, lambda: out(shape=(3, 64)),
                         r"t_out must have the shape \[t_offsets.numel\(\) - 1, row_words\] = \[4, 64\]"),
    "out-other-width": (64, idx, offs, lambda: out(shape=(4, 65)), "t_out must have the shape"),
    "out-flat": (64, idx, offs, lambda: out(shape=(256,)), "t_out must have the shape"),
    "out-last-dim-strided": (64, idx, offs, lambda: out(shape=(4, 128))[:, ::2], "last dimension must be contiguous"),
    "out-rows-overlap": (64, idx, offs, lambda: out(shape=(64,)).as_strided((4, 64), (0, 1)),
                         "rows must not overlap"),
    "out-rows-too-close": (64, idx, offs, lambda: out(shape=(512,)).as_strided((4, 64), (63, 1)),
                           "rows must not overlap"),
    "cpu-idx": (64, idx, offs, out, "t_idx and t_offsets must be contiguous GPU tensors"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    rw, make_idx, make_offs, make_out, msg = OP_REJECTS[case]
    a, i, f, o = arch(), make_idx(), make_offs(), make_out()
    keep = [t.clone() for t in (a, i, f, o)]
    with pytest.raises(RuntimeError, match=msg):
        D.gather_rows_sum(a, rw, i, f, o)
    assert all(torch.equal(x, y) for x, y in zip((a, i, f, o), keep))


# -------------------------------------------------------- Python wrapper ----

WRAPPER_REJECTS = {
    "idx-list": (dict(idx=[0, 1]), "idx must be a contiguous 1-d int32 or int64 tensor"),
    "idx-float": (dict(idx=idx(torch.float32)), "idx must be a contiguous 1-d int32 or int64 tensor"),
    "offsets-2d": (dict(offsets=offs().reshape(5, 1)), "offsets must be a contiguous 1-d int32 or int64 tensor"),
    "mixed-32-64": (dict(idx=idx(torch.int32)), "idx and offsets must share a dtype"),
    "mixed-64-32": (dict(offsets=offs(torch.int32)), "idx and offsets must share a dtype"),
    "no-offsets": (dict(offsets=offs(n=0)), "offsets must hold B \\+ 1 >= 1 entries"),
    "byte-archive": (dict(dtype=torch.uint8), "byte archives hold no floats to sum"),
    "fp64-archive": (dict(dtype=torch.float64), "unsupported dtype torch.float64"),
    "fp16-out-of-bf16": (dict(out_dtype=torch.float16), "out dtype torch.float16 does not go with torch.bfloat16"),
    "bf16-out-of-fp32": (dict(dtype=torch.float32, out_dtype=torch.bfloat16),
                         "out dtype torch.bfloat16 does not go with torch.float32"),
    "fp64-out": (dict(out_dtype=torch.float64), "out dtype torch.float64 does not go with"),
    "wrong-out-tensor-dtype": (dict(out=out(torch.float16)), "out dtype torch.float16 does not go with"),
    "row-words-0": (dict(row_words=0), "row_words must be at least 1"),
    "cpu-tensors": (dict(), "idx and offsets must be CUDA tensors on one device"),
}


@pytest.mark.parametrize("case", WRAPPER_REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    kw, msg = WRAPPER_REJECTS[case]
    args = dict(archive=arch(), row_words=64, idx=idx(), offsets=offs(), dtype=torch.bfloat16)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        C.gather_rows_sum(**args)
