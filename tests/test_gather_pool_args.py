"""The refusals of the pooled row gather with a mode that come
before any device is touched, so they run without a GPU: the C ABI's
dietgpu_float_gather_rows_pool with every pointer null, and
torch.ops.dietgpu.gather_rows_pool and codec.gather_rows_pool on CPU tensors."""
import re

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu


def test_the_names_are_public():
    N.lib()
    assert "dietgpu_float_gather_rows_pool" in N.EXPORTED and hasattr(N.lib(), "dietgpu_float_gather_rows_pool")
    assert ops.POOL_MODE_OPS == ("gather_rows_pool",) and ops.gather_rows_pool is D.gather_rows_pool
    assert ops.POOL_OPS == ("gather_rows_sum",)


def c_call(ft=2, pb=10, rw=64, bags=4, out32=0, stride=64, mode=0, wtype=0, pad=-1):
    rc = N.lib().dietgpu_float_gather_rows_pool(None, ft, pb, None, rw, bags, 9, None, None, 1, mode, None, wtype, pad,
                                                None, out32, stride, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


C_REJECTS = {
    "mode-3": (dict(mode=3), "unknown pooling mode 3"),
    "mode-negative": (dict(mode=-1), "unknown pooling mode -1"),
    "weights-with-mean": (dict(mode=1, wtype=3), "per-sample weights go with mode sum alone, not with mean"),
    "weights-with-max": (dict(mode=2, wtype=2), "per-sample weights go with mode sum alone, not with max"),
    "fp16-weights-bf16-archive": (dict(wtype=1), "weight type 1 does not go with float type 2"),
    "fp64-weights": (dict(wtype=4), "weight type 4 does not go with float type 2"),
    "bf16-weights-fp32-archive": (dict(ft=3, out32=1, wtype=2), "weight type 2 does not go with float type 3"),
    "prob-bits": (dict(pb=12), "unhandled pdf precision 12"),
    "fp64-archive": (dict(ft=4, out32=1), "a pooled row gather takes fp16, bf16 or fp32 archives"),
    "byte-archive": (dict(ft=0), "float_type must be 1..4"),
    "16-bit-out-of-fp32": (dict(ft=3), "the pooled rows of an fp32 archive are fp32"),
    "row-words-0": (dict(rw=0, stride=0), "rowWords must be at least 1"),
    "stride-below-row": (dict(stride=63), r"outRowStrideWords \(63\) must be at least rowWords \(64\)"),
}


@pytest.mark.parametrize("case", C_REJECTS)
def test_c_abi_rejects(case):
    kw, msg = C_REJECTS[case]
    rc, got = c_call(**kw)
    assert rc == N.DIETGPU_ERR_INVALID
    assert re.search(msg, got), got


def test_c_abi_passes_good_arguments_on_and_counts_its_tasks():
    for kw in ({}, dict(mode=1), dict(mode=2, pad=5), dict(wtype=3), dict(wtype=2), dict(ft=3, out32=1, wtype=3)):
        rc, msg = c_call(**kw)
        assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg, kw
    stack = N.Stack(0)  # (an empty stack: the task count comes before any pointer is looked at)
    rc = N.lib().dietgpu_float_gather_rows_pool(stack.h, 2, 10, None, 129, 1 << 31, 9, None, None, 1, 0, None, 0, -1,
                                                None, 0, 129, None, None)
    assert rc == N.DIETGPU_ERR_INVALID
    assert "too many bags: numBags (2147483648) times the 2 column tiles" in N.lib().dietgpu_last_error().decode()


ALONE = "per_sample_weights go with mode 'sum' alone"
WDTYPE = "per_sample_weights must be float32 or of the archive's dtype"
OUT_DTYPE = "t_out must be float16, bfloat16 or float32"
OP_DEVICE = "t_idx and t_offsets must be contiguous GPU tensors"
PY_DEVICE = "idx and offsets must be CUDA tensors on one device"
# name -> (what differs from a good call on a [4, 64] bfloat16 table with 9 indices, the operator's message, the
# wrapper's; None: the layer cannot express it on CPU tensors).  mode / pad / rows: the arguments; w, wn: the
# weights' dtype and length; rw: row_words; out: t_out's dtype; dtype: the wrapper's archive dtype; stride: t_out's.
REJECTS = {
    "unknown-mode": (dict(mode="median"), "unknown mode", "unknown mode"),
    "weights-with-mean": (dict(mode="mean", w=torch.float32), ALONE, ALONE),
    "weights-with-max": (dict(mode="max", w=torch.bfloat16), ALONE, ALONE),
    "fp16-weights-bf16-table": (dict(w=torch.float16), WDTYPE, WDTYPE),
    "fp64-weights": (dict(w=torch.float64), WDTYPE, WDTYPE),
    "too-few-weights": (dict(w=torch.float32, wn=8), "per_sample_weights must be 1-d with t_idx's 9 entries",
                        "per_sample_weights must be a contiguous 1-d tensor of idx's 9 entries"),
    "negative-padding-alone": (dict(pad=-1), "a negative padding_idx .* needs num_rows",
                               "a negative padding_idx .* needs num_rows"),
    "padding-before-the-table": (dict(pad=-41, rows=40), "padding_idx -41 lies outside a table of 40 rows",
                                 "padding_idx -41 lies outside a table of 40 rows"),
    # gather_rows_sum's refusals, in every mode's entry
    "row-words-0": (dict(rw=0), "row_words must be at least 1", "row_words must be at least 1"),
    "fp64-out": (dict(out=torch.float64), OUT_DTYPE, "out dtype torch.float64 does not go with torch.bfloat16"),
    "byte-out": (dict(out=torch.uint8, mode="max"), OUT_DTYPE, "out dtype torch.uint8 does not go with"),
    "fp64-archive": (dict(dtype=torch.float64, mode="mean"), None, "unsupported dtype torch.float64"),
    "byte-archive": (dict(dtype=torch.uint8), None, "byte archives hold no floats to pool"),
    "16-bit-out-of-fp32": (dict(dtype=torch.float32, mode="max"), None,
                           "out dtype torch.bfloat16 does not go with torch.float32"),
    "stride-below-the-row": (dict(stride=63, mode="mean"), "t_out's rows must not overlap", None),
    "rows-overlap": (dict(stride=0, w=torch.float32), "t_out's rows must not overlap", None),
    "idx-32-offsets-64": (dict(idx=torch.int32), "t_offsets must have t_idx's dtype",
                          "idx and offsets must share a dtype"),
    # good calls get as far as the device check
    "good-sum": (dict(), OP_DEVICE, PY_DEVICE),
    "good-mean-padding": (dict(mode="mean", pad=3), OP_DEVICE, PY_DEVICE),
    "good-max-negative-padding": (dict(mode="max", pad=-2, rows=40), OP_DEVICE, PY_DEVICE),
    "good-fp32-weights": (dict(w=torch.float32, pad=0), OP_DEVICE, PY_DEVICE),
    "good-own-weights": (dict(w=torch.bfloat16), OP_DEVICE, PY_DEVICE),
}


@pytest.mark.parametrize("case", REJECTS)
def test_operator_and_wrapper_reject(case):
    kw, op_msg, py_msg = REJECTS[case]
    rw, mode, pad, rows = kw.get("rw", 64), kw.get("mode", "sum"), kw.get("pad"), kw.get("rows")
    a, f = torch.arange(64, dtype=torch.uint8), torch.zeros([5], dtype=torch.int64)
    i = torch.zeros([9], dtype=kw.get("idx", torch.int64))
    w = torch.ones([kw.get("wn", 9)], dtype=kw["w"]) if "w" in kw else None
    o = torch.full([4 * 64], 3, dtype=kw.get("out", torch.bfloat16)).as_strided((4, rw), (kw.get("stride", 64), 1))
    if op_msg:
        with pytest.raises(RuntimeError, match=op_msg):
            D.gather_rows_pool(a, rw, i, f, o, mode, w, pad, rows)
    if py_msg:
        with pytest.raises(ValueError, match=py_msg):
            C.gather_rows_pool(a, rw, i, f, kw.get("dtype", torch.bfloat16), mode=mode, per_sample_weights=w,
                               padding_idx=pad, num_rows=rows, out=o)
    assert bool((o == 3).all())
