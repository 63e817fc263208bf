"""The argument checks of the matmul through the matrix pipe that fire before any
device is touched: the C ABI, the C++ entry through its test hook, the operator and the wrapper."""
import re

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu


def test_the_operator_its_list_and_the_export():
    assert str(D.matmul_tile.default._schema) == (
        "dietgpu::matmul_tile(Tensor t_in, int row_words, Tensor t_x, Tensor t_out, Tensor? temp_mem=None, "
        "Tensor? out_status=None) -> int")
    assert ops.TILE_OPS == ("matmul_tile",) and ops.matmul_tile is D.matmul_tile
    assert len(ops.OPS) == 12 and ops.MATMUL_OPS == ("matmul_rows",)
    N.lib()
    assert "dietgpu_float_matmul_tile" in N.EXPORTED and hasattr(N.lib(), "dietgpu_float_matmul_tile")
    assert "dietgpu_set_matmul_grid" in N.EXPORTED and hasattr(N.lib(), "dietgpu_set_matmul_grid")
    N.testlib()
    assert "dietgpu_test_matmul_tile_config" in N.TEST_EXPORTED


C_REJECTS = {  # name -> (C ABI arguments that differ from a good call, message); every pointer is null
    "fp32": (dict(ft=3, out32=1), "matmul_rows is the path of an fp32 archive"),
    "fp64": (dict(ft=4, out32=1), r"takes fp16 or bf16 archives \(float type 1 or 2\), not fp64"),
    "bytes": (dict(ft=0), "float_type must be 1..4"),
    "row-words-257": (dict(rw=257), r"rowWords \(257\) must be a positive multiple of 256"),
    "m-65": (dict(m=65), r"M \(65\) must be in 1 .. 64"),
    "prob-bits": (dict(pb=12), "unhandled pdf precision 12"),
    "x-stride-misaligned": (dict(xs=260), r"xRowStrideWords \(260\) must be a whole number of 16 B"),
    "out-too-small": (dict(os=8), r"outRowStrideWords \(8\) must be at least numRows \(9\)"),
    "too-many-words": (dict(rows=1 << 24, os=1 << 24), "must be below 2\\^32"),
    "good": (dict(), "null dietgpu_stack"),  # a good call reaches the next check
}


@pytest.mark.parametrize("case", C_REJECTS)
def test_c_abi_rejects(case):
    kw, msg = C_REJECTS[case]
    a = dict(ft=2, pb=10, rw=256, rows=9, m=3, xs=256, out32=0, os=9)
    a.update(kw)
    rc = N.lib().dietgpu_float_matmul_tile(None, a["ft"], a["pb"], None, a["rw"], a["rows"], None, a["m"], a["xs"],
                                           None, a["out32"], a["os"], None, None)
    assert rc == N.DIETGPU_ERR_INVALID and re.search(msg, N.lib().dietgpu_last_error().decode())


@pytest.mark.parametrize("ft,checksum,out32,m,msg", [
    (2, 1, 0, 3, "a compressed matmul cannot verify a checksum (the decoded words are never stored)"),
    (3, 0, 1, 3, "matmul_rows is the path of an fp32 archive"),
    (2, 0, 0, 65, "M (65) must be in 1 .. 64"),
    (2, 0, 0, 3, "must not be null"),  # a good call reaches the pointer check
])
def test_entry_point_rejects(ft, checksum, out32, m, msg):  # floatMatmulTile itself, over an empty stack
    T = N.testlib()
    rc = T.dietgpu_test_matmul_tile_config(N.Stack(0).h, ft, checksum, None, 256, 9, None, m, None, out32, None, None)
    assert rc == N.DIETGPU_ERR_INVALID and msg in T.dietgpu_test_last_error().decode()


def x(dtype=torch.bfloat16, shape=(3, 256)):
    return torch.full(shape, 3, dtype=dtype)


out = lambda dtype=torch.bfloat16, shape=(3, 9): x(dtype, shape)  # noqa: E731


OP_REJECTS = {  # name -> (row_words, t_x, t_out, message), on CPU tensors
    "fp32-x": (256, lambda: x(torch.float32), lambda: out(torch.float32), "matmul_rows is the path of a float32"),
    "fp64-x": (256, lambda: x(torch.float64), out, "t_x must be float16, bfloat16 or float32"),
    "m-65": (256, lambda: x(shape=(65, 256)), lambda: out(shape=(65, 9)), "t_x must hold 1 .. 64 rows"),
    "cpu-x": (256, x, out, "t_x must be a GPU tensor"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    rw, make_x, make_out, msg = OP_REJECTS[case]
    t, o = make_x(), make_out()
    keep = o.clone()
    with pytest.raises(RuntimeError, match=msg):
        D.matmul_tile(torch.arange(64, dtype=torch.uint8), rw, t, o)
    assert torch.equal(o, keep)


WRAPPER_REJECTS = {
    "byte-archive": (dict(dtype=torch.uint8), "matmul_tile: byte archives hold no floats to multiply"),
    "fp32-archive": (dict(dtype=torch.float32, x=x(torch.float32)), "float32 archives go through matmul_rows"),
    "fp64-archive": (dict(dtype=torch.float64), r"unsupported dtype torch.float64 \(float16 or bfloat16 archives\)"),
    "cpu-tensors": (dict(), "matmul_tile: x and out must be CUDA tensors on one device"),
}


@pytest.mark.parametrize("case", WRAPPER_REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    kw, msg = WRAPPER_REJECTS[case]
    args = dict(archive=torch.arange(64, dtype=torch.uint8), row_words=256, x=x(), dtype=torch.bfloat16, out=out())
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        C.matmul_tile(**args)
