"""Argument checks of the matmul on a sparse archive that fire
before any device is touched, so they run without a GPU -- the C ABI's
dietgpu_float_matmul_sparse_rows, the C++ entry point through its test hook,
torch.ops.dietgpu.matmul_sparse and codec.matmul_sparse, each rejection matched
to its own message -- and the scratch arithmetic of planSparseMatmul."""
import re

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMA = ("dietgpu::matmul_sparse(Tensor t_in, int row_words, Tensor t_x, Tensor t_out, int nnz_bound, "
          "Tensor? temp_mem=None, Tensor? out_status=None) -> int")


def test_the_operator_its_list_and_the_export():
    assert str(D.matmul_sparse.default._schema) == SCHEMA
    assert ops.SPARSE_MATMUL_OPS == ("matmul_sparse",) and ops.matmul_sparse is D.matmul_sparse
    assert len(ops.OPS) == 12 and ops.MATMUL_OPS == ("matmul_rows",) and ops.GROUP_OPS == ("matmul_grouped",)
    N.lib()
    for name in ("dietgpu_float_matmul_sparse_rows", "dietgpu_float_matmul_sparse_scratch_bytes"):
        assert name in N.EXPORTED and hasattr(N.lib(), name)
    N.testlib()
    assert "dietgpu_test_matmul_sparse_config" in N.TEST_EXPORTED


# name -> (C ABI arguments that differ from a good call, message); every pointer is null
C_REJECTS = {
    "row-words-0": (dict(rw=0, xs=0), r"rowWords \(0\) must be a positive multiple of 256"),
    "row-words-255": (dict(rw=255), r"rowWords \(255\) must be a positive multiple of 256"),
    "row-words-257": (dict(rw=257), r"rowWords \(257\) must be a positive multiple of 256"),
    "m-0": (dict(m=0), r"M \(0\) must be in 1 .. 64"),
    "m-65": (dict(m=65), r"M \(65\) must be in 1 .. 64"),
    "fp64": (dict(ft=4, out32=1), r"takes fp16, bf16 or fp32 archives \(float type 1..3\), not 4"),
    "bytes": (dict(ft=0), "float_type must be 1..4"),
    "fp32-to-16-bit": (dict(ft=3), "the products of an fp32 archive are fp32"),
    "x-stride-short": (dict(xs=248), r"xRowStrideWords \(248\) must be at least rowWords \(256\)"),
    "x-stride-misaligned": (dict(xs=260), r"xRowStrideWords \(260\) must be a whole number of 16 B"),
    "out-too-small": (dict(os=8), r"outRowStrideWords \(8\) must be at least numRows \(9\)"),
    "too-many-words": (dict(rows=1 << 24, os=1 << 24), "must be below 2\\^32"),
    "list-capacity-0": (dict(cap=0), r"listCapacityWords \(0\) must be in 1 .. 2\^32 - 34"),
    "list-capacity-wraps": (dict(cap=(1 << 32) - 20), r"listCapacityWords \(4294967276\) must be in 1 .. 2\^32 - 34"),
    "good": (dict(), "null dietgpu_stack"),  # a good call reaches the next check
}


@pytest.mark.parametrize("case", C_REJECTS)
def test_c_abi_rejects(case):
    kw, msg = C_REJECTS[case]
    a = dict(ft=2, pb=10, rw=256, rows=9, m=3, xs=256, out32=0, os=9, cap=1000)
    a.update(kw)
    rc = N.lib().dietgpu_float_matmul_sparse_rows(None, a["ft"], a["pb"], None, a["rw"], a["rows"], None, a["m"],
                                                  a["xs"], None, a["out32"], a["os"], a["cap"], None, None)
    assert rc == N.DIETGPU_ERR_INVALID
    assert re.search(msg, N.lib().dietgpu_last_error().decode())


@pytest.mark.parametrize("args,msg", [
    ((2, 1, 0, 256, 9, 3, 9), "a compressed matmul cannot verify a checksum (the decoded words are never stored)"),
    ((4, 0, 1, 256, 9, 3, 9), "takes fp16, bf16 or fp32 archives (float type 1..3), not 4"),
    ((2, 0, 0, 257, 9, 3, 9), "rowWords (257) must be a positive multiple of 256"),
    ((2, 0, 0, 256, 9, 65, 9), "M (65) must be in 1 .. 64"),
    ((2, 0, 0, 256, 9, 3, 0), "listCapacityWords (0) must be in 1 .. 2^32 - 34"),
    ((2, 0, 0, 256, 9, 3, 9), "must not be null"),  # a good call reaches the pointer check
])
def test_entry_point_rejects(args, msg):
    """floatMatmulSparseRows' own refusals, over an empty stack: a config with
    useChecksum set, which no layer above can express, among them."""
    ft, checksum, out32, rw, rows, m, cap = args
    T = N.testlib()
    rc = T.dietgpu_test_matmul_sparse_config(N.Stack(0).h, ft, checksum, None, rw, rows, None, m, None, out32, cap,
                                             None, None)
    assert rc == N.DIETGPU_ERR_INVALID and msg in T.dietgpu_test_last_error().decode()


def x(dtype=torch.bfloat16, shape=(3, 256)):
    return torch.ones(shape, dtype=dtype)


def out(dtype=torch.bfloat16, shape=(3, 9)):
    return torch.full(shape, 3, dtype=dtype)


# name -> (row_words, t_x, t_out, nnz_bound, message); CPU tensors: these checks come before any device check
OP_REJECTS = {
    "row-words-0": (0, x, out, 9, "row_words must be a positive multiple of 256"),
    "row-words-257": (257, lambda: x(shape=(3, 257)), out, 9, "row_words must be a positive multiple of 256"),
    "fp64-x": (256, lambda: x(torch.float64), out, 9, "t_x must be float16, bfloat16 or float32"),
    "fp16-out-of-bf16": (256, x, lambda: out(torch.float16), 9, "t_out must have t_x's dtype"),
    "x-other-width": (256, lambda: x(shape=(3, 512)), out, 9, "t_x must have the shape"),
    "out-other-lead": (256, x, lambda: out(shape=(4, 9)), 9, "t_out must have the shape"),
    "out-too-small": (256, x, lambda: out(shape=(3, 0)), 9, "t_out must have the shape"),
    "m-65": (256, lambda: x(shape=(65, 256)), lambda: out(shape=(65, 9)), 9, "t_x must hold 1 .. 64 rows"),
    "m-0": (256, lambda: x(shape=(0, 256)), lambda: out(shape=(0, 9)), 9, "t_x must hold 1 .. 64 rows"),
    "nnz-bound-0": (256, x, out, 0, "nnz_bound must be at least 1"),
    "x-misaligned": (256, lambda: x(shape=(3 * 256 + 1,))[1:].view(3, 256), out, 9, "t_x's rows must be 16-byte aligned"),
    "x-stride-misaligned": (256, lambda: x(shape=(3, 260))[:, :256], out, 9, "t_x's rows must be 16-byte aligned"),
    "out-rows-overlap": (256, x, lambda: out(shape=(9,)).as_strided((3, 9), (0, 1)), 9, "rows must not overlap"),
    "cpu-x": (256, x, out, 9, "t_x must be a GPU tensor"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    rw, make_x, make_out, bound, msg = OP_REJECTS[case]
    t, o = make_x(), make_out()
    keep = o.clone()
    with pytest.raises(RuntimeError, match=msg):
        D.matmul_sparse(torch.arange(64, dtype=torch.uint8), rw, t, o, bound)
    assert torch.equal(o, keep)


WRAPPER_REJECTS = {
    "byte-archive": (dict(dtype=torch.uint8), "matmul_sparse: byte archives hold no floats to multiply"),
    "x-of-another-dtype": (dict(x=x(torch.float16)), "matmul_sparse: x must be a 2-d torch.bfloat16 tensor"),
    "row-words-255": (dict(row_words=255), "matmul_sparse: row_words must be a positive multiple of 256"),
    "x-other-width": (dict(row_words=512), "x must have row_words = 512 columns"),
    "fp16-out-of-bf16": (dict(out=out(torch.float16)), "out dtype torch.float16 does not go with torch.bfloat16"),
    "nnz-bound-0": (dict(nnz_bound=0), "matmul_sparse: nnz_bound must be at least 1"),
    "out-other-rows": (dict(out=out(shape=(4, 9))), r"out must be a torch.bfloat16 tensor of shape \[3, R\]"),
    "x-misaligned": (dict(x=x(shape=(3, 260))[:, :256]), "x's rows must be contiguous, 16-byte aligned"),
    "cpu-tensors": (dict(), "matmul_sparse: x and out must be CUDA tensors on one device"),
    "cpu-tensors-no-bound": (dict(nnz_bound=None), "matmul_sparse: x and out must be CUDA tensors on one device"),
}


@pytest.mark.parametrize("case", WRAPPER_REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    kw, msg = WRAPPER_REJECTS[case]
    args = dict(archive=torch.arange(64, dtype=torch.uint8), row_words=256, x=x(), dtype=torch.bfloat16, out=out(),
                nnz_bound=9)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        C.matmul_sparse(**args)


@pytest.mark.parametrize("ft,K,R,M,cap", [(2, 256, 9, 1, 1), (1, 768, 7, 5, 2700), (3, 1024, 257, 64, 263169),
                                          (2, 4096, 4096, 64, 1 << 23)])
def test_scratch_is_the_plans(ft, K, R, M, cap):
    """planSparseMatmul: a wave per 1024-word chunk of the table, R + chunks
    pieces per activation row, the list rounded up to 16 words plus 16, every
    allocation a whole number of 256-byte granules."""
    gran = lambda b: max(1, -(-b // 256)) * 256  # noqa: E731
    chunks = -(-R * K // 1024)
    word = 4 if ft == 3 else 2
    want = (gran(8) + gran(4) + gran(1) + gran((-(-cap // 16) * 16 + 16) * word) + gran(4 * chunks) +
            gran(4 * -(-chunks // 256)) + gran(4 * M * (R + chunks)))
    assert C.matmul_sparse_scratch_bytes(ft, K, R, M, cap) == want


def test_scratch_query_refuses_what_the_call_refuses():
    for args, msg in (((4, 256, 9, 3, 9), "float type 1..3"), ((2, 255, 9, 3, 9), "multiple of 256"),
                      ((2, 256, 9, 65, 9), "must be in 1 .. 64"), ((2, 256, 9, 3, 0), "listCapacityWords")):
        assert N.lib().dietgpu_float_matmul_sparse_scratch_bytes(*args) == 0
        assert msg in N.lib().dietgpu_last_error().decode()
