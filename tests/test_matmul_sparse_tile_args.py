"""Argument checks of the matmul on a sparse archive through the matrix pipe
 that fire before any device is touched, so they run without a
GPU -- the C ABI's dietgpu_float_matmul_sparse_tile and
codec.matmul_sparse_tile, each rejection matched to its own message -- and the
scratch arithmetic of planSparseMatmulTile."""
import re

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMA = ("dietgpu::matmul_sparse_tile(Tensor t_in, int row_words, Tensor t_x, Tensor t_out, int nnz_bound, "
          "Tensor? temp_mem=None, Tensor? out_status=None) -> int")


def test_the_operator_its_list_and_the_exports():
    assert str(D.matmul_sparse_tile.default._schema) == SCHEMA
    assert ops.SPARSE_TILE_OPS == ("matmul_sparse_tile",) and ops.matmul_sparse_tile is D.matmul_sparse_tile
    N.lib()
    for name in ("dietgpu_float_matmul_sparse_tile", "dietgpu_float_matmul_sparse_tile_scratch_bytes"):
        assert name in N.EXPORTED and hasattr(N.lib(), name)


# name -> (C ABI arguments that differ from a good call, message); every pointer is null
C_REJECTS = {
    "row-words-0": (dict(rw=0, xs=0), r"rowWords \(0\) must be a positive multiple of 256"),
    "row-words-255": (dict(rw=255), r"rowWords \(255\) must be a positive multiple of 256"),
    "row-words-257": (dict(rw=257), r"rowWords \(257\) must be a positive multiple of 256"),
    "m-0": (dict(m=0), r"M \(0\) must be in 1 .. 64"),
    "m-65": (dict(m=65), r"M \(65\) must be in 1 .. 64"),
    "fp32": (dict(ft=3, out32=1), "a tiled sparse matmul multiplies 16-bit words .* matmul_sparse is the path of an fp32"),
    "fp64": (dict(ft=4, out32=1), r"a tiled sparse matmul takes fp16 or bf16 archives \(float type 1 or 2\), not fp64"),
    "bytes": (dict(ft=0), "float_type must be 1..4"),
    "x-stride-short": (dict(xs=248), r"xRowStrideWords \(248\) must be at least rowWords \(256\)"),
    "x-stride-misaligned": (dict(xs=260), r"xRowStrideWords \(260\) must be a whole number of 16 B"),
    "out-too-small": (dict(os=20), r"outRowStrideWords \(20\) must be at least numRows \(21\)"),
    "too-many-words": (dict(rows=1 << 24, os=1 << 24), "must be below 2\\^32"),
    "list-capacity-0": (dict(cap=0), r"listCapacityWords \(0\) must be in 1 .. 2\^32 - 34"),
    "list-capacity-wraps": (dict(cap=(1 << 32) - 20), r"listCapacityWords \(4294967276\) must be in 1 .. 2\^32 - 34"),
    "good": (dict(), "null dietgpu_stack"),  # a good call reaches the next check
}


@pytest.mark.parametrize("case", C_REJECTS)
def test_c_abi_rejects(case):
    kw, msg = C_REJECTS[case]
    a = dict(ft=2, pb=10, rw=256, rows=21, m=17, xs=256, out32=0, os=21, cap=1000)
    a.update(kw)
    rc = N.lib().dietgpu_float_matmul_sparse_tile(None, a["ft"], a["pb"], None, a["rw"], a["rows"], None, a["m"],
                                                  a["xs"], None, a["out32"], a["os"], a["cap"], None, None)
    assert rc == N.DIETGPU_ERR_INVALID
    assert re.search(msg, N.lib().dietgpu_last_error().decode())


def x(dtype=torch.bfloat16, shape=(3, 256)):
    return torch.ones(shape, dtype=dtype)


def out(dtype=torch.bfloat16, shape=(3, 21)):
    return torch.full(shape, 3, dtype=dtype)


WRAPPER_REJECTS = {
    "byte-archive": (dict(dtype=torch.uint8), "matmul_sparse_tile: byte archives hold no floats to multiply"),
    "fp32-archive": (dict(dtype=torch.float32, x=x(torch.float32)),
                     "matmul_sparse_tile: float32 archives go through matmul_sparse"),
    "fp64-archive": (dict(dtype=torch.float64), "matmul_sparse_tile: unsupported dtype torch.float64"),
    "x-of-another-dtype": (dict(x=x(torch.float16)), "matmul_sparse_tile: x must be a 2-d torch.bfloat16 tensor"),
    "row-words-255": (dict(row_words=255), "matmul_sparse_tile: row_words must be a positive multiple of 256"),
    "row-words-0": (dict(row_words=0), "matmul_sparse_tile: row_words must be a positive multiple of 256"),
    "x-other-width": (dict(row_words=512), "x must have row_words = 512 columns"),
    "m-65": (dict(x=x(shape=(65, 256))), "matmul_sparse_tile: x must hold 1 .. 64 rows"),
    "m-0": (dict(x=x(shape=(0, 256))), "matmul_sparse_tile: x must hold 1 .. 64 rows"),
    "fp16-out-of-bf16": (dict(out=out(torch.float16)), "out dtype torch.float16 does not go with torch.bfloat16"),
    "nnz-bound-0": (dict(nnz_bound=0), "matmul_sparse_tile: nnz_bound must be at least 1"),
    "out-other-rows": (dict(out=out(shape=(4, 21))), r"out must be a torch.bfloat16 tensor of shape \[3, R\]"),
    "x-misaligned": (dict(x=x(shape=(3, 260))[:, :256]), "x's rows must be contiguous, 16-byte aligned"),
    "out-stride-short": (dict(out=out(shape=(21,)).as_strided((3, 21), (0, 1))), "its rows at least R apart"),
    "too-many-words": (dict(out=out(shape=(1,)).as_strided((3, 1 << 24), (0, 0))), r"R \* row_words must be below 2\^32"),
    "cpu-tensors": (dict(), "matmul_sparse_tile: x and out must be CUDA tensors on one device"),
    "cpu-tensors-no-bound": (dict(nnz_bound=None), "matmul_sparse_tile: x and out must be CUDA tensors on one device"),
}


@pytest.mark.parametrize("case", WRAPPER_REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    kw, msg = WRAPPER_REJECTS[case]
    args = dict(archive=torch.arange(64, dtype=torch.uint8), row_words=256, x=x(), dtype=torch.bfloat16, out=out(),
                nnz_bound=9)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        C.matmul_sparse_tile(**args)


@pytest.mark.parametrize("ft,K,R,M,cap", [(1, 1280, 17, 5, 9000), (2, 4096, 4096, 64, 1 << 23)])
def test_scratch_is_the_plans(ft, K, R, M, cap):
    """planSparseMatmulTile: the list rounded up to 16 words plus 16; a count,
    a prefix and a list offset per 1024-word chunk of the table, a total per
    256 chunks; ceil(K / 1024) partial sums per (m, r); every allocation a
    whole number of 256-byte granules."""
    gran = lambda b: max(1, -(-b // 256)) * 256  # noqa: E731
    chunks, slices = -(-R * K // 1024), -(-K // 1024)
    want = (gran(8) + gran(4) + gran(1) + gran((-(-cap // 16) * 16 + 16) * 2) + 2 * gran(4 * chunks) +
            gran(4 * -(-chunks // 256)) + gran(4 * M * R * slices))
    assert C.matmul_sparse_tile_scratch_bytes(ft, K, R, M, cap) == want
    assert N.lib().dietgpu_float_matmul_sparse_tile_scratch_bytes(3, K, R, M, cap) == 0
    assert "matmul_sparse is the path of an fp32 archive" in N.lib().dietgpu_last_error().decode()
