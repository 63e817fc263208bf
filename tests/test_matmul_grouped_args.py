"""The argument checks of the grouped matmul that fire before any device is touched: the
C ABI, the C++ entry through its test hook, the operator and the wrapper; the operator's list; and
planMatmulGrouped's scratch arithmetic through the C ABI's query."""
import re

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu


def test_the_operator_its_list_and_the_export():
    assert str(D.matmul_grouped.default._schema) == (
        "dietgpu::matmul_grouped(Tensor t_archives, int row_words, Tensor t_x, Tensor t_offsets, Tensor t_out, "
        "Tensor? temp_mem=None, Tensor? out_status=None) -> int")
    assert ops.GROUP_OPS == ("matmul_grouped",) and ops.matmul_grouped is D.matmul_grouped
    assert len(ops.OPS) == 12 and ops.MATMUL_OPS == ("matmul_rows",) and ops.TILE_OPS == ("matmul_tile",)
    assert (ops.MORE_OPS, ops.REDUCE_OPS, ops.POOL_OPS) == (("gather_rows",), ("reduce_data",), ("gather_rows_sum",))
    N.lib(), N.testlib()
    assert {"dietgpu_float_matmul_grouped", "dietgpu_set_matmul_grouped_grid"} <= set(N.EXPORTED)
    assert "dietgpu_test_matmul_grouped_config" in N.TEST_EXPORTED


@pytest.mark.parametrize("E,rw,R,T,want", [
    # head 16 + statuses 64 + (64 + 1) entries of 16 B + 4 * T * (R + blocks): pieces 2048 + 2048
    (64, 4096, 2048, 64, 16 + 64 + 16 * 65 + 4 * 64 * 4096),
    # 38,400 words are 10 blocks: pieces 60; T / 64 = 0 chunks past the experts' first
    (4, 768, 50, 25, 16 + 16 + 16 * 4 + 4 * 25 * 60),
    (1025, 768, 50, 25, 0), (4, 768, 50, 0, 0), (4, 700, 50, 25, 0), (4, 768, 1 << 20, 1 << 12, 0),  # refused
])
def test_scratch_bytes_follow_the_plan(E, rw, R, T, want):
    assert N.lib().dietgpu_float_matmul_grouped_scratch_bytes(E, rw, R, T) == want


C_REJECTS = {  # name -> (C ABI arguments that differ from a good call, message); every pointer is null
    "fp32": (dict(ft=3, out32=1), "matmul_rows is the path of an fp32 archive"),
    "fp64": (dict(ft=4, out32=1), r"takes fp16 or bf16 archives \(float type 1 or 2\), not fp64"),
    "bytes": (dict(ft=0), "float_type must be 1..4"),
    "row-words-257": (dict(rw=257), r"rowWords \(257\) must be a positive multiple of 256"),
    "no-expert": (dict(e=0), r"numExperts \(0\) must be in 1 .. 1024"),
    "experts-1025": (dict(e=1025), r"numExperts \(1025\) must be in 1 .. 1024"),
    "no-row": (dict(t=0), "T must be at least 1"),
    "prob-bits": (dict(pb=12), "unhandled pdf precision 12"),
    "x-stride-misaligned": (dict(xs=260), r"xRowStrideWords \(260\) must be a whole number of 16 B"),
    "out-too-small": (dict(os=8), r"outRowStrideWords \(8\) must be at least numRows \(9\)"),
    "partials-past-2^32": (dict(rows=1 << 20, os=1 << 20, t=1 << 12), "must stay below 2\\^32 words"),
    "good": (dict(), "null dietgpu_stack"),  # a good call reaches the next check
}


@pytest.mark.parametrize("case", C_REJECTS)
def test_c_abi_rejects(case):
    kw, msg = C_REJECTS[case]
    a = dict(ft=2, pb=10, e=4, rw=256, rows=9, t=70, xs=256, out32=0, os=9)
    a.update(kw)
    rc = N.lib().dietgpu_float_matmul_grouped(None, a["ft"], a["pb"], None, a["e"], a["rw"], a["rows"], None, a["t"],
                                              a["xs"], None, 1, None, a["out32"], a["os"], None, None)
    assert rc == N.DIETGPU_ERR_INVALID and re.search(msg, N.lib().dietgpu_last_error().decode())


@pytest.mark.parametrize("ft,checksum,out32,e,msg", [
    (2, 1, 0, 4, "a compressed matmul cannot verify a checksum (the decoded words are never stored)"),
    (3, 0, 1, 4, "matmul_rows is the path of an fp32 archive"),
    (2, 0, 0, 1025, "numExperts (1025) must be in 1 .. 1024"),
    (2, 0, 0, 4, "must not be null"),  # a good call reaches the pointer check
])
def test_entry_point_rejects(ft, checksum, out32, e, msg):  # floatMatmulGrouped itself, over an empty stack
    T = N.testlib()
    rc = T.dietgpu_test_matmul_grouped_config(N.Stack(0).h, ft, checksum, None, e, 256, 9, None, 70, None, None,
                                              out32, None, None)
    assert rc == N.DIETGPU_ERR_INVALID and msg in T.dietgpu_test_last_error().decode()


def x(dtype=torch.bfloat16, shape=(3, 256)):
    return torch.full(shape, 3, dtype=dtype)


def ints(n=4, dtype=torch.int64):
    return torch.zeros([n], dtype=dtype)


# name -> (arguments that differ from a good call on CPU tensors, the wrapper's message, the operator's)
REJECTS = {
    "byte-archive": (dict(dtype=torch.uint8), "byte archives hold no floats to multiply", None),
    "fp32-archive": (dict(dtype=torch.float32, x=x(torch.float32)), "float32 archives go through matmul_rows",
                     "multiplies float16 or bfloat16 words, not Float"),
    "fp64-archive": (dict(dtype=torch.float64, x=x(torch.float64)), r"unsupported dtype torch.float64",
                     "multiplies float16 or bfloat16 words, not Double"),
    "row-words-257": (dict(row_words=257), "row_words must be a positive multiple of 256", "positive multiple of 256"),
    "no-expert": (dict(archive_ptrs=ints(0), offsets=ints(1)), "must hold 1 .. 1024 addresses, not 0",
                  "must hold 1 .. 1024 addresses, not 0"),
    "experts-1025": (dict(archive_ptrs=ints(1025), offsets=ints(1026)), "must hold 1 .. 1024 addresses, not 1025",
                     "must hold 1 .. 1024 addresses, not 1025"),
    "x-of-another-dtype": (dict(x=x(torch.float16)), "x must be a 2-d torch.bfloat16 tensor", None),
    "out-of-another-dtype": (dict(out=x(torch.float16, (3, 9))), "out dtype torch.float16 does not go with",
                             r"t_out must have t_x's dtype \(BFloat16\) or float32, not Half"),
    "x-misaligned": (dict(x=x(shape=(3, 260))[:, 4:]), "x's rows must be contiguous, 16-byte aligned",
                     "t_x's rows must be 16-byte aligned"),
    "float-offsets": (dict(offsets=ints(5, torch.float32)), "offsets must be a contiguous 1-d int32 or int64",
                      "t_offsets must be a contiguous 1-d int32 or int64"),
    "offsets-count": (dict(offsets=ints(4)), r"offsets must hold E \+ 1 = 5 entries, not 4", "= 5 entries"),
    "cpu-tensors": (dict(), "archive_ptrs, x and offsets must be CUDA tensors on one device",
                    "t_x must be a GPU tensor"),
}


def arguments(case):
    args = dict(archive_ptrs=ints(4), row_words=256, x=x(), offsets=ints(5), dtype=torch.bfloat16, out=x(shape=(3, 9)))
    args.update(REJECTS[case][0])
    return args


@pytest.mark.parametrize("case", REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    with pytest.raises(ValueError, match="matmul_grouped: .*" + REJECTS[case][1]):
        C.matmul_grouped(**arguments(case))


@pytest.mark.parametrize("case", [c for c in REJECTS if REJECTS[c][2]])
def test_operator_rejects(case):
    a = arguments(case)
    keep = a["out"].clone()
    with pytest.raises(RuntimeError, match=REJECTS[case][2]):
        D.matmul_grouped(a["archive_ptrs"], a["row_words"], a["x"], a["offsets"], a["out"])
    assert torch.equal(a["out"], keep)
