"""Argument checks of the fused multi-archive reduce that fire before any
device is touched, so they run without a GPU: torch.ops.dietgpu.reduce_data
(csrc/torch_ops.cpp), the C ABI's dietgpu_float_reduce (csrc/capi.cpp) and
codec.float_reduce.  Every rejection is matched to its message and leaves the
caller's tensors as they were.  tests/test_gpu_reduce.py holds the calls that
need device tensors."""
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMA = ("dietgpu::reduce_data(Tensor[] ts_in, int num_sources, Tensor[] ts_out, Tensor[]? ts_init=None, Tensor? "
          "temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int")


def test_the_operator_is_registered():
    assert ops.REDUCE_OPS == ("reduce_data",)
    assert str(D.reduce_data.default._schema) == SCHEMA
    assert ops.reduce_data is D.reduce_data
    # the operator lists that other tests pin stay as they were
    assert len(ops.OPS) == 12 and ops.MORE_OPS == ("gather_rows",)


def arch():
    return torch.arange(64, dtype=torch.uint8)


def vec(dtype=torch.float32, n=16):
    return torch.arange(n, dtype=torch.float64).to(dtype)


# name -> (ts_in, num_sources, ts_out, ts_init, message)
OP_REJECTS = {
    "k-0": (lambda: ([], 0, [vec()], None), r"num_sources \(0\) must be in 1 .. 64"),
    "k-65": (lambda: ([arch()] * 65, 65, [vec()], None), r"num_sources \(65\) must be in 1 .. 64"),
    "k-negative": (lambda: ([arch()], -1, [vec()], None), "must be in 1 .. 64"),
    "no-outputs": (lambda: ([], 2, [], None), "num_sources archives for each"),
    "too-few-archives": (lambda: ([arch()] * 3, 2, [vec(), vec()], None), "num_sources archives for each"),
    "too-many-archives": (lambda: ([arch()] * 3, 2, [vec()], None), "num_sources archives for each"),
    "init-length": (lambda: ([arch()] * 2, 2, [vec()], [vec(), vec()]), "ts_init and ts_out must have the same length"),
    "mixed-out-dtypes": (lambda: ([arch()] * 2, 1, [vec(), vec(torch.bfloat16)], None), "ts_out must share a dtype"),
    "mixed-init-dtypes": (lambda: ([arch()] * 2, 1, [vec(), vec()], [vec(), vec(torch.float16)]),
                          "ts_init must share a dtype"),
    "float64-out": (lambda: ([arch()], 1, [vec(torch.float64)], None), "ts_out must be float16, bfloat16 or float32"),
    "integer-out": (lambda: ([arch()], 1, [vec(torch.int32)], None), "ts_out must be float16, bfloat16 or float32"),
    "float64-init": (lambda: ([arch()], 1, [vec()], [vec(torch.float64)]),
                     "ts_init must be float16, bfloat16 or float32"),
    "fp16-init-bf16-out": (lambda: ([arch()], 1, [vec(torch.bfloat16)], [vec(torch.float16)]),
                           "different 16-bit archive types"),
    "cpu-tensors": (lambda: ([arch()] * 2, 2, [vec()], None), "inputs must be GPU tensors"),
    "cpu-tensors-with-init": (lambda: ([arch()] * 2, 2, [vec(torch.bfloat16)], [vec()]), "inputs must be GPU tensors"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    make, msg = OP_REJECTS[case]
    ins, k, outs, inits = make()
    every = ins + outs + (inits or [])
    keep = [t.clone() for t in every]
    with pytest.raises(RuntimeError, match=msg):
        D.reduce_data(ins, k, outs, inits)
    assert all(torch.equal(a, b) for a, b in zip(every, keep))


def capi(ft=2, pb=10, k=3, has_init=False, init_type=0, out_type=2):
    """The C ABI with a null stack: the flattened checks come first."""
    import ctypes

    init = ctypes.cast(N.ptr_array([0]), ctypes.c_void_p) if has_init else None
    rc = N.lib().dietgpu_float_reduce(None, ft, pb, 1, k, None, init, init_type, None, None, out_type, None, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


def test_c_abi_is_declared():
    assert "dietgpu_float_reduce" in N.EXPORTED and hasattr(N.lib(), "dietgpu_float_reduce")


@pytest.mark.parametrize("k", [0, 65, 1 << 20])
def test_c_abi_rejects_the_source_count(k):
    rc, msg = capi(k=k)
    assert rc == N.DIETGPU_ERR_INVALID and f"numSources ({k}) must be in 1 .. 64" in msg


@pytest.mark.parametrize("ft,msg", [(0, "float_type must be 1..4"), (5, "float_type must be 1..4"),
                                    (4, "fp16, bf16 or fp32 archives")])
def test_c_abi_rejects_the_float_type(ft, msg):
    rc, got = capi(ft=ft, out_type=ft)
    assert rc == N.DIETGPU_ERR_INVALID and msg in got


@pytest.mark.parametrize("ft,out_type", [(1, 2), (2, 1), (2, 4), (3, 1), (3, 2), (2, 0), (1, 5)])
def test_c_abi_rejects_a_bad_out_type(ft, out_type):
    rc, msg = capi(ft=ft, out_type=out_type)
    assert rc == N.DIETGPU_ERR_INVALID and f"out type {out_type} does not go with float type {ft}" in msg


@pytest.mark.parametrize("ft,init_type", [(1, 2), (2, 1), (2, 4), (3, 2), (2, 0)])
def test_c_abi_rejects_a_bad_init_type(ft, init_type):
    rc, msg = capi(ft=ft, has_init=True, init_type=init_type, out_type=3)
    assert rc == N.DIETGPU_ERR_INVALID and f"init type {init_type} does not go with float type {ft}" in msg


@pytest.mark.parametrize("pb", [0, 8, 12])
def test_c_abi_rejects_prob_bits(pb):
    rc, msg = capi(pb=pb)
    assert rc == N.DIETGPU_ERR_INVALID and f"unhandled pdf precision {pb}" in msg


@pytest.mark.parametrize("ft,has_init,init_type,out_type",
                         [(1, False, 0, 1), (2, False, 7, 3), (3, False, 0, 3), (1, True, 1, 3), (2, True, 3, 2),
                          (3, True, 3, 3)])
def test_c_abi_passes_good_types_on_to_the_next_check(ft, has_init, init_type, out_type):
    for k in (1, 64):
        rc, msg = capi(ft=ft, k=k, has_init=has_init, init_type=init_type, out_type=out_type)
        assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg


def test_python_wrapper_rejects_before_the_device():
    a, f32 = arch(), vec()
    keep = f32.clone()
    with pytest.raises(ValueError, match=r"number of sources \(0\)"):
        C.float_reduce([], [f32])
    with pytest.raises(ValueError, match=r"number of sources \(65\)"):
        C.float_reduce([[a]] * 65, [f32])
    with pytest.raises(ValueError, match="empty batch"):
        C.float_reduce([[]], [])
    with pytest.raises(ValueError, match="one entry per member"):
        C.float_reduce([[a, a], [a]], [f32, f32], ft=2)
    with pytest.raises(ValueError, match="one entry per member"):
        C.float_reduce([[a]], [f32], inits=[f32, f32], ft=2)
    with pytest.raises(ValueError, match="outs must share a dtype"):
        C.float_reduce([[a, a]], [f32, vec(torch.float16)], ft=1)
    with pytest.raises(ValueError, match="inits must share a dtype"):
        C.float_reduce([[a, a]], [f32, f32], inits=[f32, vec(torch.float16)], ft=1)
    with pytest.raises(ValueError, match="unsupported outs dtype"):
        C.float_reduce([[a]], [vec(torch.int32)])
    with pytest.raises(ValueError, match="outs must be contiguous"):
        C.float_reduce([[a]], [vec(n=32)[::2]], ft=2)
    with pytest.raises(ValueError, match="fp16, bf16 or fp32 archives only"):
        C.float_reduce([[a]], [vec(torch.float64)])
    for ft, dt in ((1, torch.bfloat16), (2, torch.float16), (3, torch.bfloat16)):
        with pytest.raises(ValueError, match=f"out type .* does not go with float type {ft}"):
            C.float_reduce([[a]], [vec(dt)], ft=ft)
        with pytest.raises(ValueError, match=f"init type .* does not go with float type {ft}"):
            C.float_reduce([[a]], [f32], inits=[vec(dt)], ft=ft)
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        C.float_reduce([[a], [a]], [f32], inits=[f32], ft=2)
    assert torch.equal(f32, keep)


def test_the_checksum_config_hook_is_declared():
    """The C ABI and the operator have no checksum flag; floatReduceArchives'
    refusal of config.useChecksum is reached through a test hook, which needs a
    stack (tests/test_gpu_reduce.py calls it)."""
    N.testlib()
    assert "dietgpu_test_reduce_config" in N.TEST_EXPORTED


def test_routing_rule_of_the_collectives():
    from dietgpu_fork_amd import dist as Dd

    class Loop:
        pass

    class Fused:
        def reduce(self, own, archives, out_dtype):
            raise AssertionError

    f32, bf, h, d = torch.float32, torch.bfloat16, torch.float16, torch.float64
    for dt in (bf, h, f32):
        assert Dd._fused_reduce(Fused(), dt, f32, 1) and Dd._fused_reduce(Fused(), dt, f32, 64)
        assert not Dd._fused_reduce(Loop(), dt, f32, 3)
        assert not Dd._fused_reduce(Fused(), dt, f32, 0) and not Dd._fused_reduce(Fused(), dt, f32, 65)
    assert not Dd._fused_reduce(Fused(), bf, bf, 3) and not Dd._fused_reduce(Fused(), h, h, 3)
    assert not Dd._fused_reduce(Fused(), d, d, 3)
    assert hasattr(Dd.GpuFloatCodec(), "reduce") and not hasattr(Dd.GpuSparseFloatCodec(), "reduce")
