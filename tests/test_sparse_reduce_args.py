"""Argument checks of the fused sparse reduce that fire before any device is
touched, so they run without a GPU: codec.sparse_reduce (every Python-side
rejection, matched to its message, the caller's tensors left as they were),
the flattened checks of the C ABI's dietgpu_float_reduce_sparse, the scratch
query's refusals, and the routing clause of the collectives.
tests/test_gpu_sparse_reduce.py holds the calls that need device tensors."""
import ctypes

import pytest
import torch

import dietgpu_fork_amd  # noqa: F401
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import codec as C


def arch():
    return torch.arange(64, dtype=torch.uint8)


def vec(dtype=torch.float32, n=16):
    return torch.arange(n, dtype=torch.float64).to(dtype)


A, F32 = arch(), vec()

# name -> (sources, outs, inits, ft, message)
REJECTS = {
    "k-0": (lambda: ([], [F32], None, None), r"sparse_reduce: the number of sources \(0\) must be in 1 .. 64"),
    "k-65": (lambda: ([[A]] * 65, [F32], None, None), r"sparse_reduce: the number of sources \(65\) must be in 1 .. 64"),
    "empty-batch": (lambda: ([[]], [], None, None), "sparse_reduce: empty batch"),
    "ragged-sources": (lambda: ([[A, A], [A]], [F32, vec()], None, 2), "one entry per member"),
    "ragged-inits": (lambda: ([[A]], [F32], [vec(), vec()], 2), "one entry per member"),
    "mixed-out-dtypes": (lambda: ([[A, A]], [F32, vec(torch.float16)], None, 1), "the outs must share a dtype"),
    "mixed-init-dtypes": (lambda: ([[A, A]], [F32, vec()], [vec(), vec(torch.float16)], 1),
                          "the inits must share a dtype"),
    "integer-out": (lambda: ([[A]], [vec(torch.int32)], None, None), "unsupported outs dtype"),
    "fp64": (lambda: ([[A]], [vec(torch.float64)], None, None), "fp16, bf16 or fp32 archives only, not float type 4"),
    "fp64-init": (lambda: ([[A]], [F32], [vec(torch.float64)], 2), "init type 4 does not go with float type 2"),
    "bf16-out-of-fp16": (lambda: ([[A]], [vec(torch.bfloat16)], None, 1), "out type 2 does not go with float type 1"),
    "fp16-out-of-bf16": (lambda: ([[A]], [vec(torch.float16)], None, 2), "out type 1 does not go with float type 2"),
    "bf16-out-of-fp32": (lambda: ([[A]], [vec(torch.bfloat16)], None, 3), "out type 2 does not go with float type 3"),
    "fp16-init-of-bf16": (lambda: ([[A]], [F32], [vec(torch.float16)], 2), "init type 1 does not go with float type 2"),
    "bf16-init-of-fp32": (lambda: ([[A]], [F32], [vec(torch.bfloat16)], 3), "init type 2 does not go with float type 3"),
    "non-contiguous-out": (lambda: ([[A]], [vec(n=32)[::2]], None, 2), "the outs must be contiguous"),
    "non-contiguous-init": (lambda: ([[A]], [F32], [vec(n=32)[::2]], 2), "the inits must be contiguous"),
    "cpu-tensors": (lambda: ([[A], [A]], [F32], None, 2), "sparse_reduce: archives, inits and outs must be CUDA tensors"),
    "cpu-tensors-with-init": (lambda: ([[A]], [vec(torch.bfloat16)], [vec()], None), "must be CUDA tensors"),
}


@pytest.mark.parametrize("case", REJECTS)
def test_python_wrapper_rejects_before_the_device(case):
    make, msg = REJECTS[case]
    sources, outs, inits, ft = make()
    every = [a for row in sources for a in row] + list(outs) + list(inits or [])
    keep = [t.clone() for t in every]
    with pytest.raises(ValueError, match=msg):
        C.sparse_reduce(sources, outs, inits=inits, ft=ft)
    assert all(torch.equal(a, b) for a, b in zip(every, keep))


def capi(ft=2, pb=10, k=3, has_init=False, init_type=0, out_type=2):
    """The C ABI with a null stack: the flattened checks come first."""
    init = ctypes.cast(N.ptr_array([0]), ctypes.c_void_p) if has_init else None
    rc = N.lib().dietgpu_float_reduce_sparse(None, ft, pb, 1, k, None, init, init_type, None, None, out_type, None,
                                             None, None)
    return rc, N.lib().dietgpu_last_error().decode()


def test_c_abi_is_declared_and_bound():
    for name in ("dietgpu_float_reduce_sparse", "dietgpu_float_reduce_sparse_scratch_bytes"):
        assert name in N.EXPORTED and hasattr(N.lib(), name)
    N.testlib()
    assert "dietgpu_test_sparse_reduce_config" in N.TEST_EXPORTED


@pytest.mark.parametrize("kw,msg", [
    (dict(k=0), "numSources (0) must be in 1 .. 64"), (dict(k=65), "numSources (65) must be in 1 .. 64"),
    (dict(ft=0, out_type=0), "float_type must be 1..4"), (dict(ft=4, out_type=4), "fp16, bf16 or fp32 archives"),
    (dict(ft=1, out_type=2), "out type 2 does not go with float type 1"),
    (dict(ft=3, out_type=1), "out type 1 does not go with float type 3"),
    (dict(ft=2, has_init=True, init_type=1, out_type=3), "init type 1 does not go with float type 2"),
    (dict(pb=8), "unhandled pdf precision 8"), (dict(pb=12), "unhandled pdf precision 12"),
])
def test_c_abi_rejects(kw, msg):
    rc, got = capi(**kw)
    assert rc == N.DIETGPU_ERR_INVALID and msg in got


@pytest.mark.parametrize("ft,has_init,init_type,out_type",
                         [(1, False, 0, 1), (2, False, 7, 3), (3, False, 0, 3), (1, True, 1, 3), (2, True, 3, 2),
                          (3, True, 3, 3)])
def test_c_abi_passes_good_types_on_to_the_next_check(ft, has_init, init_type, out_type):
    for k in (1, 64):
        rc, msg = capi(ft=ft, k=k, has_init=has_init, init_type=init_type, out_type=out_type)
        assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg


def test_scratch_query_refuses_what_the_call_refuses():
    for ft, k, msg in ((4, 3, "fp16, bf16 or fp32 archives"), (2, 0, "must be in 1 .. 64"), (2, 65, "must be in 1 .. 64")):
        assert N.lib().dietgpu_float_reduce_sparse_scratch_bytes(ft, 1, k, 1000) == 0
        assert msg in N.lib().dietgpu_last_error().decode()
        with pytest.raises(N.DietGpuError, match=msg):
            C.sparse_reduce_scratch_bytes(ft, 1, k, 1000)
    assert C.sparse_reduce_scratch_bytes(2, 1, 3, 1000) > 0


def test_routing_clause_of_the_collectives():
    """dist._fused_reduce: a codec whose `reduce_fits` says no keeps the loop;
    a codec without one (GpuFloatCodec) is never asked; GpuSparseFloatCodec
    answers from the scratch query and its workspace size."""
    from dietgpu_fork_amd import dist as D

    class Fused:
        def reduce(self, own, archives, out_dtype):
            raise AssertionError

    class Bounded(Fused):
        def __init__(self, limit):
            self.limit = limit

        def reduce_fits(self, numel, dtype, num_archives):
            return numel <= self.limit

    f32, bf = torch.float32, torch.bfloat16
    assert D._fused_reduce(Fused(), bf, f32, 7, 10 ** 9)
    assert D._fused_reduce(Bounded(1000), bf, f32, 7, 1000) and not D._fused_reduce(Bounded(1000), bf, f32, 7, 1001)
    assert not D._fused_reduce(Bounded(1000), bf, bf, 7, 10)  # the other clauses still hold
    assert not hasattr(D.GpuFloatCodec(), "reduce_fits")
    # the sparse codec's fused reduction skips zeros: it is `sparse_reduce`, not `reduce`
    assert D._fused_entry(D.GpuSparseFloatCodec()) is not None and hasattr(D.GpuSparseFloatCodec, "sparse_reduce")
    assert D._fused_entry(Fused()) is not None and D._fused_entry(object()) is None
    big, small = D.GpuSparseFloatCodec(), D.GpuSparseFloatCodec(workspace_bytes=1 << 20)
    assert big.reduce_fits(70001, bf, 7) and not small.reduce_fits(70001 * 16, bf, 7)
    need = C.sparse_reduce_scratch_bytes(2, 1, 7, 15_000_000)
    assert big.reduce_fits(15_000_000, bf, 7) == (need <= 256 << 20)
    assert D._fused_reduce(small, bf, f32, 7, 1000) and not D._fused_reduce(small, bf, f32, 7, 70001 * 16)
