"""GPU tests of the matmul on a sparse archive through the matrix pipe (DESIGN.md
5.2o): codec.matmul_sparse_tile, torch.ops.dietgpu.matmul_sparse_tile and the C
ABI's dietgpu_float_matmul_sparse_tile over k_sparseMatmulTile.  The tables,
the activations and the bound are test_gpu_matmul_sparse.py's own helpers:
seeded N(0, 1), magnitude-pruned, compressed by codec.sparse_compress, W what
codec.sparse_decompress returns; against the fp64 product within K 2^-23
(|x| |W|^T), plus one rounding to nearest for a 16-bit out (5.2j)."""
import ctypes

import pytest
import torch

from tests import matmul_cases as MC
from tests.gpu_harness import C, DEV, N, dense_at, retyped, workspace_fixture  # noqa: F401
from tests.test_gpu_matmul_sparse import _MADE, _blank, _gap, _mirror, acts, archive_of, bits, close, table
from tests.util import TORCH_FLOAT

pytestmark = pytest.mark.gpu

# (K, R): a full row block and one of five rows, four rows per chunk; groups of
# a block from different chunks, a slice shorter than 1024; two slices (1024 +
# 256) and a row block of one row
SHAPES = [(256, 21), (768, 19), (1280, 17)]
# ... and 263,168 words: a second counting workgroup
CASES = [(K, R, M) for K, R in SHAPES for M in (1, 5, 16, 17, 64)] + [(1024, 257, 17)]
FILL = 0xA5

ws = workspace_fixture(16 << 20)


def run(C, ws, a, K, x, R, ft, out_dtype=torch.float32, **kw):
    out = torch.empty([x.size(0), R], dtype=out_dtype, device=DEV)
    C.matmul_sparse_tile(a, K, x.to(DEV), TORCH_FLOAT[ft], out=out, ws=ws, check=True, **kw)
    return out


@pytest.mark.parametrize("zeros", [0.5, 0.9])
@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,R,M", CASES, ids=[f"{K}x{R}-M{M}" for K, R, M in CASES])
def test_against_fp64(C, ws, K, R, M, ft, zeros):
    """fp32 out at 50 % zeros, the archive's own type at 90 %; nnz_bound read from the archive."""
    W, a, _ = table(C, ws, ft, K, R, zeros)
    x = acts(ft, M, K)
    assert close(run(C, ws, a, K, x, R, ft, torch.float32 if zeros == 0.5 else TORCH_FLOAT[ft]), x, W, ft)


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pattern", ["no-zeros", "zero-rows-and-chunk", "tail-37", "more-rows"])
def test_patterns_and_prefix_tables(C, ws, pattern, ft):
    """Words past the table (37 of them, or three more rows) change no bit of out."""
    K, R, x = 256, 21, acts(ft, 17, 256)
    if pattern in ("tail-37", "more-rows"):
        W, a, _ = table(C, ws, ft, K, R)
        Wt, at, _ = table(C, ws, ft, K, R, tail=37 if pattern == "tail-37" else 3 * K)
        assert torch.equal(bits(Wt), bits(W))
        assert torch.equal(bits(run(C, ws, at, K, x, R, ft)), bits(run(C, ws, a, K, x, R, ft)))
    else:
        W, a, _ = table(C, ws, ft, K, R, zeros=0.0 if pattern == "no-zeros" else 0.5,
                        edit=_blank if pattern != "no-zeros" else None, key=pattern)
        assert (pattern == "no-zeros") == bool((W != 0).all())
    out = run(C, ws, a, K, x, R, ft)
    assert close(out, x, W, ft) and (pattern != "zero-rows-and-chunk" or bool((out[:, [0, 4, 5, 6, 7]] == 0).all()))


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("edit", [None, _gap, _mirror], ids=["units", "gap", "mirror"])
@pytest.mark.parametrize("K,R", [(256, 21), (1280, 17)])
def test_unit_vectors_return_the_words(C, ws, K, R, edit, ft):
    """x[m] = e_k: out[m, r] is W[r, k] itself, the last two words of the element among them."""
    W, a, _ = table(C, ws, ft, K, R, edit=edit, key=edit and edit.__name__)
    ks = [0, 63, 64, 255, K // 2 + 1, K - 2, K - 1]
    out = run(C, ws, a, K, MC.unit_acts(ft, ks, K), R, ft)
    assert torch.equal(bits(out), bits(W[:, ks].float().T.contiguous() + 0.0))
    assert edit is None or (float(W[-1, -1]), float(W[-1, -2])) in ((1.5, 0.0), (0.0, 1.5))


@pytest.mark.parametrize("M", [5, 64])
@pytest.mark.parametrize("K,R", [(768, 19), (1280, 17)])
@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_exact_sums(C, ws, ft, K, R, M):
    """Integer products with half the table punched out: out equals b @ a.T bit for bit."""
    a, e, W = MC.exact_table(ft, K, R)
    hole = torch.rand([R, K], generator=torch.Generator().manual_seed(3)) < 0.5
    a[hole.numpy()] = 0
    W[hole] = 0
    b, x = MC.exact_acts(ft, M, K, e)
    back, arch, _ = _MADE.get(("exact", ft, K, R), lambda: archive_of(C, ws, W.reshape(-1), ft))
    assert torch.equal(bits(back), bits(W.reshape(-1)))
    assert torch.equal(bits(run(C, ws, arch, K, x, R, ft)), bits(MC.exact_product(b, a)))


def test_order_is_a_function_of_k_alone(C, ws):
    K, R, x = 1280, 17, acts(2, 64, 1280)
    W, a, _ = table(C, ws, 2, K, R)
    _, a20, _ = table(C, ws, 2, K, R, tail=3 * K)
    o64 = run(C, ws, a, K, x, R, 2)
    assert torch.equal(bits(o64), bits(run(C, ws, a, K, x, R, 2)))
    for M in (1, 5, 17):
        assert torch.equal(bits(o64[:M]), bits(run(C, ws, a, K, x[:M], R, 2))), M
    assert torch.equal(bits(o64), bits(run(C, ws, a20, K, x, R + 3, 2)[:, :R]))
    for R1 in (16, 1):
        assert torch.equal(bits(o64[:, :R1]), bits(run(C, ws, a, K, x, R1, 2))), R1


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_a_clear_bit_is_multiplied(C, ws, ft):
    """Inf in x[0, k]: NaN where W[r, k] is zero, +-Inf by W's sign where it is not; the other rows as ever."""
    K, R, k = 256, 21, 5
    W, a, _ = table(C, ws, ft, K, R)
    zero = W[:, k] == 0
    assert bool(zero.any()) and not bool(zero.all())
    x = acts(ft, 4, K)
    x[0, k] = float("inf")
    out = run(C, ws, a, K, x, R, ft).cpu()
    assert bool(out[0, zero].isnan().all()) and close(out[1:], x[1:], W, ft)
    assert torch.equal(out[0, ~zero], float("inf") * torch.sign(W[~zero, k].float()))


@pytest.mark.parametrize("fault", ["float-type", "one-row-more", "nnz-bound-short"])
def test_failure_writes_the_status_alone(C, ws, fault):
    K, R, M = 768, 19, 3
    _, a, nnz = table(C, ws, 2, K, R)
    if fault == "float-type":
        a = retyped(a, 2, at=dense_at(R * K) + 8)
    rows = R + 1 if fault == "one-row-more" else R
    out = torch.full([M, 4 * rows], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    kw = dict(out=out, ws=ws, nnz_bound=nnz - 1 if fault == "nnz-bound-short" else nnz)
    _, ok = C.matmul_sparse_tile(a, K, acts(2, M, K).to(DEV), torch.bfloat16, **kw)
    assert int(ok) == 0
    with pytest.raises(C.N.DietGpuError, match="matmul_sparse_tile: the archive does not match"):
        C.matmul_sparse_tile(a, K, acts(2, M, K).to(DEV), torch.bfloat16, check=True, **kw)
    assert bool((out.view(torch.uint8) == FILL).all())


def test_strided_out_operator_and_c_abi_give_the_wrappers_bits(C, N, ws):
    K, R, M = 768, 19, 17
    W, a, nnz = table(C, ws, 2, K, R)
    x = acts(2, M, K).to(DEV)
    want = run(C, ws, a, K, x, R, 2, torch.bfloat16)
    # rows R + 3 apart inside canaries, two rows more than M behind them
    buf = torch.full([2 * (17 + (M + 2) * (R + 3))], FILL, dtype=torch.uint8, device=DEV).view(torch.bfloat16)
    before = buf.clone()
    view = lambda t: t[17:17 + M * (R + 3)].view(M, R + 3)[:, :R]  # noqa: E731
    C.matmul_sparse_tile(a, K, x, torch.bfloat16, out=view(buf), ws=ws, nnz_bound=nnz, check=True)
    view(before).copy_(want)
    assert torch.equal(bits(buf), bits(before)) and close(want, x, W, 2)
    temp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    for tm, st in ((temp, torch.zeros([1], dtype=torch.uint8, device=DEV)), (None, None)):
        got = torch.zeros_like(want)
        used = torch.ops.dietgpu.matmul_sparse_tile(a, K, x, got, nnz, tm, st)
        assert used >= C.matmul_sparse_tile_scratch_bytes(2, K, R, M, nnz) and (st is None or int(st) == 1)
        assert torch.equal(bits(got), bits(want))
    got, ok = torch.zeros_like(want), torch.zeros([1], dtype=torch.uint8, device=DEV)
    N.check(N.lib().dietgpu_float_matmul_sparse_tile(ws.h, 2, 10, a.data_ptr(), K, R, x.data_ptr(), M, K,
                                                     got.data_ptr(), 0, R, nnz, ctypes.c_void_p(ok.data_ptr()), None))
    torch.cuda.synchronize()
    assert int(ok) == 1 and torch.equal(bits(got), bits(want))


def test_graph_capture_replay(C, ws):
    """Captured once with nnz_bound given, into a workspace the warm-up sized;
    replayed on new x and on new archive bytes of the same shape, each replay
    against the eager call on the same inputs."""
    K, R, M = 1280, 17, 17
    gws = C.Workspace(1 << 20)
    tabs = [table(C, ws, 2, K, R, seed=s) for s in range(4)]
    bound = max(t[2] for t in tabs)
    abuf = torch.zeros([C.max_sparse_float_compressed_size(2, K * R)], dtype=torch.uint8, device=DEV)
    abuf[: tabs[0][1].numel()] = tabs[0][1]
    x = torch.zeros([M, K], dtype=torch.bfloat16, device=DEV)
    out = torch.empty([M, R], dtype=torch.float32, device=DEV)
    ok = torch.empty([1], dtype=torch.uint8, device=DEV)
    call = lambda o, w: C.matmul_sparse_tile(abuf, K, x, torch.bfloat16, out=o, out_status=ok, ws=w,  # noqa: E731
                                             nnz_bound=bound)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        call(out, gws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        call(out, gws)
    for rep in range(3):
        a = tabs[rep + 1][1]
        abuf.zero_()
        abuf[: a.numel()] = a
        x.copy_(acts(2, M + rep + 1, K)[:M])
        eager = torch.empty_like(out)
        call(eager, ws)
        assert close(eager, x, tabs[rep + 1][0], 2)
        for _ in range(2):
            out.fill_(7)
            ok.fill_(7)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert int(ok) == 1 and torch.equal(bits(out), bits(eager)), rep
