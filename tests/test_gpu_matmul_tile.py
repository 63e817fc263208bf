"""GPU tests of the matmul through the matrix pipe, k_matmulTile,
through codec.matmul_tile, the operator and the C ABI.  Tables, activations and the
bound rowWords * 2^-23 * (|x| |W|^T) against fp64 are test_gpu_matmul_rows'."""
import ctypes

import pytest
import torch

from tests.gpu_harness import C, DEV, N, workspace_fixture  # noqa: F401
from tests.test_gpu_matmul_rows import FILL, acts, close, table
from tests.util import FT_NAME, TORCH_FLOAT

pytestmark = pytest.mark.gpu

# (rowWords, R): every segment a piece; period 3, rows straddling blocks; period 1, a second group with
# one live half; period 2, a full group and a tail of two; period 17, one live half per workgroup
SHAPES = [(256, 150), (768, 50), (4096, 9), (8192, 9), (4352, 9)]
CASES = [(rw, R, ft, M) for rw, R in SHAPES for ft in (1, 2) for M in (5, 17, 64)]
CASES += [(8192, 9, 2, M) for M in (1, 16, 33)]  # a tile exactly full, and one row into the next
# periods 5 (40.6 blocks: a second run starts), 7 and 43 (one live half per group)
CASES += [(rw, R, 2, 17) for rw, R in ((1280, 130), (1792, 94), (11008, 3))]

ws = workspace_fixture(16 << 20)


def run(C, ws, a, rw, x, R, ft=2, dtype=torch.float32, **kw):
    out = torch.empty([x.size(0), R], dtype=dtype, device=DEV)
    C.matmul_tile(a, rw, x, TORCH_FLOAT[ft], out=out, ws=ws, check=True, **kw)
    return out


@pytest.mark.parametrize("rw,R,ft,M", CASES, ids=[f"{rw}x{R}-{FT_NAME[ft]}-M{M}" for rw, R, ft, M in CASES])
def test_against_fp64(C, ws, rw, R, ft, M):
    W, a, _ = table(ft, rw, R)
    x = acts(ft, M, rw).to(DEV)
    assert close(run(C, ws, a, rw, x, R, ft), x, W)  # (check=True: the status byte is 1)


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rw,R", [(768, 50), (8192, 9)])
def test_exact_indexing(C, ws, rw, R, ft):  # x[m] = e_k: out[m, r] is W[r, k] itself
    W, a, _ = table(ft, rw, R)
    ks = [0, 7, 8, 31, 32, 255, 256, rw - 1]
    x = torch.zeros([len(ks), rw], dtype=TORCH_FLOAT[ft])
    x[range(len(ks)), ks] = 1
    assert torch.equal(run(C, ws, a, rw, x.to(DEV), R, ft).cpu(), W[:, ks].float().T)


def test_order_is_the_rows_own(C, ws):
    W9, a9, _ = table(2, 8192, 9)
    _, a30, _ = table(2, 8192, 30, head=W9)
    x = acts(2, 37, 8192).to(DEV)
    o9 = run(C, ws, a9, 8192, x, 9).view(torch.int32)
    assert torch.equal(o9, run(C, ws, a9, 8192, x, 9).view(torch.int32))
    assert torch.equal(o9, run(C, ws, a30, 8192, x, 30)[:, :9].view(torch.int32))
    assert torch.equal(o9[:5], run(C, ws, a9, 8192, x[:5], 9).view(torch.int32))


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_one_rounding(C, ws, ft):
    _, a, _ = table(ft, 8192, 9)
    x = acts(ft, 17, 8192).to(DEV)
    o32, o16 = run(C, ws, a, 8192, x, 9, ft), run(C, ws, a, 8192, x, 9, ft, TORCH_FLOAT[ft])
    assert torch.equal(o16.view(torch.int16), o32.to(TORCH_FLOAT[ft]).view(torch.int16))


@pytest.mark.parametrize("variant", ["strides", "archive-4-off", "pb9", "pb11", "side-stream"])
def test_layout(C, ws, variant):
    rw, R, M = 8192, 9, 19
    pb = {"pb9": 9, "pb11": 11}.get(variant, 10)
    W, a16, a4 = table(2, rw, R, pb)
    a = a4 if variant == "archive-4-off" else a16
    x = acts(2, M, rw).to(DEV)
    if variant == "strides":  # x rows rw + 8 apart; out R + 3 apart, one word off 16 B, inside canaries
        xs = torch.zeros([M, rw + 8], dtype=torch.bfloat16, device=DEV)
        xs[:, :rw] = x
        buf = torch.full([4 * (17 + M * (R + 3) + 16)], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
        before = buf.clone()
        out = buf[17:17 + M * (R + 3)].view(M, R + 3)[:, :R]
        assert out.data_ptr() % 16 == 4
        C.matmul_tile(a, rw, xs[:, :rw], torch.bfloat16, out=out, ws=ws, check=True)
        want = run(C, ws, a, rw, x, R)
        before[17:17 + M * (R + 3)].view(M, R + 3)[:, :R] = want
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)) and close(want, x, W)
        return
    stream = torch.cuda.Stream() if variant == "side-stream" else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = run(C, ws, a, rw, x, R, prob_bits=pb)
    stream.synchronize()
    assert close(out, x, W)


@pytest.mark.parametrize("fault", ["float-type", "prob-bits", "magic", "one-row-more"])
def test_failure_writes_the_status_alone(C, ws, fault):
    rw, R, M = 8192, 9, 19
    _, a, _ = table(2, rw, R)
    dtype, pb = torch.float16 if fault == "float-type" else torch.bfloat16, 9 if fault == "prob-bits" else 10
    rows = R + 1 if fault == "one-row-more" else R
    if fault == "magic":
        a = a.clone()
        a[0] ^= 1
    x = acts(2, M, rw).to(dtype).to(DEV)
    out = torch.full([M, 4 * rows], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    assert int(C.matmul_tile(a, rw, x, dtype, out=out, ws=ws, prob_bits=pb)[1]) == 0
    with pytest.raises(C.N.DietGpuError, match="matmul_tile: the archive does not match"):
        C.matmul_tile(a, rw, x, dtype, out=out, ws=ws, prob_bits=pb, check=True)
    assert bool((out.view(torch.uint8) == FILL).all())


def test_operator_and_c_abi_give_the_wrappers_bits(C, N, ws):
    rw, R, M = 8192, 9, 19
    _, a, _ = table(2, rw, R)
    x = acts(2, M, rw).to(DEV)
    want = run(C, ws, a, rw, x, R, dtype=torch.bfloat16).view(torch.int16)
    temp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    for tm, st in ((temp, torch.zeros([1], dtype=torch.uint8, device=DEV)), (None, None)):
        got = torch.zeros([M, R], dtype=torch.bfloat16, device=DEV)
        used = torch.ops.dietgpu.matmul_tile(a, rw, x, got, tm, st)
        assert used >= 4 * M * (R + 18) and (st is None or int(st) == 1) and torch.equal(got.view(torch.int16), want)
    got, ok = torch.zeros([M, R], dtype=torch.bfloat16, device=DEV), torch.zeros([1], dtype=torch.uint8, device=DEV)
    N.check(N.lib().dietgpu_float_matmul_tile(ws.h, 2, 10, a.data_ptr(), rw, R, x.data_ptr(), M, rw, got.data_ptr(),
                                              0, R, ctypes.c_void_p(ok.data_ptr()), None))
    torch.cuda.synchronize()
    assert int(ok) == 1 and torch.equal(got.view(torch.int16), want)


def test_graph_capture_replay(C):
    """Captured once; each replay, on new x and new archive bytes, against the eager call."""
    rw, R, M = 8192, 9, 19
    ws = C.Workspace(1 << 20)
    abuf = torch.zeros([C.max_float_compressed_size(2, rw * R)], dtype=torch.uint8, device=DEV)
    x = torch.zeros([M, rw], dtype=torch.bfloat16, device=DEV)
    out, ok = torch.empty([M, R], dtype=torch.float32, device=DEV), torch.empty([1], dtype=torch.uint8, device=DEV)
    abuf[: table(2, rw, R)[1].numel()] = table(2, rw, R)[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.matmul_tile(abuf, rw, x, torch.bfloat16, out=out, out_status=ok, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        C.matmul_tile(abuf, rw, x, torch.bfloat16, out=out, out_status=ok, ws=ws)
    for rep in range(3):
        a = table(2, rw, R, seed=rep + 1)[1]
        abuf.zero_()
        abuf[: a.numel()] = a
        x.copy_(acts(2, M + rep + 1, rw)[:M])
        eager = torch.empty_like(out)
        C.matmul_tile(abuf, rw, x, torch.bfloat16, out=eager, ws=ws)
        for _ in range(2):
            out.fill_(7), ok.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            assert int(ok) == 1 and torch.equal(out.view(torch.int32), eager.view(torch.int32)), rep
