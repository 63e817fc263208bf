"""GPU tests of the matmul on a compressed weight table:
codec.matmul_rows, torch.ops.dietgpu.matmul_rows and the C ABI's
dietgpu_float_matmul_rows over k_matmulRows / k_matmulFinish.  Weights and
activations are N(0, 1) cast to the type, archives come from the CPU oracle,
and every table is just over 8 blocks: two workgroups run, the last block is
partial.  The reference is the fp64 product; the tolerance is the standard
bound gamma_K * sum|x w| for K fp32 adds in any order, doubled."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, N, Cache, compress_one, workspace_fixture  # noqa: F401
from tests.util import FT_NAME, NP_WORD, TORCH_FLOAT, TORCH_WORD

pytestmark = pytest.mark.gpu

# (rowWords, R): 16 pieces per block; pieces of 3 segments, rows straddling
# blocks; row edges on block edges (the skipped ids); the row edge moving
# through the block; rows of three pieces
SHAPES = [(256, 150), (768, 50), (4096, 9), (4352, 9), (8448, 5)]
CASES = [(rw, R, ft, M) for rw, R in SHAPES for ft in (1, 2, 3) for M in (1, 3, 8)]
# every instance, a masked remainder, and two, three and eight passes
CASES += [(4352, 9, 2, M) for M in (2, 4, 5, 9, 17, 64)]
FILL = 0xA5

ws = workspace_fixture(16 << 20)
_MADE = Cache()


def table(ft, rw, R, pb=10, head=None, seed=0):
    """(W [R, rw] on the CPU, its oracle archive 16 B-aligned, the same 4 B
    off), made once per key; head: the table's first rows."""
    def make():
        g = torch.Generator().manual_seed(ft * 100003 + rw * 31 + R + 1000 * seed)
        W = torch.randn([R, rw], generator=g).to(TORCH_FLOAT[ft])
        if head is not None:
            W[: head.size(0)] = head
        words = W.view(TORCH_WORD[ft]).numpy().view(NP_WORD[ft]).reshape(-1)
        a = torch.from_numpy(np.asarray(O.float_compress(words, ft, pb, False), dtype=np.uint8).copy()).to(DEV)
        room = torch.zeros([a.numel() + 32], dtype=torch.uint8, device=DEV)
        room[4: 4 + a.numel()] = a
        assert a.data_ptr() % 16 == 0 and room.data_ptr() % 16 == 0
        return W, a, room[4: 4 + a.numel()]
    return _MADE.get((ft, rw, R, pb, head is not None, seed), make)


def acts(ft, M, rw):
    g = torch.Generator().manual_seed(M * 7919 + rw)
    return torch.randn([M, rw], generator=g).to(TORCH_FLOAT[ft])


def close(out, x, W):
    """|out - x W^T| <= rowWords * 2^-23 * (|x| |W|^T), elementwise, in fp64."""
    xd, Wd = x.double().cpu(), W.double()
    err = (out.double().cpu() - xd @ Wd.T).abs()
    return bool((err <= x.size(1) * 2.0 ** -23 * (xd.abs() @ Wd.abs().T)).all())


@pytest.mark.parametrize("rw,R,ft,M", CASES, ids=[f"{rw}x{R}-{FT_NAME[ft]}-M{M}" for rw, R, ft, M in CASES])
def test_against_fp64(C, ws, rw, R, ft, M):
    W, a, _ = table(ft, rw, R)
    x = acts(ft, M, rw).to(DEV)
    out = torch.empty([M, R], dtype=torch.float32, device=DEV)
    _, ok = C.matmul_rows(a, rw, x, TORCH_FLOAT[ft], out=out, ws=ws)
    assert int(ok) == 1 and close(out, x, W)


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_one_rounding(C, ws, ft):
    _, a, _ = table(ft, 4352, 9)
    x = acts(ft, 3, 4352).to(DEV)
    o32 = torch.empty([3, 9], dtype=torch.float32, device=DEV)
    o16 = torch.empty([3, 9], dtype=TORCH_FLOAT[ft], device=DEV)
    C.matmul_rows(a, 4352, x, TORCH_FLOAT[ft], out=o32, ws=ws, check=True)
    C.matmul_rows(a, 4352, x, TORCH_FLOAT[ft], out=o16, ws=ws, check=True)
    assert torch.equal(o16.view(torch.int16), o32.to(TORCH_FLOAT[ft]).view(torch.int16))


@pytest.mark.parametrize("ft", [1, 2, 3], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("rw,R", [(768, 50), (4352, 9)])
def test_exact_indexing(C, ws, rw, R, ft):
    """x[m] = e_k: out[m, r] is W[r, k] itself."""
    W, a, _ = table(ft, rw, R)
    assert bool(((W != 0) & torch.isfinite(W)).all())
    ks = [0, 7, 8, 255, 256, rw - 1]
    x = torch.zeros([len(ks), rw], dtype=TORCH_FLOAT[ft])
    x[range(len(ks)), ks] = 1
    out = torch.empty([len(ks), R], dtype=torch.float32, device=DEV)
    C.matmul_rows(a, rw, x.to(DEV), TORCH_FLOAT[ft], out=out, ws=ws, check=True)
    assert torch.equal(out.cpu(), W[:, ks].float().T)


def test_order_is_the_rows_own(C, ws):
    W9, a9, _ = table(2, 4352, 9)
    _, a30, _ = table(2, 4352, 30, head=W9)
    x = acts(2, 8, 4352).to(DEV)
    run = lambda a, x, R: C.matmul_rows(a, 4352, x, torch.bfloat16, ws=ws, check=True,  # noqa: E731
                                        out=torch.empty([x.size(0), R], dtype=torch.float32, device=DEV))[0]
    o9 = run(a9, x, 9)
    assert torch.equal(o9.view(torch.int32), run(a9, x, 9).view(torch.int32))
    assert torch.equal(o9.view(torch.int32), run(a30, x, 30)[:, :9].view(torch.int32))
    assert torch.equal(o9[:3].view(torch.int32), run(a9, x[:3], 9).view(torch.int32))


@pytest.mark.parametrize("variant", ["strides", "archive-4-off", "pb9", "pb11", "gpu-archive", "side-stream"])
def test_layout(C, ws, variant):
    rw, R, M = 4352, 9, 3
    pb = {"pb9": 9, "pb11": 11}.get(variant, 10)
    W, a16, a4 = table(2, rw, R, pb)
    a = a4 if variant == "archive-4-off" else a16
    if variant == "gpu-archive":
        a = compress_one(C, ws, W.view(torch.int16).to(DEV).reshape(-1), 2, pb=pb, clone=True)
    x = acts(2, M, rw).to(DEV)
    if variant == "strides":  # x rows rw + 8 apart; out R + 3 apart, one word off 16 B, inside canaries
        xs = torch.zeros([M, rw + 8], dtype=torch.bfloat16, device=DEV)
        xs[:, :rw] = x
        buf = torch.full([4 * (17 + M * (R + 3) + 16)], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
        before = buf.clone()
        out = buf[17:17 + M * (R + 3)].view(M, R + 3)[:, :R]
        assert out.data_ptr() % 16 == 4
        C.matmul_rows(a, rw, xs[:, :rw], torch.bfloat16, out=out, ws=ws, check=True)
        want = torch.empty([M, R], dtype=torch.float32, device=DEV)
        C.matmul_rows(a, rw, x, torch.bfloat16, out=want, ws=ws, check=True)
        before[17:17 + M * (R + 3)].view(M, R + 3)[:, :R] = want
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)) and close(want, x, W)
        return
    out = torch.empty([M, R], dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream() if variant == "side-stream" else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _, ok = C.matmul_rows(a, rw, x, torch.bfloat16, out=out, ws=ws, prob_bits=pb)
    stream.synchronize()
    assert int(ok) == 1 and close(out, x, W)


@pytest.mark.parametrize("status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("fault", ["float-type", "prob-bits", "magic", "one-row-more"])
def test_failure_writes_the_status_alone(C, fault, status):
    rw, R, M = 4352, 9, 3
    _, a, _ = table(2, rw, R)
    dtype = torch.float16 if fault == "float-type" else torch.bfloat16
    pb = 9 if fault == "prob-bits" else 10
    rows = R + 1 if fault == "one-row-more" else R
    if fault == "magic":
        a = a.clone()
        a[0] ^= 1
    x = acts(2, M, rw).to(dtype).to(DEV)
    out = torch.full([M, 4 * rows], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    ws = C.Workspace(1 << 20)
    if status:
        _, ok = C.matmul_rows(a, rw, x, dtype, out=out, ws=ws, prob_bits=pb)
        assert int(ok) == 0
        with pytest.raises(C.N.DietGpuError, match="matmul_rows: the archive does not match"):
            C.matmul_rows(a, rw, x, dtype, out=out, ws=ws, prob_bits=pb, check=True)
    else:
        C.N.check(C.N.lib().dietgpu_float_matmul_rows(ws.h, C.FLOAT_TYPE[dtype], pb, a.data_ptr(), rw, rows,
                                                      x.data_ptr(), M, rw, out.data_ptr(), 1, rows, None, None))
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == FILL).all())


def test_operator_and_c_abi_give_the_wrappers_bits(C, N, ws):
    rw, R, M = 4352, 9, 5
    _, a, _ = table(2, rw, R)
    x = acts(2, M, rw).to(DEV)
    want = torch.empty([M, R], dtype=torch.bfloat16, device=DEV)
    C.matmul_rows(a, rw, x, torch.bfloat16, out=want, ws=ws, check=True)
    temp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    for tm, st in ((temp, torch.zeros([1], dtype=torch.uint8, device=DEV)), (None, None)):
        got = torch.zeros_like(want)
        used = torch.ops.dietgpu.matmul_rows(a, rw, x, got, tm, st)
        assert used >= 4 * 3 * (R + 10) and (st is None or int(st) == 1)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    got = torch.zeros_like(want)
    ok = torch.zeros([1], dtype=torch.uint8, device=DEV)
    N.check(N.lib().dietgpu_float_matmul_rows(ws.h, 2, 10, a.data_ptr(), rw, R, x.data_ptr(), M, rw, got.data_ptr(),
                                              0, R, ctypes.c_void_p(ok.data_ptr()), None))
    torch.cuda.synchronize()
    assert int(ok) == 1 and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_graph_capture_replay(C):
    """Captured once; replayed on new x and on new archive bytes of the same
    shape, each replay against the eager call on the same inputs."""
    rw, R, M = 4352, 9, 5
    ws = C.Workspace(1 << 20)
    abuf = torch.zeros([C.max_float_compressed_size(2, rw * R)], dtype=torch.uint8, device=DEV)
    x = torch.zeros([M, rw], dtype=torch.bfloat16, device=DEV)
    out = torch.empty([M, R], dtype=torch.float32, device=DEV)
    ok = torch.empty([1], dtype=torch.uint8, device=DEV)
    abuf[: table(2, rw, R)[1].numel()] = table(2, rw, R)[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.matmul_rows(abuf, rw, x, torch.bfloat16, out=out, out_status=ok, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        C.matmul_rows(abuf, rw, x, torch.bfloat16, out=out, out_status=ok, ws=ws)
    for rep in range(3):
        a = table(2, rw, R, seed=rep + 1)[1]
        abuf.zero_()
        abuf[: a.numel()] = a
        x.copy_(acts(2, M + rep + 1, rw)[:M])
        eager = torch.empty_like(out)
        C.matmul_rows(abuf, rw, x, torch.bfloat16, out=eager, ws=ws)
        for _ in range(2):
            out.fill_(7)
            ok.fill_(7)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert int(ok) == 1 and torch.equal(out.view(torch.int32), eager.view(torch.int32)), rep
