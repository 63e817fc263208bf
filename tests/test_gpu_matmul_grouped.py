"""GPU tests of the grouped matmul on compressed expert tables: k_matmulGroupPlan,
k_matmulTileGrouped and k_matmulFinishGrouped through codec.matmul_grouped, the operator and the C ABI.
Tables, activations and the bound rowWords * 2^-23 * (|x| |W|^T) against fp64 are test_gpu_matmul_rows';
expert e's table is table(ft, rw, R, seed=e).  out lies inside a canary row on either side and x holds
TAIL rows past offsets[E]."""
import ctypes
from itertools import accumulate

import pytest
import torch

from tests.gpu_harness import C, DEV, N, Cache, workspace_fixture  # noqa: F401
from tests.test_gpu_matmul_rows import FILL, acts, close, table
from tests.util import FT_NAME, TORCH_FLOAT

pytestmark = pytest.mark.gpu

# (rowWords, R): every segment a piece, 2 task groups; period 3; period 2 with a tail
SHAPES = [(256, 150), (768, 50), (8192, 9)]
# rows per expert: mixed; one expert alone; one expert chunked 64 + 6 and one exactly full
ROUTINGS = [[5, 0, 17, 1], [0, 0, 3, 0], [70, 0, 64, 1]]
CASES = [(rw, R, ft, i) for rw, R in SHAPES for ft in (1, 2) for i in range(len(ROUTINGS))]
IDS = [f"{rw}x{R}-{FT_NAME[ft]}-r{i}" for rw, R, ft, i in CASES]
TAIL = 2

ws = workspace_fixture(16 << 20)
_RUNS = Cache()


def offsets_of(counts, dtype=torch.int64):
    return torch.tensor([0] + list(accumulate(counts)), dtype=dtype, device=DEV)


def experts(C, ft, rw, R, counts, pb=10, four_off=None):
    """(the tables, their archives, the address tensor, x with TAIL rows past the last expert's)"""
    tabs = [table(ft, rw, R, pb, seed=e) for e in range(len(counts))]
    arch = [t[2] if e == four_off else t[1] for e, t in enumerate(tabs)]
    return [t[0] for t in tabs], arch, C.archive_ptrs(arch), acts(ft, sum(counts) + TAIL, rw).to(DEV)


def run(C, ws, ptrs, rw, x, offs, R, ft=2, dtype=torch.float32, **kw):
    """(out inside its canary rows, ok): buf[0] and buf[-1] are the canaries, buf[1 + t] is out[t]"""
    T = x.size(0)
    buf = torch.full([T + 2, R * dtype.itemsize], FILL, dtype=torch.uint8, device=DEV).view(dtype)
    ok = C.matmul_grouped(ptrs, rw, x, offs, TORCH_FLOAT[ft], out=buf[1:T + 1], ws=ws, **kw)[1]
    return buf, ok


def untouched(rows):
    return bool((rows.contiguous().view(torch.uint8) == FILL).all())


def served(C, ws, rw, R, ft, i):  # the grouped call of a case, made once
    def make():
        Ws, arch, ptrs, x = experts(C, ft, rw, R, ROUTINGS[i])
        buf, ok = run(C, ws, ptrs, rw, x, offsets_of(ROUTINGS[i]), R, ft)
        return Ws, arch, ptrs, x, buf, ok
    return _RUNS.get((rw, R, ft, i), make)


@pytest.mark.parametrize("rw,R,ft,i", CASES, ids=IDS)
def test_against_fp64(C, ws, rw, R, ft, i):
    Ws, _, _, x, buf, ok = served(C, ws, rw, R, ft, i)
    lo = 0
    for e, cnt in enumerate(ROUTINGS[i]):
        assert close(buf[1 + lo:1 + lo + cnt], x[lo:lo + cnt], Ws[e]), e
        lo += cnt
    assert ok.tolist() == [1] * len(Ws) and untouched(buf[0]) and untouched(buf[1 + lo:])


@pytest.mark.parametrize("rw,R,ft,i", CASES, ids=IDS)
def test_bits_are_matmul_tiles_chunk_by_chunk(C, ws, rw, R, ft, i):
    _, arch, _, x, buf, _ = served(C, ws, rw, R, ft, i)
    offs = [0] + list(accumulate(ROUTINGS[i]))
    for e, cnt in enumerate(ROUTINGS[i]):
        for lo in range(offs[e], offs[e] + cnt, 64):
            hi = min(lo + 64, offs[e + 1])
            want = torch.empty([hi - lo, R], dtype=torch.float32, device=DEV)
            C.matmul_tile(arch[e], rw, x[lo:hi], TORCH_FLOAT[ft], out=want, ws=ws, check=True)
            assert torch.equal(buf[1 + lo:1 + hi].view(torch.int32), want.view(torch.int32)), (e, lo)


@pytest.mark.parametrize("rw,R,ft,i", [c for c in CASES if c[2] == 2], ids=[s for s in IDS if "bf16" in s])
def test_one_workgroup_crossing_entries(C, ws, rw, R, ft, i):
    """1, 2 and 3 workgroups for the whole task line: each rebuilds its table from entry to entry."""
    _, _, ptrs, x, buf, _ = served(C, ws, rw, R, ft, i)
    try:
        for cap in (1, 2, 3):
            C.set_matmul_grouped_grid(cap)
            got, ok = run(C, ws, ptrs, rw, x, offsets_of(ROUTINGS[i]), R, ft)
            assert bool(ok.all()) and torch.equal(got.view(torch.int32), buf.view(torch.int32)), cap
    finally:
        C.set_matmul_grouped_grid(0)


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rw,R", [(768, 50), (8192, 9)])
def test_exact_indexing(C, ws, rw, R, ft):  # x[t] = e_k: out[t, r] is W_e[r, k] itself
    counts, ks = [3, 0, 5, 0], [0, 7, 8, 31, 32, 255, 256, rw - 1]
    Ws, _, ptrs, _ = experts(C, ft, rw, R, counts)
    x = torch.zeros([len(ks), rw], dtype=TORCH_FLOAT[ft])
    x[range(len(ks)), ks] = 1
    buf, _ = run(C, ws, ptrs, rw, x.to(DEV), offsets_of(counts), R, ft, check=True)
    want = torch.cat([Ws[0][:, ks[:3]].float().T, Ws[2][:, ks[3:]].float().T])
    assert torch.equal(buf[1:-1].cpu(), want)


def test_one_bad_expert(C, ws):
    rw, R, ft, i = 768, 50, 2, 0
    _, arch, _, x, good, _ = served(C, ws, rw, R, ft, i)
    broken = arch[2].clone()
    broken[0] ^= 1  # the magic word
    ptrs = C.archive_ptrs(arch[:2] + [broken] + arch[3:])
    buf, ok = run(C, ws, ptrs, rw, x, offsets_of(ROUTINGS[i]), R, ft)
    assert ok.tolist() == [1, 1, 0, 1] and untouched(buf[1 + 5:1 + 22])
    keep = [t for t in range(buf.size(0)) if not 6 <= t < 23]
    assert torch.equal(buf[keep].view(torch.int32), good[keep].view(torch.int32))
    with pytest.raises(C.N.DietGpuError, match=r"matmul_grouped: archive\(s\) \[2\] do not match"):
        run(C, ws, ptrs, rw, x, offsets_of(ROUTINGS[i]), R, ft, check=True)


def test_rows_come_from_archive_0_without_out(C, ws):
    rw, R, ft, i = 768, 50, 2, 0
    _, arch, ptrs, x, good, _ = served(C, ws, rw, R, ft, i)
    out, ok = C.matmul_grouped(ptrs, rw, x, offsets_of(ROUTINGS[i]), torch.bfloat16, out_dtype=torch.float32, ws=ws)
    assert list(out.shape) == [x.size(0), R] and bool(ok.all())
    assert torch.equal(out[:23].view(torch.int32), good[1:24].view(torch.int32))
    broken = arch[0].clone()
    broken[8] ^= 3  # the float type
    with pytest.raises(C.N.DietGpuError, match="archive 0 is no torch.bfloat16 archive"):
        C.matmul_grouped(C.archive_ptrs([broken] + arch[1:]), rw, x, offsets_of(ROUTINGS[i]), torch.bfloat16, ws=ws)


@pytest.mark.parametrize("rw,R", [(256, 150), (768, 50)])
def test_rows_below_the_first_offset_are_untouched(C, ws, rw, R):
    """offsets[0] = 2: no expert owns rows 0 and 1, and the rest carry matmul_tile's bits."""
    _, arch, ptrs, x, _, _ = served(C, ws, rw, R, 2, 0)  # 23 + TAIL rows
    offs = [2, 7, 7, 24, 25]
    buf, ok = run(C, ws, ptrs, rw, x, torch.tensor(offs, dtype=torch.int64, device=DEV), R)
    assert ok.tolist() == [1] * 4 and untouched(buf[:3]) and untouched(buf[-1])
    for e in (0, 2, 3):
        want = torch.empty([offs[e + 1] - offs[e], R], dtype=torch.float32, device=DEV)
        C.matmul_tile(arch[e], rw, x[offs[e]:offs[e + 1]], torch.bfloat16, out=want, ws=ws, check=True)
        assert torch.equal(buf[1 + offs[e]:1 + offs[e + 1]].view(torch.int32), want.view(torch.int32)), e


@pytest.mark.parametrize("offs", [[0, 5, 3, 22, 23], [0, 5, 5, 22, 26], [-1, 5, 5, 22, 23]],
                         ids=["decreasing", "past-T", "negative"])
def test_bad_offsets_write_the_statuses_alone(C, ws, offs):
    rw, R, ft = 768, 50, 2
    _, _, ptrs, x, _, _ = served(C, ws, rw, R, ft, 0)  # T = 23 + TAIL
    offs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    buf, ok = run(C, ws, ptrs, rw, x, offs, R, ft)
    assert ok.tolist() == [0] * 4 and untouched(buf)
    with pytest.raises(C.N.DietGpuError, match="matmul_grouped: the offsets are not ascending"):
        run(C, ws, ptrs, rw, x, offs, R, ft, check=True)


@pytest.mark.parametrize("variant", ["int32-offsets", "archive-4-off", "pb9", "pb11", "own-dtype"])
def test_variants(C, ws, variant):
    rw, R, ft, counts = 768, 50, 2, ROUTINGS[0]
    pb = {"pb9": 9, "pb11": 11}.get(variant, 10)
    Ws, _, ptrs, x = experts(C, ft, rw, R, counts, pb, four_off=2 if variant == "archive-4-off" else None)
    offs = offsets_of(counts, torch.int32 if variant == "int32-offsets" else torch.int64)
    dtype = torch.bfloat16 if variant == "own-dtype" else torch.float32
    buf, ok = run(C, ws, ptrs, rw, x, offs, R, ft, dtype, prob_bits=pb)
    assert bool(ok.all()) and untouched(buf[0]) and untouched(buf[24:])
    if variant == "archive-4-off":  # one workgroup crossing from an aligned archive into the 4 B-off one and out of it
        try:
            C.set_matmul_grouped_grid(1)
            assert torch.equal(run(C, ws, ptrs, rw, x, offs, R, ft)[0].view(torch.int32), buf.view(torch.int32))
        finally:
            C.set_matmul_grouped_grid(0)
    if pb != 10:
        spans = [(0, 5), (5, 5), (5, 22), (22, 23)]
        assert all(close(buf[1 + lo:1 + hi], x[lo:hi], Ws[e]) for e, (lo, hi) in enumerate(spans))
        return
    want = served(C, ws, rw, R, ft, 0)[4][1:24]  # the int64, 16 B-aligned, fp32 call
    assert torch.equal(buf[1:24].view(torch.int16), want.to(dtype).view(torch.int16))


def test_operator_and_c_abi_give_the_wrappers_bits(C, N, ws):
    rw, R, ft, counts = 768, 50, 2, ROUTINGS[0]
    _, _, ptrs, x, buf, _ = served(C, ws, rw, R, ft, 0)
    T, offs, want = x.size(0), offsets_of(counts), buf[1:-1].view(torch.int32)
    temp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    need = N.lib().dietgpu_float_matmul_grouped_scratch_bytes(4, rw, R, T)
    for tm, st in ((temp, torch.zeros([4], dtype=torch.uint8, device=DEV)), (None, None)):
        got = torch.full([T, 4 * R], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
        used = torch.ops.dietgpu.matmul_grouped(ptrs, rw, x, offs, got, tm, st)
        assert used >= need > 4 * T * R and (st is None or st.tolist() == [1] * 4)
        assert torch.equal(got.view(torch.int32), want)
    got = torch.full([T, 4 * R], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    ok = torch.zeros([4], dtype=torch.uint8, device=DEV)
    N.check(N.lib().dietgpu_float_matmul_grouped(ws.h, 2, 10, ptrs.data_ptr(), 4, rw, R, x.data_ptr(), T, rw,
                                                 offs.data_ptr(), 1, got.data_ptr(), 1, R,
                                                 ctypes.c_void_p(ok.data_ptr()), None))
    torch.cuda.synchronize()
    assert ok.tolist() == [1] * 4 and torch.equal(got.view(torch.int32), want)


def test_graph_capture_replay(C):
    """Captured once; each replay, on new offsets, new x and new archive bytes, against the eager call.
    Expert 1 goes from no rows to nine and back."""
    rw, R, T = 768, 50, 25
    ws = C.Workspace(1 << 20)
    tabs = [table(2, rw, R, seed=e)[1] for e in range(4)]
    abufs = [torch.zeros([C.max_float_compressed_size(2, rw * R)], dtype=torch.uint8, device=DEV) for _ in range(4)]
    ptrs = C.archive_ptrs(abufs)
    x = torch.zeros([T, rw], dtype=torch.bfloat16, device=DEV)
    offs = torch.zeros([5], dtype=torch.int64, device=DEV)
    out, ok = torch.empty([T, R], dtype=torch.float32, device=DEV), torch.empty([4], dtype=torch.uint8, device=DEV)

    def load(rep, counts):
        for e in range(4):
            a = tabs[(e + rep) % 4]
            abufs[e].zero_()
            abufs[e][: a.numel()] = a
        x.copy_(acts(2, T + rep, rw)[:T])
        offs.copy_(offsets_of(counts))

    call = lambda o, s: C.matmul_grouped(ptrs, rw, x, offs, torch.bfloat16, out=o, out_status=s, ws=ws)  # noqa: E731
    load(0, ROUTINGS[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        call(out, ok)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        call(out, ok)
    for rep, counts in enumerate([ROUTINGS[0], [2, 9, 0, 12], [0, 0, 25, 0], ROUTINGS[0]]):
        load(rep, counts)
        eager = torch.full_like(out, 7)
        call(eager, None)
        for _ in range(2):
            out.fill_(7), ok.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            assert ok.tolist() == [1] * 4 and torch.equal(out.view(torch.int32), eager.view(torch.int32)), rep
