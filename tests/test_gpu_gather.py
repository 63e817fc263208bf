"""GPU tests of the row gather with device-resident indices:
codec.gather_rows_device, torch.ops.dietgpu.gather_rows and the C ABI's
dietgpu_*_gather_rows over k_gather.  The codec is lossless, so the expected
output is words[: R * rw].reshape(R, rw)[idx], compared bit for bit on integer
views.  Every destination lies inside a 0xA5-filled buffer with 16 canary
words on each side; the whole buffer is compared, so a stray write, a write
into the gap of a wider stride or any write to a failing row fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gather_cases as G
from tests.gpu_harness import (C, DEV, N, Cache, compress_one, make_words, to_dev,  # noqa: F401
                               workspace_fixture)
from tests.util import FT_IDS, NP_W, TORCH_OUT, TORCH_WORD, WORD_BYTES, float_words

pytestmark = pytest.mark.gpu

FTS = [0, 1, 2, 3, 4]  # ft 0 = the byte codec
CANARY = 16  # words on each side of the destination
FILL = 0xA5  # byte pattern of canaries, gaps and untouched rows
IDX_T = {32: torch.int32, 64: torch.int64}

ws = workspace_fixture(64 << 20)
_TABLES = Cache()


def table(C, ws, ft, kind="normal", pb=10, checksum=False, n=G.N_TABLE):
    """(words on the device as integers, archive, the archive 4 bytes off 16 B
    alignment), computed once per key and left unchanged."""
    def make():
        t = to_dev(make_words(ft, n, kind, seed=ft + 3), ft)
        a = compress_one(C, ws, t, ft, pb, checksum)
        shifted = torch.empty([a.numel() + 16], dtype=torch.uint8, device=DEV)
        assert shifted.data_ptr() % 16 == 0
        shifted[4: 4 + a.numel()] = a
        return t, a, shifted[4: 4 + a.numel()]
    return _TABLES.get((ft, kind, pb, checksum, n), make)


def idx_tensor(idx, bits):
    return torch.tensor(idx, dtype=IDX_T[bits], device=DEV).reshape(len(idx))


def expect_ok(idx, rw, n=G.N_TABLE):
    return [int(0 <= v and (v + 1) * rw <= n) for v in idx]


class Dest:
    """numIdx rows of rw words at `stride`, starting `off` words past a 16 B
    boundary inside a FILL-ed buffer, 16 canary words on each side; and the
    buffer as it must look afterwards."""

    def __init__(self, ft, words, rw, idx, off=0, pad=0, ok=None, n=G.N_TABLE):
        wb = WORD_BYTES[ft]
        per16 = 16 // wb
        m = len(idx)
        self.stride = rw + pad
        self.start = -(-CANARY // per16) * per16 + off
        total = self.start + m * self.stride + CANARY + per16
        self.buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(TORCH_WORD[ft])
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.view(self.buf, m, rw).view(TORCH_OUT[ft])
        assert m == 0 or (self.out.data_ptr() % 16 == 0) == (off % per16 == 0)
        self.want = self.buf.clone()
        self.ok = expect_ok(idx, rw, n) if ok is None else ok
        good = torch.tensor(self.ok, dtype=torch.bool, device=DEV)
        if m and bool(good.any()):
            R = n // rw
            rows = torch.tensor([v if g else 0 for v, g in zip(idx, self.ok)], dtype=torch.int64, device=DEV)
            self.view(self.want, m, rw)[good] = words[: R * rw].view(R, rw)[rows[good]]

    def view(self, buf, m, rw):
        return buf.as_strided((m, rw), (self.stride, 1), self.start)

    def check(self, status=None, what=""):
        torch.cuda.synchronize()
        if status is not None:
            assert status.cpu().reshape(-1).tolist() == self.ok, what
        if not torch.equal(self.buf, self.want):
            bad = torch.nonzero(self.buf != self.want).reshape(-1)
            raise AssertionError(f"{what}: {bad.numel()} words differ, first at buffer word {int(bad[0])} "
                                 f"(rows start at {self.start}, stride {self.stride})")


def gather(C, ws, ft, arch, rw, idx_t, dest, pb=10, **kw):
    status = torch.full([idx_t.numel()], 7, dtype=torch.uint8, device=DEV)
    out, ok = C.gather_rows_device(arch, rw, idx_t, TORCH_OUT[ft], out=dest.out, out_status=status, prob_bits=pb, ws=ws,
                                   **kw)
    assert out is dest.out and ok is status
    return status


# (output offset in words, stride padding, archive 4 B off)
PLACEMENTS = [(off, pad, shifted) for off in (0, 1) for pad in (0, 3) for shifted in (False, True)]


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
@pytest.mark.parametrize("rw", G.ROW_WORDS)
def test_index_lists(C, ws, ft, rw):
    """Every index list of the width, int32 and int64 indices, on every
    placement: output base 16 B-aligned and one word off, stride rw and rw + 3,
    archive 16 B-aligned and 4 B off."""
    words, a16, a4 = table(C, ws, ft)
    for name, (idx, _) in G.index_lists(rw).items():
        for off, pad, shifted in PLACEMENTS:
            for bits in (32, 64):
                dest = Dest(ft, words, rw, idx, off, pad)
                assert all(dest.ok)
                status = gather(C, ws, ft, a4 if shifted else a16, rw, idx_tensor(idx, bits), dest)
                dest.check(status, f"{name} off {off} pad {pad} shifted {shifted} int{bits}")


@pytest.mark.parametrize("bits", [32, 64])
def test_more_task_groups_than_resident_workgroups(C, ws, bits):
    """70,000 indices at 8 words: the workgroups stride over the task groups."""
    words, a16, _ = table(C, ws, 2)
    idx = G.long_list()
    dest = Dest(2, words, G.LONG_RW, idx, off=0, pad=0)
    status = gather(C, ws, 2, a16, G.LONG_RW, idx_tensor(idx, bits), dest)
    dest.check(status, "long list")


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
@pytest.mark.parametrize("rw", [1, 8, 257, 4096, 9000])
@pytest.mark.parametrize("bits", [32, 64])
def test_failing_rows_in_a_mixed_list(C, N, ws, ft, rw, bits):
    """-1, R, R + 5 (and 2^31, 2^40, INT64_MIN as int64) give status 0 and
    leave their rows untouched; their neighbours come out exact.  With and
    without a status array."""
    words, a16, a4 = table(C, ws, ft)
    idx, ok = G.mixed_list(rw, wide=bits == 64)
    for off, pad, arch in ((0, 0, a16), (1, 3, a4)):
        dest = Dest(ft, words, rw, idx, off, pad)
        assert dest.ok == ok
        status = gather(C, ws, ft, arch, rw, idx_tensor(idx, bits), dest)
        dest.check(status, "with status")
        # no status array: the C ABI with a null pointer
        dest = Dest(ft, words, rw, idx, off, pad)
        c_abi(N, ws, ft, arch, rw, idx_tensor(idx, bits), dest, None)
        dest.check(None, "without status")


def c_abi(N, ws, ft, arch, rw, idx_t, dest, status, pb=10):
    tail = (arch.data_ptr(), rw, idx_t.numel(), idx_t.data_ptr(), int(idx_t.dtype == torch.int64),
            dest.out.data_ptr(), dest.stride, status.data_ptr() if status is not None else None,
            torch.cuda.current_stream().cuda_stream)
    if ft == 0:
        rc = N.lib().dietgpu_ans_gather_rows(ws.h, pb, *tail)
    else:
        rc = N.lib().dietgpu_float_gather_rows(ws.h, ft, pb, *tail)
    assert rc == N.DIETGPU_OK, N.lib().dietgpu_last_error()


def empty_archive(ft, pb=10):
    """An element of 0 words, from the CPU oracle."""
    w = np.zeros(0, dtype=NP_W[ft])
    a = O.ans_encode(w, pb) if ft == 0 else O.float_compress(w, ft, pb)
    return torch.from_numpy(np.asarray(a, dtype=np.uint8).copy()).to(DEV)


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
@pytest.mark.parametrize("how", ["other_type", "other_prob_bits", "corrupt_magic", "inner_magic", "zero_words"])
def test_failing_archive(C, ws, ft, how):
    """Every status is 0 and nothing is written."""
    words, a16, _ = table(C, ws, ft)
    call_ft, pb, arch = ft, 10, a16
    if how == "other_type":
        if ft == 0:
            arch = table(C, ws, 2)[1]   # a float archive read as bytes
        else:
            call_ft = {1: 2, 2: 1, 3: 4, 4: 3}[ft]
    elif how == "other_prob_bits":
        pb = 11
    elif how == "corrupt_magic":
        arch = a16.clone()
        arch[0] ^= 1
    elif how == "inner_magic":
        # the ANS archive inside a float archive (the byte archive's only magic
        # is its first word: flip a higher bit of it instead)
        arch = a16.clone()
        if ft == 0:
            arch[3] ^= 0x40
        else:
            n = G.N_TABLE
            n4, n8, n16 = -(-n // 4) * 4, -(-n // 8) * 8, -(-n // 16) * 16
            raw = {1: n16, 2: n16, 3: 2 * n8 + n16, 4: 4 * n4 + 2 * n8}[ft]
            arch[32 + raw] ^= 1
    else:
        arch = empty_archive(ft)
    for rw, idx in ((8, [0, 1, 2, 5000, 17]), (9000, [0, 6, 3]), (1, [0])):
        for bits in (32, 64):
            dest = Dest(call_ft, words, rw, idx, off=0, pad=0, ok=[0] * len(idx))
            status = gather(C, ws, call_ft, arch, rw, idx_tensor(idx, bits), dest, pb=pb)
            dest.check(status, f"{how} rw {rw}")


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, ft, pb):
    words, a16, a4 = table(C, ws, ft, pb=pb)
    for rw in (64, 257, 9000):
        idx = G.index_lists(rw)["random"][0][:100] + G.index_lists(rw)["edges"][0]
        for arch, off in ((a16, 0), (a4, 1)):
            dest = Dest(ft, words, rw, idx, off=off, pad=0)
            status = gather(C, ws, ft, arch, rw, idx_tensor(idx, 64), dest, pb=pb)
            dest.check(status, f"pb {pb} rw {rw}")


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
def test_incompressible_content_refills_the_ring(C, ws, ft):
    """Uniformly random bit patterns: blocks of more than 512 compressed words."""
    words, a16, a4 = table(C, ws, ft, kind="uniform")
    for rw in (8, 1024, 4097):
        idx = G.index_lists(rw)["random"][0][:200] + G.index_lists(rw)["edges"][0]
        for arch, off, pad in ((a16, 0, 0), (a4, 1, 3)):
            dest = Dest(ft, words, rw, idx, off=off, pad=pad)
            status = gather(C, ws, ft, arch, rw, idx_tensor(idx, 32), dest)
            dest.check(status, f"uniform rw {rw}")


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
def test_archive_from_the_cpu_oracle(C, ws, ft):
    w = make_words(ft, G.N_TABLE, seed=40 + ft)
    a = O.ans_encode(w, 10) if ft == 0 else O.float_compress(w, ft, 10)
    arch = torch.from_numpy(np.asarray(a, dtype=np.uint8).copy()).to(DEV)
    words = to_dev(w, ft)
    for rw in (7, 1024, 9000):
        idx = G.index_lists(rw)["random"][0][:100] + G.index_lists(rw)["edges"][0]
        dest = Dest(ft, words, rw, idx)
        status = gather(C, ws, ft, arch, rw, idx_tensor(idx, 64), dest)
        dest.check(status, f"oracle rw {rw}")


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
def test_checksummed_archive_decodes_normally(C, ws, ft):
    words, a16, _ = table(C, ws, ft, checksum=True)
    for rw in (64, 4097):
        idx = G.index_lists(rw)["random"][0][:100] + G.index_lists(rw)["edges"][0]
        dest = Dest(ft, words, rw, idx)
        status = gather(C, ws, ft, a16, rw, idx_tensor(idx, 32), dest)
        dest.check(status, f"checksummed rw {rw}")


def test_side_stream(C, ws):
    words, a16, _ = table(C, ws, 2)
    rw = 257
    idx = G.index_lists(rw)["random"][0]
    dest = Dest(2, words, rw, idx, off=1, pad=3)
    it = idx_tensor(idx, 64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        status = gather(C, ws, 2, a16, rw, it, dest)
    side.synchronize()
    dest.check(status, "side stream")


@pytest.mark.parametrize("ft", [0, 2], ids=FT_IDS.get)
def test_no_indices(C, N, ws, ft):
    words, a16, _ = table(C, ws, ft)
    for bits in (32, 64):
        dest = Dest(ft, words, 64, [])
        it = torch.empty([0], dtype=IDX_T[bits], device=DEV)
        out, ok = C.gather_rows_device(a16, 64, it, TORCH_OUT[ft], ws=ws)
        assert tuple(out.shape) == (0, 64) and tuple(ok.shape) == (0,)
        c_abi(N, ws, ft, a16, 64, it, dest, None)
        dest.check(None, "no indices")


def test_index_tensor_of_any_shape_and_a_strided_out(C, ws):
    words, a16, _ = table(C, ws, 3)
    rw, R = 64, G.rows_of(64)
    idx = torch.tensor(G.index_lists(rw)["random"][0][:24], dtype=torch.int64, device=DEV).reshape(2, 3, 4)
    want = words[: R * rw].view(R, rw)[idx.reshape(-1)].view(2, 3, 4, rw)
    out, ok = C.gather_rows_device(a16, rw, idx, torch.float32, ws=ws)
    assert tuple(out.shape) == (2, 3, 4, rw) and tuple(ok.shape) == (2, 3, 4) and bool(ok.all())
    assert torch.equal(out.view(torch.int32), want)
    # a column block of a wider matrix: rows at stride 200, 16 B-aligned or not
    for col in (0, 3):
        wide = torch.full([24, 200], -1.0, dtype=torch.float32, device=DEV)
        keep = wide.clone()
        view = wide[:, col: col + rw]
        out, ok = C.gather_rows_device(a16, rw, idx.reshape(24), torch.float32, out=view, ws=ws)
        assert out is view and bool(ok.all())
        keep[:, col: col + rw] = want.view(24, rw).view(torch.float32)
        assert torch.equal(wide.view(torch.int32), keep.view(torch.int32))
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        C.gather_rows_device(a16, rw, idx.reshape(24), torch.float32,
                             out=torch.empty([24, 2 * rw], dtype=torch.float32, device=DEV)[:, ::2], ws=ws)
    with pytest.raises(ValueError, match="of shape"):
        C.gather_rows_device(a16, rw, idx, torch.float32, out=torch.empty([24, rw], dtype=torch.float32, device=DEV),
                             ws=ws)


def test_graph_capture_replay(C):
    """Captured once; replayed after new indices were written into the same
    index tensor and new archive bytes into the same archive buffer."""
    n, rw, m = G.N_TABLE, 257, 300
    R = n // rw
    ws = C.Workspace(16 << 20)
    x = torch.empty([n], dtype=torch.bfloat16, device=DEV)
    abuf = torch.zeros([C.max_float_compressed_size(2, n)], dtype=torch.uint8, device=DEV)
    idx = torch.zeros([m], dtype=torch.int64, device=DEV)
    out = torch.empty([m, rw], dtype=torch.bfloat16, device=DEV)
    ok = torch.empty([m], dtype=torch.uint8, device=DEV)

    def load(seed):
        """New table, new archive bytes in abuf, new indices (two of them bad)."""
        w = to_dev(float_words(2, n, seed=seed, scale=1 + seed % 3), 2)
        a = compress_one(C, ws, w, 2)
        abuf.zero_()
        abuf[: a.numel()] = a
        rows = torch.from_numpy(np.random.default_rng(seed).integers(0, R, m))
        rows[seed % m] = R + seed
        rows[(seed + 7) % m] = -1 - seed
        idx.copy_(rows)
        good = (rows >= 0) & (rows < R)
        return w, rows.to(DEV), good.to(DEV)

    load(1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.gather_rows_device(abuf, rw, idx, torch.bfloat16, out=out, out_status=ok, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        C.gather_rows_device(abuf, rw, idx, torch.bfloat16, out=out, out_status=ok, ws=ws)
    for rep in range(3):
        w, rows, good = load(100 + rep)
        out.view(torch.int16).fill_(0x5A5A)
        ok.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ok, good.to(torch.uint8)), f"replay {rep}"
        want = torch.full([m, rw], 0x5A5A, dtype=torch.int16, device=DEV)
        want[good] = w[: R * rw].view(R, rw)[rows[good]]
        assert torch.equal(out.view(torch.int16), want), f"replay {rep}"


@pytest.mark.parametrize("as_float", [True, False], ids=["float", "bytes"])
def test_torch_operator(C, ws, as_float):
    ft = 2 if as_float else 0
    words, a16, a4 = table(C, ws, ft)
    op = torch.ops.dietgpu.gather_rows
    rw = 257
    idx, ok = G.mixed_list(rw, wide=True)
    tmp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    for temp_mem, with_status, arch, off, pad in ((None, False, a16, 0, 0), (tmp, True, a4, 1, 3),
                                                  (None, True, a16, 0, 3), (tmp, False, a4, 1, 0)):
        dest = Dest(ft, words, rw, idx, off, pad)
        status = torch.full([len(idx)], 7, dtype=torch.uint8, device=DEV) if with_status else None
        used = op(as_float, arch, rw, idx_tensor(idx, 64), dest.out, temp_mem, status)
        assert isinstance(used, int) and used >= 0
        dest.check(status, "operator")
    # the guards that need device tensors, each with its own message
    i64 = idx_tensor([0, 1], 64)
    o = torch.empty([2, rw], dtype=TORCH_OUT[ft], device=DEV)
    with pytest.raises(RuntimeError, match="compressed inputs must be 4-byte aligned"):
        shifted = torch.empty([a16.numel() + 16], dtype=torch.uint8, device=DEV)
        op(as_float, shifted[1: 1 + a16.numel()], rw, i64, o)
    with pytest.raises(RuntimeError, match="at least the 32-byte archive header"):
        op(as_float, a16[:16], rw, i64, o)
    with pytest.raises(RuntimeError, match="compressed inputs must be contiguous GPU tensors on one device"):
        op(as_float, a16.cpu(), rw, i64, o)
    with pytest.raises(RuntimeError, match="t_out must be on the archive's device"):
        op(as_float, a16, rw, i64, o.cpu())
    with pytest.raises(RuntimeError, match="out_status must have 2 entries"):
        op(as_float, a16, rw, i64, o, None, torch.empty([3], dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
def test_c_abi_through_ctypes(C, N, ws, ft):
    words, a16, a4 = table(C, ws, ft)
    for rw, bits, arch, off, pad in ((64, 32, a16, 0, 0), (4097, 64, a4, 1, 3)):
        idx, _ = G.mixed_list(rw, wide=bits == 64)
        dest = Dest(ft, words, rw, idx, off, pad)
        status = torch.full([len(idx)], 7, dtype=torch.uint8, device=DEV)
        c_abi(N, ws, ft, arch, rw, idx_tensor(idx, bits), dest, status)
        dest.check(status, "C ABI")
    # an archive off 4 B alignment is refused by the call, nothing is launched
    odd = torch.empty([a16.numel() + 16], dtype=torch.uint8, device=DEV)[2: 2 + a16.numel()]
    first = Dest(ft, words, 64, [0, 1])
    it = idx_tensor([0, 1], 32)
    tail = (odd.data_ptr(), 64, 2, it.data_ptr(), 0, first.out.data_ptr(), 64, None, None)
    rc = (N.lib().dietgpu_ans_gather_rows(ws.h, 10, *tail) if ft == 0
          else N.lib().dietgpu_float_gather_rows(ws.h, ft, 10, *tail))
    assert rc == N.DIETGPU_ERR_INVALID and b"must be 4-byte aligned" in N.lib().dietgpu_last_error()
    torch.cuda.synchronize()
    dest = Dest(ft, words, 64, [0, 1], ok=[0, 0])  # (its `want`: an untouched buffer)
    dest.buf = first.buf
    dest.check(None, "refused call")


@pytest.mark.parametrize("ft", [0, 2, 4], ids=FT_IDS.get)
def test_config_with_checksum_is_rejected(C, N, ws, ft):
    """The C++ entry points refuse a config with useChecksum set (the C ABI and
    the Python / torch layers have no such flag, so this goes through the
    test-hook library, which calls the C++ functions)."""
    words, a16, _ = table(C, ws, ft)
    T = N.testlib()
    idx = [3, 0, 5]
    it = idx_tensor(idx, 64)
    stream = torch.cuda.current_stream().cuda_stream
    dest = Dest(ft, words, 64, idx, ok=[0, 0, 0])
    status = torch.full([3], 7, dtype=torch.uint8, device=DEV)
    rc = T.dietgpu_test_gather_config(ws.h, ft, 1, a16.data_ptr(), 64, 3, it.data_ptr(), dest.out.data_ptr(),
                                      status.data_ptr(), stream)
    assert rc == N.DIETGPU_ERR_INVALID
    assert b"checksum" in T.dietgpu_test_last_error()
    dest.check(None, "rejected config")
    assert status.cpu().tolist() == [7, 7, 7]
    # the same call without the flag gathers
    dest = Dest(ft, words, 64, idx)
    rc = T.dietgpu_test_gather_config(ws.h, ft, 0, a16.data_ptr(), 64, 3, it.data_ptr(), dest.out.data_ptr(),
                                      status.data_ptr(), stream)
    assert rc == N.DIETGPU_OK, T.dietgpu_test_last_error()
    dest.check(status, "accepted config")


def test_check_raises(C, N, ws):
    words, a16, _ = table(C, ws, 2)
    R = G.rows_of(64)
    good = idx_tensor([0, R - 1, 5], 32)
    out, ok = C.gather_rows_device(a16, 64, good, torch.bfloat16, ws=ws, check=True)
    assert bool(ok.all())
    assert torch.equal(out.view(torch.int16), words[: R * 64].view(R, 64)[good.long()])
    for bad in ([0, R], [-1], [3, 1 << 40, 4]):
        with pytest.raises(N.DietGpuError, match="a row lies outside the table"):
            C.gather_rows_device(a16, 64, idx_tensor(bad, 64), torch.bfloat16, ws=ws, check=True)
    # another dtype than the archive's
    with pytest.raises(N.DietGpuError, match="does not match dtype"):
        C.gather_rows_device(a16, 64, good, torch.float16, ws=ws, check=True)
    # without check the same call returns the statuses
    _, ok = C.gather_rows_device(a16, 64, idx_tensor([0, R], 64), torch.bfloat16, ws=ws)
    assert ok.cpu().tolist() == [1, 0]


@pytest.mark.parametrize("ft", FTS, ids=FT_IDS.get)
def test_equals_the_host_index_gather(C, ws, ft):
    """Bit for bit what codec.gather_rows returns for the same rows."""
    words, a16, _ = table(C, ws, ft)
    for rw in (8, 1024, 4097):
        idx = G.index_lists(rw)["random"][0][:128] + G.index_lists(rw)["edges"][0]
        host = C.gather_rows(a16, rw, idx, TORCH_OUT[ft], ws=ws)
        dev, ok = C.gather_rows_device(a16, rw, idx_tensor(idx, 64), TORCH_OUT[ft], ws=ws)
        torch.cuda.synchronize()
        assert bool(ok.all())
        assert torch.equal(host.view(TORCH_WORD[ft]), dev.view(TORCH_WORD[ft]))
