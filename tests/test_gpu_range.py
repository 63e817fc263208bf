"""GPU tests of range decode: words [first, first + count)
of an archive through ans_decode_range / float_decompress_range /
gather_rows / torch.ops.dietgpu.decompress_data_range.  The codec is
lossless, so the expected output is input[first : first + count], compared bit
for bit on integer views.  Every destination is a view into a larger buffer
with 16 canary words on each side; the whole buffer is compared, so a stray
write, or any write to a failing member's destination, fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, N, Cache, compress_one, make_words, retyped, workspace_fixture  # noqa: F401
from tests.util import FT_IDS, NP_W, TORCH_FLOAT, WORD_BYTES, float_words

pytestmark = pytest.mark.gpu

CANARY = 16  # words on each side of every destination
FILL = 0xA5  # byte pattern of canaries and untouched destinations

BLK = 4096
N_BIG = 17 * BLK + 1234  # 18 blocks (odd, partial tail): three workgroups of 8


def big_ranges(n):
    return [
        (0, n),                                 # the whole element
        (0, 1),                                 # the first word
        (n - 1, 1),                             # the last word
        (4095, 2),                              # a block straddle
        (4096, 4096),                           # exactly one block, an odd first block
        (3 * 4096, 8),                          # a short aligned read
        (7 * 4096 + 5, 2 * 4096 + 3),           # crosses the workgroup boundary, unaligned start
        (16 * 4096 + 8, n - 16 * 4096 - 8),     # runs to the tail
        (123, 0),                               # empty
    ]


ws = workspace_fixture(64 << 20)
_ARCHIVES = Cache()


def archive(C, ws, ft, n=N_BIG, kind="normal", pb=10):
    """(words, archive), computed once per key and left unchanged."""
    def make():
        w = make_words(ft, n, kind, seed=ft + 10 * n % 1000)
        return w, compress_one(C, ws, w, ft, pb)
    return _ARCHIVES.get((ft, n, kind, pb), make)


def decode_range(C, ws, ft, archives, firsts, counts, outs, pb=10):
    if ft == 0:
        return C.ans_decode_range(archives, firsts, counts, outs, prob_bits=pb, ws=ws)
    return C.float_decompress_range(archives, firsts, counts, outs, dtype=TORCH_FLOAT[ft],
                                    prob_bits=pb, ws=ws)


def run_members(C, ws, ft, members, pb=10):
    """members: (archive, words or None, first, count, offset words, expect ok).
    One batched call; every destination starts `offset` words past a 16 B
    boundary inside one buffer, 16 canary words on each side.  Checks status,
    sizes and the whole buffer."""
    wb = WORD_BYTES[ft]
    per16 = 16 // wb
    starts, cur = [], 0
    for (_, _, _, count, off, _) in members:
        st = -(-(cur + CANARY) // per16) * per16 + off
        starts.append(st)
        cur = st + count + CANARY
    total = cur + per16
    buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(
        torch.uint8 if ft == 0 else {2: torch.int16, 4: torch.int32, 8: torch.int64}[wb])
    assert buf.data_ptr() % 16 == 0
    expect = np.full(total * wb, FILL, dtype=np.uint8).view(NP_W[ft]).copy()
    outs = []
    for (_, words, first, count, _, good), st in zip(members, starts):
        # a failing member's destination still has room for its count
        outs.append(buf[st: st + count])
        if good:
            expect[st: st + count] = words[first: first + count]
    _, ok, sz = decode_range(C, ws, ft, [m[0] for m in members], [m[2] for m in members],
                             [m[3] for m in members], outs, pb)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [int(m[5]) for m in members]
    assert sz.cpu().tolist() == [m[3] if m[5] else 0 for m in members]
    got = buf.cpu().numpy().view(NP_W[ft])
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, (f"{bad.size} words differ, first at buffer word {bad[0]} "
                           f"(member starts {starts})")


@pytest.mark.parametrize("off", [0, 1, 5])
@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4], ids=FT_IDS.get)
def test_ranges_of_a_large_element(C, ws, ft, off):
    """The issue's nine ranges of an 18-block element as one batch that shares
    one archive.  off: the destination's offset from a 16 B boundary, in
    words.  With off = 0 ranges whose first is a multiple of 16 B take the
    vector join and the others the scalar one; off = 5 aligns the range that
    starts at 7 * 4096 + 5 instead, whose edge chunks then switch between the
    two."""
    w, a = archive(C, ws, ft)
    run_members(C, ws, ft, [(a, w, f, c, off, True) for f, c in big_ranges(N_BIG)])


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4], ids=FT_IDS.get)
def test_small_elements(C, ws, ft):
    members = []
    for n in (1, 31, 4096, 4097):
        w, a = archive(C, ws, ft, n=n)
        for f, c in ((0, n), (0, 1), (n - 1, 1)):
            for off in (0, 1):
                members.append((a, w, f, c, off, True))
    run_members(C, ws, ft, members)


@pytest.mark.parametrize("pb", [9, 10, 11])
@pytest.mark.parametrize("ft", [0, 2], ids=FT_IDS.get)
def test_prob_bits(C, ws, ft, pb):
    w, a = archive(C, ws, ft, pb=pb)
    run_members(C, ws, ft, [(a, w, f, c, off, True) for f, c in big_ranges(N_BIG) for off in (0, 1)],
                pb=pb)


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4], ids=FT_IDS.get)
def test_failing_members(C, ws, ft):
    """Ranges past the element's end, an archive of another type and one of
    other prob bits: ok 0, size 0, destination untouched; the other members
    of the batch decode."""
    n = N_BIG
    w, a = archive(C, ws, ft)
    # (for the byte codec: a float archive, whose magic differs)
    wrong_type = archive(C, ws, 2)[1] if ft == 0 else retyped(a, ft)
    wrong_pb = archive(C, ws, ft, pb=9)[1]
    members = [
        (a, w, 5, 100, 0, True),
        (a, w, n, 1, 0, False),
        (a, w, n - 1, 2, 1, False),
        (a, w, 0xFFFFFFF0, 0x20, 0, False),
        (wrong_type, None, 0, 64, 0, False),
        (wrong_pb, None, 4096, 64, 0, False),
        (a, w, n - 1, 1, 0, True),
        (a, w, n, 0, 0, True),  # empty, at the very end
        (a, w, 8 * 4096, 4096 + 17, 0, True),
    ]
    run_members(C, ws, ft, members)


@pytest.mark.parametrize("ft", [0, 2, 3], ids=FT_IDS.get)
def test_high_entropy(C, ws, ft):
    """Uniformly random bit patterns: every block holds more than 512
    compressed words, so the ring refill and prefetch run inside ranges that
    start mid-archive.  (The normal data of the other tests fits the ring.)"""
    w, a = archive(C, ws, ft, kind="random")
    members = [(a, w, f, c, off, True) for f, c in big_ranges(N_BIG) for off in (0, 1)]
    run_members(C, ws, ft, members)


@pytest.mark.parametrize("ft", [2, 4], ids=FT_IDS.get)
def test_archive_from_the_cpu_oracle(C, ws, ft):
    w = make_words(ft, N_BIG, seed=321)
    a = torch.from_numpy(O.float_compress(w, ft)).to(DEV)
    run_members(C, ws, ft, [(a, w, f, c, off, True) for f, c in big_ranges(N_BIG) for off in (0, 1)])


def test_archive_with_a_checksum_decodes(C, ws):
    w = make_words(2, N_BIG, seed=5)
    a = compress_one(C, ws, w, 2, checksum=True)
    run_members(C, ws, 2, [(a, w, f, c, 0, True) for f, c in big_ranges(N_BIG)])


@pytest.mark.parametrize("ft", [0, 2, 4], ids=FT_IDS.get)
def test_archive_off_16_byte_alignment(C, N, ws, ft):
    """An archive 8 B off 16 B alignment takes the decoder's non-vector input
    path.  2 B off is refused by the host: the headers are read with scalar
    loads, which need 4 B alignment (the full decoder has the same need but
    does not check it)."""
    w, a = archive(C, ws, ft)
    room = torch.zeros([a.numel() + 32], dtype=torch.uint8, device=DEV)
    assert room.data_ptr() % 16 == 0
    a8 = room[8: 8 + a.numel()]
    a8.copy_(a)
    run_members(C, ws, ft, [(a8, w, f, c, off, True) for f, c in big_ranges(N_BIG) for off in (0, 1)])
    a2 = room[2: 2 + a.numel()]
    out = torch.full([64], FILL, dtype=torch.uint8, device=DEV)
    with pytest.raises(N.DietGpuError, match="aligned"):
        decode_range(C, ws, ft, [a2], [0], [4], [out[: 4 * WORD_BYTES[ft]]])
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


@pytest.mark.parametrize("nrows", [3, 700])
@pytest.mark.parametrize("shape,ft", [((300, 257), 2), ((64, 4096), 3)], ids=["bf16_300x257", "fp32_64x4096"])
def test_gather_rows(C, ws, shape, ft, nrows):
    """Row gather from one archive: 3 rows ride in the kernel-argument table,
    700 (with repeats, shuffled) in an uploaded one."""
    R, rw = shape
    w, a = archive(C, ws, ft, n=R * rw)
    rng = np.random.default_rng(nrows)
    rows = rng.integers(0, R, nrows)
    if nrows == 3:
        rows = np.array([R - 1, 0, R // 2 + 1])
    dtype = TORCH_FLOAT[ft]
    wb = WORD_BYTES[ft]
    buf = torch.full([(nrows * rw + 2 * CANARY) * wb], FILL, dtype=torch.uint8, device=DEV)
    out = buf[CANARY * wb: (CANARY + nrows * rw) * wb].view(dtype).view(nrows, rw)
    got = C.gather_rows(a, rw, rows.tolist() if nrows == 3 else torch.from_numpy(rows), dtype, out=out, ws=ws)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    expect = np.full((nrows * rw + 2 * CANARY) * wb, FILL, dtype=np.uint8).view(NP_W[ft]).copy()
    expect[CANARY: CANARY + nrows * rw] = w.reshape(R, rw)[rows].reshape(-1)
    np.testing.assert_array_equal(buf.cpu().numpy().view(NP_W[ft]), expect)
    with pytest.raises(C.N.DietGpuError):
        C.gather_rows(a, rw, [0, R], dtype, ws=ws)


@pytest.mark.parametrize("as_float", [True, False])
def test_torch_operator(C, ws, as_float):
    ft = 2 if as_float else 0
    ws_t = torch.empty([16 << 20], dtype=torch.uint8, device=DEV)
    w0, a0 = archive(C, ws, ft)
    w1, a1 = archive(C, ws, ft, n=4097)
    dt = torch.bfloat16 if as_float else torch.uint8
    ranges = [(7 * 4096 + 5, 2 * 4096 + 3), (4095, 2)]
    outs = [torch.empty([c], dtype=dt, device=DEV) for _, c in ranges]
    first = torch.tensor([f for f, _ in ranges], dtype=torch.int64)
    ok = torch.zeros([2], dtype=torch.uint8, device=DEV)
    sz = torch.zeros([2], dtype=torch.int32, device=DEV)
    op = torch.ops.dietgpu.decompress_data_range
    used = op(as_float, [a0, a1], outs, first, ws_t, ok, sz)
    torch.cuda.synchronize()
    assert isinstance(used, int)
    assert ok.cpu().tolist() == [1, 1] and sz.cpu().tolist() == [c for _, c in ranges]
    for o, w, (f, c) in zip(outs, (w0, w1), ranges):
        got = (o.view(torch.int16) if as_float else o).cpu().numpy().view(NP_W[ft])
        np.testing.assert_array_equal(got, w[f: f + c])
    from dietgpu_fork_amd import ops

    assert "decompress_data_range" in ops.OPS
    for bad in (-1, 1 << 32, 1 << 40):
        with pytest.raises(RuntimeError):
            op(as_float, [a0, a1], outs, torch.tensor([0, bad], dtype=torch.int64), ws_t)
    with pytest.raises(RuntimeError):  # int32 t_first
        op(as_float, [a0, a1], outs, torch.tensor([0, 0], dtype=torch.int32), ws_t)


@pytest.mark.parametrize("ft", [0, 2], ids=FT_IDS.get)
def test_config_with_checksum_is_rejected(C, N, ws, ft):
    """The C++ entry points refuse a config with useChecksum set (the C ABI and
    the Python / torch layers have no such flag, so this goes through the
    test-hook library, which calls the C++ functions)."""
    w, a = archive(C, ws, ft)
    T = N.testlib()
    buf = torch.full([64], FILL, dtype=torch.uint8, device=DEV)
    ok = torch.full([1], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([1], 7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rc = T.dietgpu_test_range_config(ws.h, ft, 1, a.data_ptr(), 8, 8, buf.data_ptr(), ok.data_ptr(),
                                     sz.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == N.DIETGPU_ERR_INVALID
    assert b"checksum" in T.dietgpu_test_last_error()
    assert ok.item() == 7 and sz.item() == 7 and bool((buf == FILL).all())
    # the same call without the flag decodes
    rc = T.dietgpu_test_range_config(ws.h, ft, 0, a.data_ptr(), 8, 8, buf.data_ptr(), ok.data_ptr(),
                                     sz.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == N.DIETGPU_OK and ok.item() == 1 and sz.item() == 8
    wb = WORD_BYTES[ft]
    np.testing.assert_array_equal(buf[: 8 * wb].cpu().numpy().view(NP_W[ft]), w[8:16])
    assert bool((buf[8 * wb:] == FILL).all())


def test_graph_capture_replay(C):
    """A batch-3 range decode captured in a hipGraph (its tables ride in the
    kernel arguments) and replayed after the archive's content changed."""
    n = 3 * BLK + 77
    ws = C.Workspace(16 << 20)
    x = torch.empty([1, n], dtype=torch.bfloat16, device=DEV)
    cols = C.max_float_compressed_size(2, n)
    arch = torch.empty([1, cols], dtype=torch.uint8, device=DEV)
    sizes = torch.empty([1], dtype=torch.int32, device=DEV)
    ranges = [(4095, 2), (5, 2 * BLK), (n - 9, 9)]
    outs = [torch.empty([c], dtype=torch.bfloat16, device=DEV) for _, c in ranges]
    firsts, counts = [f for f, _ in ranges], [c for _, c in ranges]

    def load(seed):
        w = float_words(2, n, seed=seed, scale=1 + seed % 3)
        x.copy_(torch.from_numpy(w.view(np.int16)).view(1, n).view(torch.bfloat16))
        return w

    load(1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.float_compress_stride(x, ws=ws, out=arch, sizes=sizes)
        C.float_decompress_range([arch[0]] * 3, firsts, counts, outs, dtype=torch.bfloat16, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        C.float_compress_stride(x, ws=ws, out=arch, sizes=sizes)
        _, ok, sz = C.float_decompress_range([arch[0]] * 3, firsts, counts, outs, dtype=torch.bfloat16,
                                             ws=ws)
    for rep in range(3):
        w = load(100 + rep)
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == [1, 1, 1] and sz.cpu().tolist() == counts
        for o, (f, c) in zip(outs, ranges):
            np.testing.assert_array_equal(o.view(torch.int16).cpu().numpy().view(np.uint16), w[f: f + c],
                                          err_msg=f"replay {rep}")
