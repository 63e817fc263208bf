"""GPU tests of decode-and-accumulate: acc += the element an
archive encodes, through codec.float_decompress_accumulate, the C ABI,
torch.ops.dietgpu.decompress_data_accumulate and the reducing collectives of
dist.py.

The model is torch on the CPU (tests/accumulate_cases.py), never the code
under test; results are compared bit for bit on integer views wherever the
model's result is not a NaN, and must be a NaN where it is.  Archives come
from the CPU oracle, so a compressor problem cannot mask a decoder one (one
case additionally feeds a GPU-compressed archive).  All accumulators of a call
live in one buffer of random finite values with at least 16 words between
them; the buffer is compared whole, so a stray read-modify-write, or any write
to a failing member's accumulator, fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import accumulate_cases as A
from tests.dist_cases import pg  # noqa: F401
from tests.gpu_harness import (C, DEV, GUARD as CANARY, Cache, Member, accumulate_call, check_placed,  # noqa: F401
                               compress_one, expected_placed, place_members, workspace_fixture)
from tests.util import FT_OF

pytestmark = pytest.mark.gpu

ws = workspace_fixture(64 << 20)
_ARCH = Cache()
NAMES = {"codec": "float_decompress_accumulate", "op": "decompress_data_accumulate",
         "capi": "dietgpu_float_decompress_accumulate"}


def oracle_archive(ft, n, seed=0, pb=10, checksum=False):
    """(words, archive bytes) from the CPU oracle, computed once per key."""
    def make():
        w = A.member_words(ft, n, seed=seed)
        return w, O.float_compress(w, ft, pb, checksum)
    return _ARCH.get((ft, n, seed, pb, checksum), make)


def M(arch, x, cap=None, acc_off=0, arch_off=0, ok=True, size=None):
    """One member of a call: archive bytes, the words it encodes (None: it
    must fail, and reports size 0 unless `size` says otherwise), the
    accumulator's capacity and the two alignments."""
    return Member(arch, x, cap, acc_off, arch_off, ok, size)


def model_of(ft, mode):
    """(apply, touched, compare) of expected_placed() / check_placed(): the
    model adds every word, and the buffer is compared with same_bits."""
    return (lambda acc, w: A.model(acc, A.words_to_float(w, ft), mode),
            lambda w: torch.ones(w.size, dtype=torch.bool),
            lambda got, want, init, touch: None if A.same_bits(got, want) else A.mismatch_report(got, want))


def place(ft, mode, members, seed=0, acc_init=None):
    """-> (archives, accs, buf, init, starts): every archive 16 B-aligned plus
    arch_off bytes inside one uint8 buffer, every accumulator acc_off words
    past a 16 B boundary inside one buffer `buf` of random finite values
    (`init` is its CPU copy), CANARY words apart at least."""
    init = (lambda total: A.random_acc(ft, mode, total, seed=seed)) if acc_init is None else acc_init
    return place_members(members, A.acc_dtype(ft, mode), init)


def expected(ft, mode, members, init, starts):
    return expected_placed(members, init, starts, *model_of(ft, mode)[:2])[0]


def call(api, C, ws, ft, mode, archives, accs, pb=10, with_status=True, temp_mem=True):
    """-> (ok, sz) CPU lists, or None without status tensors."""
    return accumulate_call(api, NAMES, C, ws, ft, mode, archives, accs, [a.data_ptr() for a in accs], pb,
                           with_status, temp_mem)


def run(api, C, ws, ft, mode, members, pb=10, with_status=True, temp_mem=True, seed=0):
    archives, accs, buf, init, starts = place(ft, mode, members, seed=seed)
    st = call(api, C, ws, ft, mode, archives, accs, pb, with_status, temp_mem)
    check_placed(members, st, buf.cpu(), init, starts, *model_of(ft, mode))


# ------------------------------------------------------------ size edges ----

@pytest.mark.parametrize("ft,mode", A.MODES, ids=A.MODE_IDS)
def test_size_edges(C, ws, ft, mode):
    """One pointer batch of elements of every edge size; the members alternate
    between accumulators 16 B-aligned and one word off, and between archives
    16 B-aligned and 4 B off (all four combinations)."""
    members = []
    for i, n in enumerate(A.SIZES):
        w, arch = oracle_archive(ft, n, seed=i)
        members.append(M(arch, w, acc_off=i % 2, arch_off=4 * ((i // 2) % 2)))
    assert {(m.acc_off, m.arch_off) for m in members} == {(0, 0), (1, 0), (0, 4), (1, 4)}
    run("codec", C, ws, ft, mode, members, seed=ft)


# ------------------------------------------------------------ arithmetic ----

@pytest.mark.parametrize("ft,mode", [(1, 1), (2, 1), (1, 2), (2, 2)],
                         ids=["fp16-acc1", "bf16-acc1", "fp16-acc2", "bf16-acc2"])
def test_every_16_bit_pattern(C, ws, ft, mode):
    """Every 16-bit pattern as x against each of the 16 fixed accumulator
    values and one random vector: 17 x 65,536 words."""
    xw, acc = A.arithmetic16(ft, mode)
    m = M(_ARCH.get(("patterns", ft), lambda: O.float_compress(xw, ft, 10)), xw)
    archives, accs, buf, init, starts = place(ft, mode, [m], acc_init=lambda total: torch.cat(
        [A.random_acc(ft, mode, CANARY, seed=5), acc, A.random_acc(ft, mode, total - CANARY - acc.numel(), seed=6)]))
    assert starts == [CANARY]
    st = call("codec", C, ws, ft, mode, archives, accs)
    assert st == ([1], [xw.size])
    want = expected(ft, mode, [m], init, starts)
    got = buf.cpu()
    assert A.same_bits(got, want), A.mismatch_report(got, want)


@pytest.mark.parametrize("ft", [3, 4], ids=["fp32", "fp64"])
def test_special_values_crossed(C, ws, ft):
    """The special-value table crossed with itself plus 1e5 random pairs."""
    x, acc = A.cross_specials(ft)
    xw = A.float_to_words(x, ft)
    m = M(O.float_compress(xw, ft, 10), xw)
    archives, accs, buf, init, starts = place(ft, 1, [m], acc_init=lambda total: torch.cat(
        [A.random_acc(ft, 1, CANARY, seed=5), acc, A.random_acc(ft, 1, total - CANARY - acc.numel(), seed=6)]))
    assert starts == [CANARY]
    assert call("codec", C, ws, ft, 1, archives, accs) == ([1], [xw.size])
    want = expected(ft, 1, [m], init, starts)
    got = buf.cpu()
    assert A.same_bits(got, want), A.mismatch_report(got, want)


# ------------------------------------------------------ failure contract ----

def failure_members(ft):
    other = 1 if ft != 1 else 2
    w0, a0 = oracle_archive(ft, 5000, seed=1)
    w1, a1 = oracle_archive(ft, 4097, seed=2)
    _, a_other = oracle_archive(other, 4097, seed=3)
    _, a_pb = oracle_archive(ft, 4100, seed=4, pb=9)
    bad = oracle_archive(ft, 4200, seed=5)[1].copy()
    bad[0] ^= 0x40  # the magic word
    w2, a2 = oracle_archive(ft, 8, seed=6)
    return [
        M(a0, w0),
        M(a1, w1, cap=w1.size - 1, ok=False, size=w1.size),           # one word short: size n, untouched
        M(a_other, None, cap=4097, acc_off=1, ok=False, size=0),      # another float type
        M(a_pb, None, cap=4100, ok=False, size=0),                    # other prob bits
        M(bad, None, cap=4200, arch_off=4, ok=False, size=0),         # corrupt magic
        M(a2, w2, acc_off=1),
        M(a1, w1, cap=w1.size + 3),                                   # room to spare: only [0, n) changes
    ]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (3, 1), (4, 1)], ids=["bf16-acc1", "bf16-acc2", "fp32", "fp64"])
def test_failure_contract(C, ws, ft, mode, with_status):
    """Good and failing members in one batch: the good ones exact, every
    failing member's accumulator untouched, status and sizes as the full
    decode's."""
    run("capi", C, ws, ft, mode, failure_members(ft), with_status=with_status, seed=9)


# ----------------------------------------------------------- other cases ----

def test_checksummed_archive_accumulates(C, ws):
    w, arch = oracle_archive(2, 12345, seed=11, checksum=True)
    assert arch[8:12].view(np.uint32)[0] != 2  # the header's type word carries the checksum flag
    for api in ("codec", "op"):
        run(api, C, ws, 2, 2, [M(arch, w), M(arch, w, acc_off=1)])


@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, pb):
    ms = [M(*oracle_archive(ft, n, seed=pb, pb=pb)[::-1]) for ft, n in ((2, 70001), (2, 9))]
    run("codec", C, ws, 2, 1, ms, pb=pb)
    run("capi", C, ws, 2, 2, ms, pb=pb)


def test_side_stream(C, ws):
    w, arch = oracle_archive(1, 32769, seed=12)
    m = [M(arch, w)]
    archives, accs, buf, init, starts = place(1, 2, m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ok, sz = C.float_decompress_accumulate(archives, accs, ft=1, ws=ws)
    s.synchronize()
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [w.size]
    want = expected(1, 2, m, init, starts)
    assert A.same_bits(buf.cpu(), want), A.mismatch_report(buf.cpu(), want)


def test_401_member_batch(C, ws):
    """More members than ride in the kernel arguments: the tables are uploaded."""
    ms = []
    for i in range(401):
        w, arch = oracle_archive(2, 1 + (37 * i) % 700, seed=i % 8)
        ms.append(M(arch, w, acc_off=i % 2))
    run("codec", C, ws, 2, 2, ms)
    run("op", C, ws, 2, 1, ms)


@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (3, 1)], ids=["bf16-acc1", "bf16-acc2", "fp32"])
def test_gpu_compressed_archive(C, ws, ft, mode):
    w = A.member_words(ft, 70001, seed=21)
    arch = compress_one(C, ws, w, ft).cpu().numpy()
    run("codec", C, ws, ft, mode, [M(arch, w)])


@pytest.mark.parametrize("temp_mem", [True, False], ids=["temp_mem", "no-temp_mem"])
@pytest.mark.parametrize("ft,mode", A.MODES, ids=A.MODE_IDS)
def test_torch_operator(C, ws, ft, mode, temp_mem):
    """The operator picks the mode from the accumulators' dtype (and, for
    float32 accumulators, the first archive's header)."""
    ms = [M(*oracle_archive(ft, n, seed=n % 7)[::-1], acc_off=i % 2) for i, n in enumerate((4097, 9, 32768))]
    run("op", C, ws, ft, mode, ms, temp_mem=temp_mem)
    run("op", C, ws, ft, mode, ms, temp_mem=temp_mem, with_status=False)


def test_operator_rejections_on_device_tensors(C, ws):
    D = torch.ops.dietgpu
    w, arch = oracle_archive(2, 4097, seed=1)
    a = torch.from_numpy(arch.copy()).to(DEV)
    acc = torch.zeros(4097, dtype=torch.float32, device=DEV)
    keep = acc.clone()
    with pytest.raises(RuntimeError, match="must be uint8"):
        D.decompress_data_accumulate([a.view(torch.int8)], [acc])
    with pytest.raises(RuntimeError, match="archive header"):
        D.decompress_data_accumulate([a[:16]], [acc])
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        D.decompress_data_accumulate([a[1:]], [acc])
    with pytest.raises(RuntimeError, match="contiguous"):
        D.decompress_data_accumulate([a], [torch.zeros(2 * 4097, dtype=torch.float32, device=DEV)[::2]])
    with pytest.raises(RuntimeError, match="out_status must have 1 entries"):
        D.decompress_data_accumulate([a], [acc], None, torch.zeros(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="int32"):
        D.decompress_data_accumulate([a], [acc], None, None, torch.zeros(1, dtype=torch.int64, device=DEV))
    a64 = torch.from_numpy(oracle_archive(4, 100, seed=1)[1].copy()).to(DEV)
    with pytest.raises(RuntimeError, match="float64 one"):
        D.decompress_data_accumulate([a64], [acc])
    assert torch.equal(acc, keep)


def test_codec_wrapper_rejections(C, ws):
    w, arch = oracle_archive(2, 4097, seed=1)
    a = torch.from_numpy(arch.copy()).to(DEV)
    f32 = torch.zeros(4097, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="share a dtype"):
        C.float_decompress_accumulate([a, a], [f32, f32.double()], ft=2, ws=ws)
    with pytest.raises(ValueError, match="does not go with"):
        C.float_decompress_accumulate([a], [f32.double()], ft=2, ws=ws)
    with pytest.raises(ValueError, match="one entry per member"):
        C.float_decompress_accumulate([a, a], [f32], ft=2, ws=ws)
    assert not bool(f32.any())


def test_repeated_accumulation(C, ws):
    """Four bf16 archives into one fp32 accumulator, one call each."""
    n = 12345
    xs = [oracle_archive(2, n, seed=30 + k) for k in range(4)]
    init = A.random_acc(2, 2, n, seed=3)
    acc = init.to(DEV)
    want = init.clone()
    for w, arch in xs:
        a = torch.from_numpy(arch.copy()).to(DEV)
        ok, _ = C.float_decompress_accumulate([a], [acc], ft=2, ws=ws)
        assert ok.cpu().tolist() == [1]
        want = A.model(want, A.words_to_float(w, 2), 2)
    assert A.same_bits(acc.cpu(), want), A.mismatch_report(acc.cpu(), want)


def test_graph_capture_replay(C):
    """One accumulate call captured in a hipGraph and replayed twice, new
    archive bytes copied into the same buffers in between."""
    ws = C.Workspace(16 << 20)
    n = 40000
    pairs = [[oracle_archive(2, n, seed=40 + 2 * r + j) for j in range(2)] for r in range(3)]
    room = max(a.size for row in pairs for _, a in row)
    slots = [torch.zeros(room, dtype=torch.uint8, device=DEV) for _ in range(2)]
    init = A.random_acc(2, 2, 2 * n + 64, seed=4)
    buf = init.to(DEV)
    accs = [buf[16:16 + n], buf[48 + n:48 + 2 * n]]

    def load(r):
        for slot, (_, a) in zip(slots, pairs[r]):
            slot[: a.size].copy_(torch.from_numpy(a.copy()))

    load(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.float_decompress_accumulate(slots, accs, ft=2, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        ok, sz = C.float_decompress_accumulate(slots, accs, ft=2, ws=ws)
    buf.copy_(init)
    want = init.clone()
    for r in (1, 2):
        load(r)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == [1, 1] and sz.cpu().tolist() == [n, n]
        for (w, _), st in zip(pairs[r], (16, 48 + n)):
            want[st:st + n] = A.model(want[st:st + n], A.words_to_float(w, 2), 2)
        assert A.same_bits(buf.cpu(), want), f"replay {r}: " + A.mismatch_report(buf.cpu(), want)


@pytest.mark.parametrize("mode", [1, 2], ids=["acc1", "acc2"])
def test_several_passes_per_workgroup(C, mode):
    """256 x 524,288 bf16 words (the c2 shape): the host gives every workgroup
    two or more chunks there, so the double-buffered destination prefetch
    crosses a pass boundary.  Four distinct (accumulator row, element) pairs
    repeat through the batch; every row is compared with the model's."""
    nb, n, kinds = 256, 524288, 4
    ws = C.Workspace(16 << 20)
    rows = [oracle_archive(2, n, seed=50 + k) for k in range(kinds)]
    arch = [torch.from_numpy(a.copy()).to(DEV) for _, a in rows]
    init = [A.random_acc(2, mode, n, seed=60 + k) for k in range(kinds)]
    want = torch.stack([A.model(init[k], A.words_to_float(rows[k][0], 2), mode) for k in range(kinds)])
    assert not bool(torch.isnan(want).any())
    buf = torch.stack(init).to(DEV).repeat(nb // kinds, 1).contiguous()  # row i holds pair i % kinds
    ok, sz = C.float_decompress_accumulate([arch[i % kinds] for i in range(nb)], [buf[i] for i in range(nb)], ft=2,
                                           ws=ws)
    assert bool((ok == 1).all()) and bool((sz == n).all())
    got = A.bits(buf).view(nb // kinds, kinds, n)
    assert bool((got == A.bits(want).to(DEV)[None]).all())


# ----------------------------------------------------------- collectives ----

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_world_of_one_returns_its_input(pg, dtype):
    from dietgpu_fork_amd import dist as D

    x = A.random_acc(FT_OF[dtype], 1, 12345, seed=7)
    x[::5] = -0.0
    x = x.to(DEV)
    y = D.reduce_scatter_compressed([x])
    assert y.dtype == dtype and y.data_ptr() != x.data_ptr() and torch.equal(A.bits(y), A.bits(x))
    z = D.all_reduce_compressed(x.view(3, 4115))
    assert z.shape == (3, 4115) and torch.equal(A.bits(z.view(-1)), A.bits(x))


@pytest.mark.parametrize("dtype,acc", [(torch.bfloat16, None), (torch.bfloat16, torch.bfloat16),
                                       (torch.float16, None), (torch.float32, None)],
                         ids=["bf16-f32acc", "bf16-bf16acc", "fp16-f32acc", "fp32"])
def test_reduce_archives_on_gpu_compressed_peers(pg, dtype, acc):
    """The collective's local part on the real kernel: own + three peers'
    GPU-compressed archives, in order, against the model."""
    from dietgpu_fork_amd import dist as D

    ft = FT_OF[dtype]
    n = 33001
    own = A.random_acc(ft, 1, n, seed=70)
    peers = [A.random_acc(ft, 1, n, seed=71 + k) for k in range(3)]
    codec = D.GpuFloatCodec()
    comp, sizes = codec.compress([p.to(DEV) for p in peers])
    archives = [comp[i, : int(sizes[i])] for i in range(3)]
    got = D.reduce_archives(own.to(DEV), archives, codec, acc_dtype=acc)
    mode = 2 if (acc or (torch.float32 if ft <= 2 else dtype)) != dtype else 1
    a = own.to(A.acc_dtype(ft, mode))
    for p in peers:
        a = A.model(a, p, mode)
    want = a.to(dtype)
    assert got.dtype == dtype and A.same_bits(got.cpu(), want), A.mismatch_report(got.cpu(), want)
    # own=None: the first archive stands in for it
    got = D.reduce_archives(None, archives, codec, acc_dtype=acc)
    a = peers[0].to(A.acc_dtype(ft, mode))
    for p in peers[1:]:
        a = A.model(a, p, mode)
    assert A.same_bits(got.cpu(), a.to(dtype))
