"""GPU tests of the sparse decode-and-accumulate: acc += the
element a sparse archive encodes, at its nonzero words only, through
codec.sparse_decompress_accumulate, the C ABI, the C++ entry point (test hook)
and the reducing collectives of dist.py with GpuSparseFloatCodec.

The model is torch on the CPU (tests/sparse_accumulate_cases.py), never the
code under test.  Results are compared bit for bit wherever the model's result
is not a NaN and must be a NaN where it is; every word that is not under a
nonzero word of a succeeding member must keep its very bits, a NaN's payload
included.  Archives come from the CPU oracle's sparse compressor unless a test
says otherwise.  All accumulators of a call are slices of one buffer of random
finite values (every fifth one -0.0) with 16 guard words on each side, and the
buffer is compared whole: zero positions, tails past n, neighbours and failing
members' accumulators are all checked."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import pyref
from tests import sparse_accumulate_cases as S
from tests.dist_cases import pg  # noqa: F401
from tests.gpu_harness import (C, DEV, Cache, Member, accumulate_call, check_placed, dense_at,  # noqa: F401
                               expected_placed, place_members, retyped, workspace_fixture)
from tests.util import FT_OF, SPARSE_LARGE_B, float_words, sparse_far_element, sparsify

pytestmark = pytest.mark.gpu

GARBAGE = {1: 0xDEAD, 2: 0xBEEF, 3: 0xDEADBEEF, 4: 0xFFFFFFFFFFFFFFFF}

ws = workspace_fixture(512 << 20)
_ARCH = Cache()
NAMES = {"codec": "sparse_decompress_accumulate", "capi": "dietgpu_float_decompress_sparse_accumulate"}


def oracle_archive(ft, name, w, pb=10, checksum=False):
    """The CPU oracle's sparse archive, computed once per key and left unchanged."""
    return _ARCH.get((ft, name, pb, checksum), lambda: O.sparse_compress(w, ft, pb, checksum))


def random_words(ft, n, frac_zero, seed):
    return sparsify(float_words(ft, n, seed=seed), frac_zero, seed=seed + 1)


def M(arch, x, cap=None, acc_off=0, ok=True, acc=None):
    """One member of a call: archive bytes (always 16 B-aligned), the words it
    encodes, the accumulator's capacity and offset from a 16 B boundary,
    whether it must succeed, and (acc) values to put into its accumulator
    instead of the buffer's random ones.  The sparse size comes from the
    sparse header: n for every member, failing or not."""
    return Member(arch, x, cap, acc_off, ok=ok, size=x.size, acc=acc)


def model_of(ft, mode):
    """(apply, touched, compare) of expected_placed() / check_placed(): the
    model adds the nonzero words only, and S.check also holds every other
    word to the initial buffer's very bits."""
    return lambda acc, w: S.expected(acc, w, ft, mode), S.touched, S.check


def place(ft, mode, members, seed=0):
    """-> (archives, accs, buf, init, starts): every archive 16 B-aligned in
    one uint8 buffer, every accumulator acc_off words past a 16 B boundary
    inside one buffer `buf` (`init` is its CPU copy), 16 guard words apart."""
    return place_members(members, S.acc_dtype(ft, mode), lambda total: S.case_acc(ft, mode, total, seed=seed))


def expected(ft, mode, members, init, starts):
    """-> (want, touch): the buffer after the call and the words it may write."""
    return expected_placed(members, init, starts, *model_of(ft, mode)[:2])


def call(api, C, ws, ft, mode, archives, accs, buf, starts, pb=10, with_status=True):
    """-> (ok, sz) CPU lists, or None without status arrays.  The C ABI gets
    every accumulator's address inside `buf`, also for a capacity of 0 (an
    empty view has a null data pointer)."""
    return accumulate_call(api, NAMES, C, ws, ft, mode, archives, accs,
                           [buf.data_ptr() + st * buf.element_size() for st in starts], pb, with_status)


def run(api, C, ws, ft, mode, members, pb=10, with_status=True, seed=0):
    archives, accs, buf, init, starts = place(ft, mode, members, seed=seed)
    st = call(api, C, ws, ft, mode, archives, accs, buf, starts, pb, with_status)
    check_placed(members, st, buf.cpu(), init, starts, *model_of(ft, mode))


# ------------------------------------------------------------ size edges ----

@pytest.mark.parametrize("ft,mode", S.MODES, ids=S.MODE_IDS)
def test_size_edges(C, ws, ft, mode):
    """Every "small" edge element (sizes 0 .. 200 and +-2 around the row, chunk
    and dense-block edges, the four tails, zero / half / dense fills, the
    all-dense and all-zero block-edge elements) as one pointer batch, the
    accumulators alternating between 16 B-aligned and one word off; then the
    five elements around 262,144 words, the edge of a counting workgroup."""
    small = S.small_cases(ft)
    assert len(small) > 900
    run("codec", C, ws, ft, mode, [M(oracle_archive(ft, name, w), w, acc_off=i % 2)
                                   for i, (name, w) in enumerate(small)], seed=ft)
    large = S.large_cases(ft)
    assert [w.size for _, w in large] == [SPARSE_LARGE_B + d for d in range(-2, 3)]
    run("codec", C, ws, ft, mode, [M(oracle_archive(ft, name, w), w, acc_off=i % 2)
                                   for i, (name, w) in enumerate(large)], seed=10 + ft)


@pytest.mark.parametrize("mode", [2, 1], ids=["bf16-acc2", "bf16-acc1"])
def test_more_than_64_counting_workgroups(C, ws, mode):
    """The far element (bf16, 66 * 262,144 + 1102 words): its last chunks take
    the second round of totalsShare."""
    w = sparse_far_element()
    assert w.size > 65 * SPARSE_LARGE_B
    run("codec", C, ws, 2, mode, [M(oracle_archive(2, "far", w), w, acc_off=1)], seed=3)


# ------------------------------------------------------------ arithmetic ----

@pytest.mark.parametrize("ft,mode", [(1, 1), (2, 1), (1, 2), (2, 2)],
                         ids=["fp16-acc1", "bf16-acc1", "fp16-acc2", "bf16-acc2"])
def test_every_nonzero_16_bit_pattern(C, ws, ft, mode):
    """A zero-free element of every nonzero 16-bit pattern against the 16
    fixed accumulator values; then the same patterns with a zero word after
    each over -0.0, +-inf, NaNs and denormals: the zero positions keep their
    bits exactly (check() compares them with the initial buffer's)."""
    xd, ad = S.patterns16_dense(ft, mode)
    xi, ai = S.patterns16_interleaved(ft, mode)
    run("codec", C, ws, ft, mode, [M(oracle_archive(ft, "pat_dense", xd), xd, acc=ad),
                                   M(oracle_archive(ft, "pat_inter", xi), xi, acc=ai, acc_off=1)])


@pytest.mark.parametrize("ft", [3, 4], ids=["fp32", "fp64"])
def test_special_values_crossed(C, ws, ft):
    x, a = S.cross_specials_interleaved(ft)
    run("codec", C, ws, ft, 1, [M(oracle_archive(ft, "cross", x), x, acc=a, acc_off=k) for k in (0, 1)])


# -------------------------------------------------------------- gap rule ----

@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (4, 1)], ids=["bf16-acc1", "bf16-acc2", "fp64"])
def test_reference_legal_archives(C, ws, ft, mode):
    """Archives as the reference may emit them: a garbage word in the n-2 slot
    of the list, 0xFF in the bitmap's padding bytes and (n % 8 != 0) set bits
    past n in its last byte.  Neither reaches an accumulator."""
    els = {name: w for _, name, w in S.edge_elements(ft)}
    members = []
    for B in (64, 256, 1024, 4096):
        for name in (f"n{B + 1}_{('zero', 'half', 'dense')[(B + 1) % 3]}_t01",
                     f"n{B}_{('zero', 'half', 'dense')[B % 3]}_t00"):
            w = els[name]
            n = w.size
            assert w[n - 2] == 0
            plain = oracle_archive(ft, name, w)
            variants = [pyref.sparse_compress(ft, w, 10, gap_fill=GARBAGE[ft], pad_fill=0xFF)]
            if n % 8:
                variants.append(pyref.sparse_compress(ft, w, 10, gap_fill=GARBAGE[ft] - 1, pad_fill=0xFF,
                                                      pad_bits=True))
            for k, v in enumerate(variants):
                assert v.size == plain.size and not np.array_equal(v, plain)
                members.append(M(v, w, cap=n + 3 * (k % 2), acc_off=len(members) % 2))
    assert len(members) >= 12
    run("codec", C, ws, ft, mode, members, seed=5)


# ------------------------------------------------------ failure contract ----

def failure_members(ft):
    els = {name: w for _, name, w in S.edge_elements(ft)}
    a, b, c, d, e = (els[k] for k in ("n4097_dense_t01", "n1025_dense_t01", "n200_dense_t10", "n8193_zero_t01",
                                      "n2049_zero_t01"))
    arch = {id(w): oracle_archive(ft, f"fail{k}", w) for k, w in enumerate((a, b, c, d, e))}
    other = retyped(arch[id(d)], ft, at=dense_at(d.size) + 8)  # the dense header names another float type
    pb9 = oracle_archive(ft, "fail_pb9", b, pb=9)
    magic = arch[id(a)].copy()
    magic[dense_at(a.size)] ^= 0x40  # the dense magic word
    return [
        M(arch[id(a)], a),
        M(arch[id(b)], b, cap=b.size - 1, ok=False),    # accumulator one word short
        M(arch[id(c)], c, acc_off=1),
        M(other, d, ok=False),                          # dense part of another float type
        M(arch[id(e)], e, cap=e.size + 3),              # room to spare: only [0, n) may change
        M(pb9, b, acc_off=1, ok=False),                 # dense part with other prob bits
        M(magic, a, ok=False),                          # dense part with a corrupt magic
        M(arch[id(b)], b),
    ]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (3, 1), (4, 1)], ids=["bf16-acc1", "bf16-acc2", "fp32", "fp64"])
def test_failure_contract(C, ws, ft, mode, with_status):
    """Good and failing members in one batch: status 0 and size n for every
    failing one, its accumulator bitwise untouched, the good ones exact."""
    run("capi", C, ws, ft, mode, failure_members(ft), with_status=with_status, seed=9)


# --------------------------------------------------------------- variants ----

@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, pb):
    ms = [M(oracle_archive(2, f"pb{n}", w, pb=pb), w) for n in (70001, 9) for w in [random_words(2, n, 0.9, seed=pb + n)]]
    run("codec", C, ws, 2, 1, ms, pb=pb)
    run("capi", C, ws, 2, 2, ms, pb=pb)


def test_checksummed_archive_accumulates(C, ws):
    w = random_words(2, 12345, 0.9, seed=11)
    arch = oracle_archive(2, "ck", w, checksum=True)
    assert not np.array_equal(arch, oracle_archive(2, "ck", w))
    run("codec", C, ws, 2, 2, [M(arch, w), M(arch, w, acc_off=1)])


@pytest.mark.parametrize("ft,mode", [(2, 1), (2, 2), (3, 1)], ids=["bf16-acc1", "bf16-acc2", "fp32"])
def test_gpu_compressed_archive(C, ws, ft, mode):
    w = random_words(ft, 70001, 0.9, seed=21)
    out, sizes = C.sparse_compress([S.words_to_float(w, ft).to(DEV)], ft=ft, ws=ws)
    arch = out[0, : int(sizes[0])].cpu().numpy()
    run("codec", C, ws, ft, mode, [M(arch, w)])


def test_side_stream(C, ws):
    w = random_words(1, 32769, 0.9, seed=12)
    m = [M(oracle_archive(1, "side", w), w)]
    archives, accs, buf, init, starts = place(1, 2, m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ok, sz = C.sparse_decompress_accumulate(archives, accs, ft=1, ws=ws)
    s.synchronize()
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [w.size]
    want, touch = expected(1, 2, m, init, starts)
    assert S.check(buf.cpu(), want, init, touch) is None


def test_401_member_batch(C, ws):
    """More members than ride in the kernel arguments: the tables are uploaded."""
    ms = []
    for i in range(401):
        n = 1 + (37 * i) % 700
        w = random_words(2, n, 0.5, seed=i % 8)
        ms.append(M(oracle_archive(2, f"b401_{n}_{i % 8}", w), w, acc_off=i % 2))
    run("codec", C, ws, 2, 2, ms)
    run("capi", C, ws, 2, 1, ms)


def test_c_abi(C, ws):
    """The C ABI through ctypes, every mode, one aligned and one off member."""
    for ft, mode in S.MODES:
        ms = [M(oracle_archive(ft, f"capi{n}", w), w, acc_off=k)
              for k, n in enumerate((4097, 1025)) for w in [random_words(ft, n, 0.9, seed=n + ft)]]
        run("capi", C, ws, ft, mode, ms)
        run("capi", C, ws, ft, mode, ms, with_status=False)


# ----------------------------------------------------------------- mode 2 ----

def test_four_archives_into_one_fp32_accumulator(C, ws):
    n = 12345
    xs = [random_words(2, n, 0.9, seed=30 + k) for k in range(4)]
    init = S.case_acc(2, 2, n, seed=3)
    acc = init.to(DEV)
    want = init.clone()
    touch = torch.zeros(n, dtype=torch.bool)
    for k, w in enumerate(xs):
        a = torch.from_numpy(oracle_archive(2, f"four{k}", w).copy()).to(DEV)
        ok, sz = C.sparse_decompress_accumulate([a], [acc], ft=2, ws=ws)
        assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [n]
        want = S.expected(want, w, 2, 2)
        touch |= S.touched(w)
    assert S.check(acc.cpu(), want, init, touch) is None


@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_fused_equals_decompress_then_add(C, ws, ft):
    """With an accumulator free of -0.0 (and of NaNs) skipping a zero word and
    adding +0.0 are the same thing: the fused result is bitwise what
    sparse_decompress into a temporary and acc += tmp.float() give."""
    n = 70001
    w = random_words(ft, n, 0.9, seed=40)
    init = S.random_acc(ft, 2, n, seed=41)
    init[init == 0] = 1.0
    a = torch.from_numpy(oracle_archive(ft, "fused", w).copy()).to(DEV)
    fused = init.to(DEV)
    ok, _ = C.sparse_decompress_accumulate([a], [fused], ft=ft, ws=ws)
    tmp = torch.empty(n, dtype=S.TORCH_FLOAT[ft], device=DEV)
    ok2, _ = C.sparse_decompress([a], [tmp], ft=ft, ws=ws)
    unfused = init.to(DEV)
    unfused += tmp.float()
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1] == ok2.cpu().tolist()
    assert torch.equal(S.bits(fused), S.bits(unfused))


# ------------------------------------------------- the C++ entry point ----

def test_cpp_entry_point_rejects_checksum_and_bad_acc_type(C, ws):
    from dietgpu_fork_amd import _native as N

    T = N.testlib()
    w = random_words(2, 4097, 0.9, seed=50)
    a = torch.from_numpy(oracle_archive(2, "cpp", w).copy()).to(DEV)
    init = S.case_acc(2, 2, 4097, seed=51)
    acc = init.to(DEV)
    ok = torch.full([1], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([1], -7, dtype=torch.int32, device=DEV)

    def hook(ft, checksum, acc_type):
        rc = T.dietgpu_test_sparse_accumulate_config(ws.h, ft, checksum, acc_type, a.data_ptr(), acc.data_ptr(), 4097,
                                                     ok.data_ptr(), sz.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
        return rc, T.dietgpu_test_last_error().decode()

    rc, msg = hook(2, 1, 3)
    assert rc == N.DIETGPU_ERR_INVALID and "cannot verify a checksum" in msg
    for ft, acc_type in ((2, 1), (2, 4), (3, 2), (4, 3), (2, 0), (2, 7)):
        rc, msg = hook(ft, 0, acc_type)
        assert rc == N.DIETGPU_ERR_INVALID and f"accumulator type {acc_type} does not go with float type {ft}" in msg
    torch.cuda.synchronize()
    assert torch.equal(S.bits(acc.cpu()), S.bits(init)) and ok.item() == 7 and sz.item() == -7
    rc, msg = hook(2, 0, 3)  # and the good call goes through
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert ok.item() == 1 and sz.item() == 4097
    assert S.check(acc.cpu(), S.expected(init, w, 2, 2), init, S.touched(w)) is None


# ----------------------------------------------------------- collectives ----

def sparse_tensor(ft, n, seed):
    """90 % zeros, -0.0 among the nonzero words."""
    w = random_words(ft, n, 0.9, seed=seed)
    x = S.words_to_float(w, ft)
    x[3::50] = -0.0
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_world_of_one_returns_its_input(pg, dtype):
    from dietgpu_fork_amd import dist as D

    codec = D.GpuSparseFloatCodec()
    x = sparse_tensor(FT_OF[dtype], 12345, seed=7).to(DEV)
    assert bool((S.bits(x) == S.bits(torch.tensor([-0.0], dtype=dtype, device=DEV))).any())
    y = D.reduce_scatter_compressed([x], codec=codec)
    assert y.dtype == dtype and y.data_ptr() != x.data_ptr() and torch.equal(S.bits(y), S.bits(x))
    z = D.all_reduce_compressed(x.view(3, 4115), codec=codec)
    assert z.shape == (3, 4115) and torch.equal(S.bits(z.view(-1)), S.bits(x))


@pytest.mark.parametrize("dtype,acc", [(torch.bfloat16, None), (torch.bfloat16, torch.bfloat16),
                                       (torch.float16, None), (torch.float32, None)],
                         ids=["bf16-f32acc", "bf16-bf16acc", "fp16-f32acc", "fp32"])
def test_reduce_archives_on_gpu_compressed_sparse_peers(pg, dtype, acc):
    """The collective's local part on the real kernels: own + three peers'
    GPU-compressed sparse archives, in order, against the model (a peer's zero
    words are skipped)."""
    from dietgpu_fork_amd import dist as D

    ft = FT_OF[dtype]
    n = 33001
    own = S.case_acc(ft, 1, n, seed=70)
    peers = [sparse_tensor(ft, n, seed=71 + k) for k in range(3)]
    codec = D.GpuSparseFloatCodec()
    comp, sizes = codec.compress([p.to(DEV) for p in peers])
    archives = [comp[i, : int(sizes[i])] for i in range(3)]
    assert codec.info(archives[0]) == (n, dtype)
    got = D.reduce_archives(own.to(DEV), archives, codec, acc_dtype=acc)
    mode = 2 if (acc or (torch.float32 if ft <= 2 else dtype)) != dtype else 1
    a = own.to(S.acc_dtype(ft, mode))
    for p in peers:
        a = S.expected(a, S.float_to_words(p, ft), ft, mode)
    want = a.to(dtype)
    assert got.dtype == dtype and S.same_bits(got.cpu(), want), S.mismatch_report(got.cpu(), want)
    # own=None: the first archive stands in for it, through the codec's info
    got = D.reduce_archives(None, archives, codec, acc_dtype=acc)
    a = peers[0].to(S.acc_dtype(ft, mode))
    for p in peers[1:]:
        a = S.expected(a, S.float_to_words(p, ft), ft, mode)
    assert S.same_bits(got.cpu(), a.to(dtype))
