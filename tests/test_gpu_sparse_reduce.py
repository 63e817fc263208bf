"""GPU tests of the fused sparse reduce: K sparse archives per
member expanded and summed in registers by k_sparseReduce, through
codec.sparse_reduce, the C ABI, the C++ entry point (test hook) and the
reducing collectives of dist.py with GpuSparseFloatCodec.

The model is torch on the CPU (tests/sparse_reduce_cases.py), never the code
under test; results are compared with accumulate_cases.same_bits: bit for bit
wherever the model is not a NaN, a NaN where it is.  Archives come from the
CPU oracle's sparse compressor unless a test says otherwise.  The outputs (and
the inits) of a call are slices of one buffer of random finite values, every
fifth one -0.0, with 16 guard words between members and at both ends,
alternately 16 B-aligned and one word off; the buffers are compared whole, so
a stray write, or any write to a failing member, fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import accumulate_cases as A
from tests import pyref
from tests import reduce_cases as R
from tests import sparse_accumulate_cases as S
from tests import sparse_reduce_cases as SR
from tests.dist_cases import pg  # noqa: F401
from tests.gpu_harness import C, DEV, Cache, dense_at, pack_bytes, place_words, retyped, workspace_fixture  # noqa: F401
from tests.util import FT_OF, NP_WORD, SPARSE_LARGE_B, float_words, sparse_far_element, sparsify

pytestmark = pytest.mark.gpu

ws = workspace_fixture(512 << 20)
_ARCH = Cache()
FT_PARAMS = dict(argvalues=SR.FTS, ids=[A.FT_IDS[ft] for ft in SR.FTS])
GARBAGE = {1: 0xDEAD, 2: 0xBEEF, 3: 0xDEADBEEF}


def archive_of(w, ft, pb=10, checksum=False, key=None):
    """The oracle's sparse archive of the words w (cached under `key`)."""
    def make():
        return O.sparse_compress(w, ft, pb, checksum)
    return make() if key is None else _ARCH.get((key, ft, pb, checksum), make)


def random_words(ft, n, frac_zero, seed):
    """N(0,1) words, frac_zero of them +0.0 at random positions, -0.0 at a few
    of the others."""
    w = sparsify(float_words(ft, n, seed=seed), frac_zero, seed=seed + 1)
    neg0 = A.float_to_words(torch.tensor([-0.0], dtype=A.TORCH_FLOAT[ft]), ft)[0]
    w[3::50] = np.where(w[3::50] != 0, neg0, 0)
    return w


def source(ft, n, seed, frac_zero=0.7, pb=10, checksum=False):
    """(words, archive) of one random source (cached)."""
    key = ("src", ft, n, seed, frac_zero)
    w = _ARCH.get(key, lambda: random_words(ft, n, frac_zero, seed))
    return w, archive_of(w, ft, pb, checksum, key=key)


class M:
    """One member: its K archives (bytes, always 16 B-aligned), the K word
    vectors (None: the member must fail), the capacity, the offsets of out /
    init from a 16 B boundary in words, and the size it must report (the
    first source's n, from the sparse header, failing or not)."""

    def __init__(self, archs, xs, cap=None, out_off=0, init_off=0, ok=True, size=None):
        self.archs, self.xs, self.ok = archs, xs, ok
        n = xs[0].size if xs is not None else 0
        self.cap = n if cap is None else cap
        self.out_off, self.init_off = out_off, init_off
        self.size = n if size is None else size


def neg_zero_init(dtype, seed):
    """The `init` of place_words: random finite values over a wide exponent
    range, every fifth word -0.0."""
    def init(total):
        g = torch.Generator().manual_seed(3000 + seed)
        t = (torch.randn(total, generator=g, dtype=torch.float64)
             * torch.exp2(torch.randint(-12, 12, (total,), generator=g).double())).to(dtype)
        t[::5] = -0.0
        return t
    return init


def run(api, C, ws, ft, members, init_form, out_form, pb=10, with_status=True, seed=0, in_place=False):
    """One call over `members` through `api` ("codec" or "capi"); checks status,
    sizes and every word of the out and init buffers against the model."""
    K, nb = len(members[0].archs), len(members)
    out_dt, init_dt = SR.form_dtype(ft, out_form), SR.form_dtype(ft, init_form)
    views = pack_bytes([m.archs[k] for k in range(K) for m in members], [0] * (K * nb))
    sources = [views[k * nb:(k + 1) * nb] for k in range(K)]
    outs, obuf, ohost, ostarts = place_words(out_dt, [m.cap for m in members], [m.out_off for m in members],
                                             neg_zero_init(out_dt, seed))
    inits = ibuf = ihost = istarts = None
    if in_place:
        assert init_dt == out_dt
        inits, ibuf, ihost, istarts = outs, obuf, ohost, ostarts
    elif init_dt is not None:
        inits, ibuf, ihost, istarts = place_words(init_dt, [m.cap for m in members], [m.init_off for m in members],
                                                  neg_zero_init(init_dt, seed + 1))
    ok = torch.full([nb], 7, dtype=torch.uint8, device=DEV) if with_status else None
    sz = torch.full([nb], -7, dtype=torch.int32, device=DEV) if with_status else None
    if api == "codec":
        assert with_status
        ok, sz = C.sparse_reduce(sources, outs, inits=inits, ft=ft, prob_bits=pb, ws=ws)
    else:
        from dietgpu_fork_amd import _native as N

        # (every out's address inside its buffer, also for a capacity of 0)
        rc = N.lib().dietgpu_float_reduce_sparse(
            ws.h, ft, pb, nb, K, N.ptr_array([v.data_ptr() for v in views]),
            N.ptr_array([ibuf.data_ptr() + st * ibuf.element_size() for st in istarts]) if inits is not None else None,
            FT_OF[init_dt] if init_dt is not None else 0,
            N.ptr_array([obuf.data_ptr() + st * obuf.element_size() for st in ostarts]),
            N.u32_array([m.cap for m in members]), FT_OF[out_dt], ok.data_ptr() if with_status else None,
            sz.data_ptr() if with_status else None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.lib().dietgpu_last_error()
    torch.cuda.synchronize()
    if with_status:
        assert ok.cpu().tolist() == [int(m.ok) for m in members]
        assert sz.cpu().tolist() == [m.size for m in members]
    want = ohost.clone()
    for m, st, ist in zip(members, ostarts, istarts or ostarts):
        if m.ok:
            n = m.xs[0].size
            init = ihost[ist:ist + n] if ihost is not None else None
            want[st:st + n] = SR.model(m.xs, ft, init=init, out_dtype=out_dt)
    got = obuf.cpu()
    assert A.same_bits(got, want), A.mismatch_report(got, want)
    if ibuf is not None and not in_place:
        assert torch.equal(A.bits(ibuf.cpu()), A.bits(ihost)), "an init was written"


def member(ft, n, K, seed, pb=10, frac_zero=0.7, **kw):
    pairs = [source(ft, n, seed + k, frac_zero, pb) for k in range(K)]
    return M([a for _, a in pairs], [w for w, _ in pairs], **kw)


def sweep(ft, cases, group):
    """The members of a size sweep at K = 3 (sparse_reduce_cases.sweep_members),
    out and init alternately 16 B-aligned and one word off."""
    ms = []
    for i, (name, xs) in enumerate(SR.sweep_members(cases, ft)):
        archs = [archive_of(x, ft, key=(group, name, k)) for k, x in enumerate(xs)]
        ms.append(M(archs, xs, out_off=i % 2, init_off=(i // 2) % 2))
    return ms


def dev(a):
    return torch.from_numpy(a.copy()).to(DEV)


# ------------------------------------------------------------ size edges ----

@pytest.mark.parametrize("init_form,out_form", SR.FORMS, ids=[f"init-{i}-out-{o}" for i, o in SR.FORMS])
@pytest.mark.parametrize("ft", **FT_PARAMS)
def test_small_sweep(C, ws, ft, init_form, out_form):
    """Every "small" edge element (sizes 0 .. 200 and +-2 around 256, 1024,
    2048, 4096 and 8192, the four tails, the block-edge elements) as x_1 of one
    member of a pointer batch at K = 3; x_2 and x_3 have other fills and other
    tails."""
    ms = _ARCH.get(("small", ft), lambda: sweep(ft, S.small_cases(ft), "small"))
    assert len(ms) > 900 and {(m.out_off, m.init_off) for m in ms} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    run("codec", C, ws, ft, ms, init_form, out_form, seed=ft)


@pytest.mark.parametrize("ft,init_form,out_form", [(1, "T", "T"), (2, "f32", "T"), (2, "none", "f32"), (3, "f32", "f32")],
                         ids=["fp16", "bf16-f32-init", "bf16-no-init", "fp32"])
def test_large_sweep(C, ws, ft, init_form, out_form):
    """The five sizes 262,144 +- 2, the edge of a counting workgroup, at K = 3."""
    ms = _ARCH.get(("large", ft), lambda: sweep(ft, S.large_cases(ft), "large"))
    assert [m.xs[0].size for m in ms] == [SPARSE_LARGE_B + d for d in range(-2, 3)]
    run("codec", C, ws, ft, ms, init_form, out_form, seed=10 + ft)


def test_more_than_64_counting_workgroups(C, ws):
    """The far element (bf16, 66 * 262,144 + 1102 words) at K = 2: its last
    chunks take the second round of totalsShare, in both sources."""
    w = sparse_far_element()
    assert w.size > 65 * SPARSE_LARGE_B
    w2 = np.roll(w, 77777)
    w2[-2:] = (0x3F81, 0)  # the other tail
    run("codec", C, ws, 2, [M([archive_of(w, 2, key="far"), archive_of(w2, 2, key="far2")], [w, w2], out_off=1)],
        "f32", "T", seed=3)


# --------------------------------------------------- K sweep and passes ----

def sweep_sources(K):
    return [source(2, 5000, 200 + k) for k in range(K)]


@pytest.mark.parametrize("K", SR.K_SWEEP)
def test_k_sweep(C, ws, K):
    """One, two, three and more passes at n = 5,000: bf16, alternately with a
    bf16 init and bf16 out, and without an init into fp32."""
    pairs = sweep_sources(K)
    m = M([a for _, a in pairs], [w for w, _ in pairs], out_off=1)
    run("codec", C, ws, 2, [m, m], "T", "T", seed=K)
    run("codec", C, ws, 2, [m], "none", "f32", seed=K)


def test_split_is_invisible(C, ws):
    """K = 9 in one call equals a K = 4 call whose fp32 output is the init of
    a K = 5 call."""
    pairs = sweep_sources(9)
    arch = [dev(a) for _, a in pairs]
    n = 5000
    init = SR.init_fp32(2, n, seed=4)
    whole, part, both = (torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(3))
    for ok, _ in (C.sparse_reduce([[a] for a in arch], [whole], inits=[init.to(DEV)], ft=2, ws=ws),
                  C.sparse_reduce([[a] for a in arch[:4]], [part], inits=[init.to(DEV)], ft=2, ws=ws),
                  C.sparse_reduce([[a] for a in arch[4:]], [both], inits=[part], ft=2, ws=ws)):
        assert ok.cpu().tolist() == [1]
    assert torch.equal(A.bits(whole), A.bits(both))
    want = SR.model([w for w, _ in pairs], 2, init=init)
    assert A.same_bits(whole.cpu(), want), A.mismatch_report(whole.cpu(), want)


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_sources_per_launch_do_not_show(C, ws, ns):
    """K = 7 with the launches capped at 1, 2 and 3 sources (the tuning hook):
    the model's bits, as uncapped."""
    pairs = sweep_sources(7)
    m = M([a for _, a in pairs], [w for w, _ in pairs], out_off=1)
    C.set_reduce_max_sources(ns)
    try:
        run("codec", C, ws, 2, [m, m], "T", "T", seed=ns)
        run("codec", C, ws, 2, [m], "none", "T", seed=ns)
    finally:
        C.set_reduce_max_sources(0)


# -------------------------------------------------------- special values ----

def direct(C, ws, ft, xs, init, out_dt, keys):
    """One member, 16 B-aligned: (out, ok, sz) of sources xs on `init` (CPU or None)."""
    archs = [dev(archive_of(x, ft, key=k)) for x, k in zip(xs, keys)]
    out = torch.ones(xs[0].size, dtype=out_dt, device=DEV)
    init_d = init.to(DEV) if init is not None else None
    ok, sz = C.sparse_reduce([[a] for a in archs], [out], inits=None if init is None else [init_d], ft=ft, ws=ws)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [xs[0].size]
    if init is not None:
        assert torch.equal(A.bits(init_d.cpu()), A.bits(init)), "the init was written"
    return out.cpu()


@pytest.mark.parametrize("out_form", ["T", "f32"])
@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_every_nonzero_16_bit_pattern(C, ws, ft, out_form):
    """Every nonzero 16-bit pattern as x_1 with a zero word after each, over
    the fixed fp32 accumulators and a signalling NaN, with the same vector
    rolled by an odd count as x_2 (its zeros under x_1's patterns)."""
    x1, acc = S.patterns16_interleaved(ft, 2)
    x2 = np.roll(x1, 12345)
    out_dt = SR.form_dtype(ft, out_form)
    got = direct(C, ws, ft, [x1, x2], acc, out_dt, [("pat1",), ("pat2",)])
    want = SR.model([x1, x2], ft, init=acc, out_dtype=out_dt)
    assert A.same_bits(got, want), A.mismatch_report(got, want)


def test_fp32_special_values_crossed(C, ws):
    """The fp32 special table crossed with itself, zeros interleaved, as x_1
    over an init of specials; x_2 the same words rolled by one."""
    x1, acc = S.cross_specials_interleaved(3)
    x2 = np.roll(x1, 1)
    got = direct(C, ws, 3, [x1, x2], acc, torch.float32, [("cross1",), ("cross2",)])
    want = SR.model([x1, x2], 3, init=acc)
    assert A.same_bits(got, want), A.mismatch_report(got, want)


@pytest.mark.parametrize("ft", **FT_PARAMS)
def test_order_probe(C, ws, ft):
    init, xs = R.order_probe(ft)
    ws_ = [A.float_to_words(x, ft) for x in xs]
    assert all((w != 0).all() for w in ws_)
    got = direct(C, ws, ft, ws_, init, torch.float32, [None] * 3)
    want = R.model(xs, init=init)
    assert torch.equal(A.bits(got), A.bits(want)), (got.tolist(), want.tolist())


@pytest.mark.parametrize("ft", **FT_PARAMS)
def test_one_source_no_init_returns_the_element(C, ws, ft):
    """K = 1 without an init: the decoded element bit for bit, its -0.0 kept
    and +0.0 at the clear bits."""
    w = random_words(ft, 4099, 0.6, seed=5)
    x = A.words_to_float(w, ft)
    assert bool((A.bits(x) == A.bits(torch.tensor([-0.0], dtype=x.dtype))).any()) and bool((A.bits(x) == 0).any())
    got = direct(C, ws, ft, [w], None, x.dtype, [None])
    assert torch.equal(A.bits(got), A.bits(x))


@pytest.mark.parametrize("ft,form", [(1, "T"), (2, "T"), (2, "f32"), (3, "f32")], ids=["fp16", "bf16", "bf16-f32", "fp32"])
def test_all_zero_sources_leave_the_init(C, ws, ft, form):
    """Three all-zero sources: an init of -0.0, denormals and the other finite
    specials comes out bit for bit after the widening and the one rounding."""
    dt = SR.form_dtype(ft, form)
    s = A.specials(FT_OF[dt])
    s = s[~torch.isnan(s)]
    init = torch.cat([s.repeat(300), torch.full((77,), -0.0, dtype=dt)])
    z = np.zeros(init.numel(), dtype=NP_WORD[ft])
    got = direct(C, ws, ft, [z, z, z], init, dt, [("zeros", init.numel())] * 3)
    assert torch.equal(A.bits(got), A.bits(init))


@pytest.mark.parametrize("ft,form", [(1, "T"), (2, "T"), (2, "f32"), (3, "f32")], ids=["fp16", "bf16", "bf16-f32", "fp32"])
def test_in_place(C, ws, ft, form):
    """out is init: the same pointers and the same type."""
    ms = [member(ft, n, 3, seed=300 + i, out_off=i % 2) for i, n in enumerate((70001, 8, 4097, 1025))]
    run("codec", C, ws, ft, ms, form, form, in_place=True, seed=3)


# ------------------------------------------------------ failure contract ----

def failure_members(ft):
    good = member(ft, 5000, 3, seed=400)
    short = member(ft, 4097, 3, seed=410)
    base = member(ft, 4200, 3, seed=420)
    n = 4200

    def second_replaced(blob):
        return [base.archs[0], blob, base.archs[2]]

    other_type = retyped(base.archs[1], ft, at=dense_at(n) + 8)  # the dense header names another float type
    pb9 = source(ft, n, 421, pb=9)[1]  # the same words at other prob bits
    magic = base.archs[1].copy()
    magic[dense_at(n)] ^= 0x40  # the dense magic word
    return [
        good,
        M(short.archs, short.xs, cap=4096, ok=False),                                        # one word short
        M(second_replaced(source(ft, 4201, 433)[1]), None, cap=4300, out_off=1, ok=False, size=n),  # another n
        M(second_replaced(other_type), None, cap=n, ok=False, size=n),
        M(second_replaced(pb9), None, cap=n, init_off=1, ok=False, size=n),
        M(second_replaced(magic), None, cap=n, ok=False, size=n),
        M([base.archs[0], base.archs[1], magic], None, cap=n, out_off=1, ok=False, size=n),  # the last archive is bad
        M([source(ft, 4199, 434)[1], base.archs[1], base.archs[2]], None, cap=n, ok=False, size=4199),  # the first differs
        member(ft, 8, 3, seed=440, out_off=1),
        M(short.archs, short.xs, cap=4100),                                                  # room to spare
    ]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("ft,init_form,out_form", [(2, "T", "T"), (2, "f32", "f32"), (1, "none", "T"),
                                                   (3, "f32", "f32")],
                         ids=["bf16", "bf16-f32", "fp16-no-init", "fp32"])
def test_failure_contract(C, ws, ft, init_form, out_form, with_status):
    """Good and failing members in one batch: status 0 and the first source's
    n for every failing one, its out and init untouched, the good ones exact."""
    run("capi", C, ws, ft, failure_members(ft), init_form, out_form, with_status=with_status, seed=9)


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
def test_failure_contract_across_passes(C, ws, with_status):
    """K = 9 (three passes): a bad ninth archive, or one of another n, leaves
    out untouched although the first two passes never see it."""
    n = 4200
    pairs = [source(2, n, 450 + k) for k in range(9)]
    archs = [a for _, a in pairs]
    bad = archs[8].copy()
    bad[dense_at(n)] ^= 0x40
    ms = [M(archs, [w for w, _ in pairs]), M(archs[:8] + [bad], None, cap=n, out_off=1, ok=False, size=n),
          M(archs[:8] + [source(2, 4201, 460)[1]], None, cap=4300, ok=False, size=n),
          M(archs, [w for w, _ in pairs], cap=n + 5, out_off=1, init_off=1)]
    run("capi", C, ws, 2, ms, "T", "T", with_status=with_status, seed=11)


# ------------------------------------------------------- other call forms ----

@pytest.mark.parametrize("ft", [2, 3], ids=["bf16", "fp32"])
def test_reference_legal_archives(C, ws, ft):
    """Archives as the reference may emit them: a garbage word in the n-2 slot
    of the list, 0xFF in the bitmap's padding bytes, (n % 8 != 0) set bits past
    n in its last byte, and 0xFF in header bytes 4 .. 15.  None reaches a sum."""
    els = {name: w for _, name, w in S.edge_elements(ft)}
    ms = []
    for B in (64, 256, 1024, 4096):
        for name in (f"n{B + 1}_{('zero', 'half', 'dense')[(B + 1) % 3]}_t01",
                     f"n{B}_{('zero', 'half', 'dense')[B % 3]}_t00"):
            w = els[name]
            n = w.size
            assert w[n - 2] == 0
            plain = archive_of(w, ft, key=("legal", name))
            v = pyref.sparse_compress(ft, w, 10, gap_fill=GARBAGE[ft], pad_fill=0xFF, pad_bits=bool(n % 8)).copy()
            assert v.size == plain.size and not np.array_equal(v, plain)
            v[4:16] = 0xFF
            xs = [w, SR.companion(ft, w, 1, 1), w]
            ms.append(M([v, archive_of(xs[1], ft, key=("legal2", name)), v], xs, cap=n + 3 * (len(ms) % 2),
                        out_off=len(ms) % 2))
    run("codec", C, ws, ft, ms, "f32", "T", seed=5)


@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, pb):
    ms = [member(2, n, 3, seed=500 + pb, pb=pb, out_off=i) for i, n in enumerate((70001, 9))]
    run("codec", C, ws, 2, ms, "T", "T", pb=pb)
    run("capi", C, ws, 2, ms, "none", "f32", pb=pb)


def test_checksummed_archives_reduce(C, ws):
    pairs = [source(2, 12345, 510 + k, checksum=True) for k in range(2)]
    assert not np.array_equal(pairs[0][1], source(2, 12345, 510)[1])
    m = M([a for _, a in pairs], [w for w, _ in pairs])
    run("codec", C, ws, 2, [m, m], "f32", "T")


@pytest.mark.parametrize("ft", **FT_PARAMS)
def test_gpu_compressed_archives(C, ws, ft):
    xs = [random_words(ft, 70001, 0.9, seed=520 + k) for k in range(3)]
    comp, sizes = C.sparse_compress([A.words_to_float(x, ft).to(DEV) for x in xs], ft=ft, ws=ws)
    archs = [comp[i, : int(sizes[i])].cpu().numpy() for i in range(3)]
    run("codec", C, ws, ft, [M(archs, xs, out_off=1)], "T", "T")


def test_side_stream(C, ws):
    m = member(1, 32769, 3, seed=530)
    views = pack_bytes(m.archs, [0, 0, 0])
    out = torch.zeros(32769, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ok, sz = C.sparse_reduce([[v] for v in views], [out], ft=1, ws=ws)
    s.synchronize()
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [32769]
    want = SR.model(m.xs, 1)
    assert A.same_bits(out.cpu(), want), A.mismatch_report(out.cpu(), want)


def test_401_member_batch(C, ws):
    ms = []
    for i in range(401):
        ms.append(member(2, 1 + (37 * i) % 700, 2, seed=540 + 2 * (i % 8), frac_zero=0.5, out_off=i % 2,
                         init_off=(i // 2) % 2))
    run("codec", C, ws, 2, ms, "T", "f32")
    run("capi", C, ws, 2, ms, "none", "T")


def test_c_abi(C, ws):
    """The C ABI through ctypes, every float type, with and without status."""
    for ft, init_form, out_form in ((1, "f32", "T"), (2, "T", "f32"), (3, "none", "f32")):
        ms = [member(ft, n, 3, seed=560 + ft, out_off=k, init_off=1 - k) for k, n in enumerate((4097, 1025))]
        run("capi", C, ws, ft, ms, init_form, out_form)
        run("capi", C, ws, ft, ms, init_form, out_form, with_status=False)


def test_cpp_entry_point_rejects_checksum_and_bad_types(C, ws):
    from dietgpu_fork_amd import _native as N

    T = N.testlib()
    w, a = source(2, 4097, 1)
    arch = dev(a)
    init = SR.init_fp32(2, 4097, seed=51)
    init_d = init.to(DEV)
    out = torch.ones(4097, dtype=torch.bfloat16, device=DEV)
    ok = torch.full([1], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([1], -7, dtype=torch.int32, device=DEV)

    def hook(ft=2, checksum=0, k=1, init_type=3, out_type=2):
        rc = T.dietgpu_test_sparse_reduce_config(ws.h, ft, checksum, k, N.ptr_array([arch.data_ptr()] * max(k, 1)),
                                                 init_d.data_ptr(), init_type, out.data_ptr(), 4097, out_type,
                                                 ok.data_ptr(), sz.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return rc, T.dietgpu_test_last_error().decode()

    rc, msg = hook(checksum=1)
    assert rc == N.DIETGPU_ERR_INVALID and "cannot verify a checksum" in msg
    for k in (0, 65):
        rc, msg = hook(k=k)
        assert rc == N.DIETGPU_ERR_INVALID and "must be in 1 .. 64" in msg
    rc, msg = hook(ft=4, init_type=4, out_type=4)
    assert rc == N.DIETGPU_ERR_INVALID and "fp16, bf16 or fp32 archives" in msg
    for out_type in (1, 4, 0):
        rc, msg = hook(out_type=out_type)
        assert rc == N.DIETGPU_ERR_INVALID and f"out type {out_type} does not go with float type 2" in msg
    for init_type in (1, 4, 0):
        rc, msg = hook(init_type=init_type)
        assert rc == N.DIETGPU_ERR_INVALID and f"init type {init_type} does not go with float type 2" in msg
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and ok.item() == 7 and sz.item() == -7
    assert torch.equal(A.bits(init_d.cpu()), A.bits(init))
    rc, msg = hook()  # and the good call goes through
    assert rc == 0, msg
    torch.cuda.synchronize()
    want = SR.model([w], 2, init=init, out_dtype=torch.bfloat16)
    assert ok.item() == 1 and sz.item() == 4097 and A.same_bits(out.cpu(), want)


def test_graph_capture_replay(C):
    """One K = 3 reduce captured in a hipGraph and replayed twice, new archive
    bytes with other nonzero counts copied into the same buffers in between."""
    ws = C.Workspace(16 << 20)
    n = 40000
    rounds = [[source(2, n, 600 + 3 * r + k, frac_zero=(0.9, 0.5, 0.7)[r]) for k in range(3)] for r in range(3)]
    room = max(a.size for row in rounds for _, a in row)
    slots = [torch.zeros(room, dtype=torch.uint8, device=DEV) for _ in range(3)]
    init = S.case_acc(2, 1, n, seed=4)
    init_d = init.to(DEV)
    out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)

    def load(r):
        for slot, (_, a) in zip(slots, rounds[r]):
            slot[: a.size].copy_(torch.from_numpy(a.copy()))

    load(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.sparse_reduce([[s] for s in slots], [out], inits=[init_d], ft=2, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        ok, sz = C.sparse_reduce([[s] for s in slots], [out], inits=[init_d], ft=2, ws=ws)
    for r in (1, 2):
        load(r)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [n]
        want = SR.model([w for w, _ in rounds[r]], 2, init=init, out_dtype=torch.bfloat16)
        assert A.same_bits(out.cpu(), want), f"replay {r}: " + A.mismatch_report(out.cpu(), want)


# ----------------------------------------------------------- collectives ----

def per_peer_loop(codec, own, archives, dtype):
    """Today's loop, by calling codec.accumulate directly."""
    if own is None:
        n = codec.info(archives[0])[0]
        own = torch.empty(n, dtype=dtype, device=DEV)
        codec.decompress([archives[0]], [own])
        archives = archives[1:]
    acc = own.to(torch.float32, copy=True)
    for a in archives:
        codec.accumulate([a], [acc])
    return acc.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_reduce_archives_fused_equals_model_and_loop(pg, C, dtype):
    """own + 7 GPU-compressed sparse peers, n = 70,001: the model's bits and the
    per-peer loop's, with and without own; the fused call launches the
    "sparse_reduce" family and no "sparse_accumulate"; a codec whose workspace
    is too small for the plan keeps the loop and gives the same bits."""
    from dietgpu_fork_amd import dist as D

    ft = FT_OF[dtype]
    n = 70001
    own = S.case_acc(ft, 1, n, seed=800)
    peers = [random_words(ft, n, 0.9, seed=810 + k) for k in range(7)]
    codec = D.GpuSparseFloatCodec()
    comp, sizes = codec.compress([A.words_to_float(p, ft).to(DEV) for p in peers])
    archives = [comp[i, : int(sizes[i])] for i in range(7)]
    small = D.GpuSparseFloatCodec(workspace_bytes=512 << 10)
    assert codec.reduce_fits(n, dtype, 7) and not small.reduce_fits(n, dtype, 7)
    C.profile(True)
    try:
        C.profile_reset()
        got = D.reduce_archives(own.to(DEV), archives, codec)
        torch.cuda.synchronize()
        assert C.profile_query("sparse_reduce")[1] >= 1 and C.profile_query("sparse_accumulate")[1] == 0
        C.profile_reset()
        routed = D.reduce_archives(own.to(DEV), archives, small)
        torch.cuda.synchronize()
        assert C.profile_query("sparse_reduce")[1] == 0 and C.profile_query("sparse_accumulate")[1] == 14
    finally:
        C.profile(False)
    want = SR.model(peers, ft, init=own.float(), out_dtype=dtype)
    assert not bool(torch.isnan(want).any())
    assert got.dtype == dtype and A.same_bits(got.cpu(), want), A.mismatch_report(got.cpu(), want)
    assert torch.equal(A.bits(got), A.bits(per_peer_loop(codec, own.to(DEV), archives, dtype)))
    assert torch.equal(A.bits(got), A.bits(routed))
    # own=None: the first archive stands in for it
    got = D.reduce_archives(None, archives, codec)
    want = SR.model(peers, ft, out_dtype=dtype)
    assert got.dtype == dtype and A.same_bits(got.cpu(), want), A.mismatch_report(got.cpu(), want)
    assert torch.equal(A.bits(got), A.bits(per_peer_loop(codec, None, archives, dtype)))
    assert torch.equal(A.bits(got), A.bits(D.reduce_archives(None, archives, small)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_world_of_one_still_returns_its_input(pg, dtype):
    from dietgpu_fork_amd import dist as D

    codec = D.GpuSparseFloatCodec()
    x = A.words_to_float(random_words(FT_OF[dtype], 12345, 0.9, seed=7), FT_OF[dtype]).to(DEV)
    y = D.reduce_scatter_compressed([x], codec=codec)
    assert y.dtype == dtype and torch.equal(A.bits(y), A.bits(x))
    z = D.all_reduce_compressed(x.view(3, 4115), codec=codec)
    assert z.shape == (3, 4115) and torch.equal(A.bits(z.view(-1)), A.bits(x))
