"""GPU tests of the fused multi-archive reduce: K archives per
member decoded side by side and summed in registers by k_reduce, through
codec.float_reduce, the C ABI, torch.ops.dietgpu.reduce_data and the reducing
collectives of dist.py.

The model is torch on the CPU (tests/reduce_cases.py), never the code under
test; results are compared with accumulate_cases.same_bits: bit for bit
wherever the model is not a NaN, a NaN where it is.  Archives come from the
CPU oracle unless a test says otherwise.  The outputs (and the inits) of a
call live in one buffer of random finite values with at least 16 guard words
between members; the buffers are compared whole, so a stray write, or any
write to a failing member, fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import accumulate_cases as A
from tests import reduce_cases as R
from tests.dist_cases import pg  # noqa: F401
from tests.gpu_harness import C, DEV, Cache, pack_bytes, place_words, workspace_fixture  # noqa: F401
from tests.util import FT_OF

pytestmark = pytest.mark.gpu

ws = workspace_fixture(64 << 20)
_ARCH = Cache()


def archive_of(x, ft, pb=10, checksum=False, key=None):
    """The oracle's archive of float CPU tensor x (cached under `key`)."""
    def make():
        return O.float_compress(A.float_to_words(x, ft), ft, pb, checksum)
    return make() if key is None else _ARCH.get((key, pb, checksum), make)


def source(ft, n, seed, pb=10, checksum=False):
    """(values, archive) of one random source (cached)."""
    key = ("src", ft, n, seed)
    x = _ARCH.get(key, lambda: A.random_acc(ft, 1, n, seed=seed))
    return x, archive_of(x, ft, pb, checksum, key=key)


class M:
    """One member: its K archives (bytes), the K value vectors (None: the
    member must fail), the capacity, and the alignments (words past a 16 B
    boundary for out / init, bytes for each archive)."""

    def __init__(self, archs, xs, cap=None, out_off=0, init_off=0, arch_offs=None, ok=True, size=None):
        self.archs, self.xs, self.ok = archs, xs, ok
        n = xs[0].numel() if xs is not None else 0
        self.cap = n if cap is None else cap
        self.out_off, self.init_off = out_off, init_off
        self.arch_offs = arch_offs or [0] * len(archs)
        self.size = (n if ok else 0) if size is None else size


def random_init(dtype, seed):
    """The `init` of place_words: random finite values over a wide exponent
    range."""
    def init(total):
        g = torch.Generator().manual_seed(2000 + seed)
        return (torch.randn(total, generator=g, dtype=torch.float64)
                * torch.exp2(torch.randint(-12, 12, (total,), generator=g).double())).to(dtype)
    return init


def run(api, C, ws, ft, members, init_form, out_form, pb=10, with_status=True, temp_mem=True, seed=0, in_place=False):
    """One call over `members` through `api`; checks status, sizes and every
    word of the out and init buffers against the model."""
    K, nb = len(members[0].archs), len(members)
    out_dt, init_dt = R.form_dtype(ft, out_form), R.form_dtype(ft, init_form)
    views = pack_bytes([a for k in range(K) for m in members for a in [m.archs[k]]],
                       [m.arch_offs[k] for k in range(K) for m in members])
    sources = [views[k * nb:(k + 1) * nb] for k in range(K)]
    outs, obuf, ohost, ostarts = place_words(out_dt, [m.cap for m in members], [m.out_off for m in members],
                                             random_init(out_dt, seed))
    inits = ibuf = ihost = istarts = None
    if in_place:
        assert init_dt == out_dt
        inits, ibuf, ihost, istarts = outs, obuf, ohost, ostarts
    elif init_dt is not None:
        inits, ibuf, ihost, istarts = place_words(init_dt, [m.cap for m in members], [m.init_off for m in members],
                                                  random_init(init_dt, seed + 1))
    ok = torch.full([nb], 7, dtype=torch.uint8, device=DEV) if with_status else None
    sz = torch.full([nb], -7, dtype=torch.int32, device=DEV) if with_status else None
    if api == "codec":
        assert with_status
        ok, sz = C.float_reduce(sources, outs, inits=inits, ft=ft, prob_bits=pb, ws=ws)
    elif api == "op":
        assert pb == 10
        used = torch.ops.dietgpu.reduce_data(views, K, outs, inits, ws.buf if temp_mem else None, ok, sz)
        assert isinstance(used, int) and used >= 0
    else:
        from dietgpu_fork_amd import _native as N

        rc = N.lib().dietgpu_float_reduce(
            ws.h, ft, pb, nb, K, N.ptr_array([v.data_ptr() for v in views]),
            N.ptr_array([t.data_ptr() for t in inits]) if inits is not None else None,
            FT_OF[init_dt] if init_dt is not None else 0, N.ptr_array([o.data_ptr() for o in outs]),
            N.u32_array([o.numel() for o in outs]), FT_OF[out_dt], ok.data_ptr() if with_status else None,
            sz.data_ptr() if with_status else None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.lib().dietgpu_last_error()
    torch.cuda.synchronize()
    if with_status:
        assert ok.cpu().tolist() == [int(m.ok) for m in members]
        assert sz.cpu().tolist() == [m.size for m in members]
    want = ohost.clone()
    for m, st, ist in zip(members, ostarts, istarts or ostarts):
        if m.ok:
            n = m.xs[0].numel()
            init = ihost[ist:ist + n] if ihost is not None else None
            want[st:st + n] = R.model(m.xs, init=init, out_dtype=out_dt)
    got = obuf.cpu()
    assert A.same_bits(got, want), A.mismatch_report(got, want)
    if ibuf is not None and not in_place:
        assert torch.equal(A.bits(ibuf.cpu()), A.bits(ihost)), "an init was written"


def member(ft, n, K, seed, pb=10, **kw):
    pairs = [source(ft, n, seed + k, pb) for k in range(K)]
    return M([a for _, a in pairs], [x for x, _ in pairs], **kw)


# ------------------------------------------------------------ size edges ----

@pytest.mark.parametrize("init_form,out_form", R.FORMS, ids=[f"init-{i}-out-{o}" for i, o in R.FORMS])
@pytest.mark.parametrize("ft", R.FTS, ids=[A.FT_IDS[ft] for ft in R.FTS])
def test_size_edges(C, ws, ft, init_form, out_form):
    """One pointer batch of members of every edge size, K = 3; out and init
    16 B-aligned or one word off, each source on its own 16 B-aligned or 4 B
    off."""
    members = []
    for i, n in enumerate(A.SIZES):
        members.append(member(ft, n, 3, seed=100 + i, out_off=i % 2, init_off=(i // 2) % 2,
                              arch_offs=[4 * ((i >> k) & 1) for k in range(3)]))
    assert {tuple(m.arch_offs) for m in members} >= {(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4)}
    assert {(m.out_off, m.init_off) for m in members} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    run("codec", C, ws, ft, members, init_form, out_form, seed=ft)


# --------------------------------------------------------------- K sweep ----

def sweep_sources(K):
    return [source(2, 33001, 200 + k) for k in range(K)]


@pytest.mark.parametrize("K", R.K_SWEEP)
def test_k_sweep(C, ws, K):
    """One, two, three and more passes: bf16, fp32 output, no init."""
    pairs = sweep_sources(K)
    run("codec", C, ws, 2, [M([a for _, a in pairs], [x for x, _ in pairs], out_off=1)], "none", "f32", seed=K)


def test_split_is_invisible(C, ws):
    """K = 9 in one call equals a K = 4 call whose fp32 output is the init of
    a K = 5 call."""
    pairs = sweep_sources(9)
    arch = [torch.from_numpy(a.copy()).to(DEV) for _, a in pairs]
    n = 33001
    whole = torch.zeros(n, dtype=torch.float32, device=DEV)
    part = torch.zeros(n, dtype=torch.float32, device=DEV)
    both = torch.zeros(n, dtype=torch.float32, device=DEV)
    for ok, _ in (C.float_reduce([[a] for a in arch], [whole], ft=2, ws=ws),
                  C.float_reduce([[a] for a in arch[:4]], [part], ft=2, ws=ws),
                  C.float_reduce([[a] for a in arch[4:]], [both], inits=[part], ft=2, ws=ws)):
        assert ok.cpu().tolist() == [1]
    assert torch.equal(A.bits(whole), A.bits(both))
    want = R.model([x for x, _ in pairs])
    assert A.same_bits(whole.cpu(), want), A.mismatch_report(whole.cpu(), want)


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_sources_per_launch_do_not_show(C, ws, ns):
    """K = 7 with the launches capped at 1, 2 and 3 sources (the tuning hook):
    the bits of the uncapped call, bf16 output on a bf16 init."""
    pairs = sweep_sources(7)
    m = M([a for _, a in pairs[:7]], [x for x, _ in pairs[:7]], out_off=1)
    C.set_reduce_max_sources(ns)
    try:
        run("codec", C, ws, 2, [m, m], "T", "T", seed=ns)
    finally:
        C.set_reduce_max_sources(0)


# ------------------------------------------------------------ arithmetic ----

@pytest.mark.parametrize("out_form", ["T", "f32"])
@pytest.mark.parametrize("ft", [1, 2], ids=["fp16", "bf16"])
def test_every_16_bit_pattern(C, ws, ft, out_form):
    """Every 16-bit pattern as x_1 on top of the 16 fixed fp32 accumulators
    and a random vector, with x_2 a second fixed pattern vector."""
    xw, acc = A.arithmetic16(ft, 2)
    x1 = A.words_to_float(xw, ft)
    x2 = A.words_to_float(np.roll(xw, 12345), ft)
    archs = [archive_of(x1, ft, key=("pat1", ft)), archive_of(x2, ft, key=("pat2", ft))]
    out_dt = R.form_dtype(ft, out_form)
    init = acc.to(DEV)
    out = torch.zeros(x1.numel(), dtype=out_dt, device=DEV)
    ok, sz = C.float_reduce([[torch.from_numpy(a.copy()).to(DEV)] for a in archs], [out], inits=[init], ft=ft, ws=ws)
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [x1.numel()]
    want = R.model([x1, x2], init=acc, out_dtype=out_dt)
    assert A.same_bits(out.cpu(), want), A.mismatch_report(out.cpu(), want)
    assert torch.equal(A.bits(init.cpu()), A.bits(acc))


def test_fp32_special_values_crossed(C, ws):
    """The fp32 special table crossed with itself as (x_1, x_2) over an init of
    specials, plus 1e5 random triples with cancellations."""
    x1, x2 = A.cross_specials(3)
    s = A.specials(3)
    init = torch.cat([s.repeat(x1.numel() // s.numel() + 1)[: 256], A.cross_specials(3, seed=9)[0][256:]])
    init[256::97] = -(x1[256::97] + x2[256::97])  # the three terms cancel
    assert init.numel() == x1.numel()
    archs = [torch.from_numpy(archive_of(x, 3).copy()).to(DEV) for x in (x1, x2)]
    out = torch.zeros(x1.numel(), dtype=torch.float32, device=DEV)
    ok, _ = C.float_reduce([[a] for a in archs], [out], inits=[init.to(DEV)], ft=3, ws=ws)
    assert ok.cpu().tolist() == [1]
    want = R.model([x1, x2], init=init)
    assert A.same_bits(out.cpu(), want), A.mismatch_report(out.cpu(), want)


@pytest.mark.parametrize("ft", R.FTS, ids=[A.FT_IDS[ft] for ft in R.FTS])
def test_order_probe(C, ws, ft):
    init, xs = R.order_probe(ft)
    archs = [torch.from_numpy(archive_of(x, ft).copy()).to(DEV) for x in xs]
    out = torch.zeros(init.numel(), dtype=torch.float32, device=DEV)
    ok, _ = C.float_reduce([[a] for a in archs], [out], inits=[init.to(DEV)], ft=ft, ws=ws)
    assert ok.cpu().tolist() == [1]
    want = R.model(xs, init=init)
    assert torch.equal(A.bits(out.cpu()), A.bits(want)), (out.cpu().tolist(), want.tolist())


@pytest.mark.parametrize("ft", R.FTS, ids=[A.FT_IDS[ft] for ft in R.FTS])
def test_one_source_no_init_returns_the_element(C, ws, ft):
    """K = 1 without an init: the decoded element bit for bit, -0.0 included."""
    x = A.random_acc(ft, 1, 4099, seed=5)
    x[::5] = -0.0
    out = torch.ones(4099, dtype=x.dtype, device=DEV)
    ok, _ = C.float_reduce([[torch.from_numpy(archive_of(x, ft).copy()).to(DEV)]], [out], ft=ft, ws=ws)
    assert ok.cpu().tolist() == [1] and torch.equal(A.bits(out.cpu()), A.bits(x))


# -------------------------------------------------------------- in place ----

@pytest.mark.parametrize("ft,form", [(1, "T"), (2, "T"), (2, "f32"), (3, "f32")],
                         ids=["fp16", "bf16", "bf16-f32", "fp32"])
def test_in_place(C, ws, ft, form):
    """out is init: the same pointers and the same type."""
    members = [member(ft, n, 3, seed=300 + i, out_off=i % 2) for i, n in enumerate((70001, 8, 4097, 32769))]
    run("codec", C, ws, ft, members, form, form, in_place=True, seed=3)


# ------------------------------------------------------ failure contract ----

def failure_members(ft):
    other = 1 if ft != 1 else 2
    good = member(ft, 5000, 3, seed=400)
    short = member(ft, 4097, 3, seed=410)
    base = member(ft, 4200, 3, seed=420)

    def second_replaced(blob):
        return [base.archs[0], blob, base.archs[2]]

    bad = base.archs[1].copy()
    bad[0] ^= 0x40  # the magic word
    return [
        good,
        M(short.archs, short.xs, cap=4096, ok=False, size=4097),                            # one word short
        M(second_replaced(source(other, 4200, 431)[1]), None, cap=4200, out_off=1, ok=False),  # another float type
        M(second_replaced(source(ft, 4200, 432, pb=9)[1]), None, cap=4200, ok=False),       # other prob bits
        M(second_replaced(bad), None, cap=4200, arch_offs=[0, 4, 0], ok=False),             # corrupt magic
        M(second_replaced(source(ft, 4201, 433)[1]), None, cap=4300, init_off=1, ok=False),  # another n
        M([base.archs[0], base.archs[1], bad], None, cap=4200, ok=False),                   # the last archive is bad
        member(ft, 8, 3, seed=440, out_off=1),
        M(short.archs, short.xs, cap=4100),                                                 # room to spare
    ]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("ft,init_form,out_form", [(2, "T", "T"), (2, "f32", "f32"), (1, "none", "T"),
                                                   (3, "f32", "f32")],
                         ids=["bf16", "bf16-f32", "fp16-no-init", "fp32"])
def test_failure_contract(C, ws, ft, init_form, out_form, with_status):
    """Good and failing members in one batch: the good ones exact, every
    failing member's out and init untouched."""
    run("capi", C, ws, ft, failure_members(ft), init_form, out_form, with_status=with_status, seed=9)


def test_failure_contract_across_passes(C, ws):
    """K = 9 (three passes): a bad ninth archive leaves out untouched although
    the first two passes never decode it."""
    pairs = [source(2, 4200, 450 + k) for k in range(9)]
    archs = [a for _, a in pairs]
    bad = archs[8].copy()
    bad[0] ^= 0x40
    ms = [M(archs, [x for x, _ in pairs]), M(archs[:8] + [bad], None, cap=4200, ok=False),
          M(archs[:8] + [source(2, 4201, 460)[1]], None, cap=4300, ok=False)]
    run("codec", C, ws, 2, ms, "T", "T", seed=11)


def test_checksum_config_is_refused(C, ws):
    from dietgpu_fork_amd import _native as N

    x, a = source(2, 4097, 1)
    arch = torch.from_numpy(a.copy()).to(DEV)
    out = torch.ones(4097, dtype=torch.bfloat16, device=DEV)
    ok = torch.full([1], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([1], -7, dtype=torch.int32, device=DEV)
    T = N.testlib()

    def hook(checksum, k=1):
        rc = T.dietgpu_test_reduce_config(ws.h, 2, checksum, k, N.ptr_array([arch.data_ptr()] * max(k, 1)),
                                          out.data_ptr(), 4097, ok.data_ptr(), sz.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        return rc, T.dietgpu_test_last_error().decode()

    rc, msg = hook(1)
    assert rc == N.DIETGPU_ERR_INVALID and "cannot verify a checksum" in msg
    for k in (0, 65):
        rc, msg = hook(0, k)
        assert rc == N.DIETGPU_ERR_INVALID and "must be in 1 .. 64" in msg
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and ok.item() == 7 and sz.item() == -7
    rc, msg = hook(0)  # and the good call goes through
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert ok.item() == 1 and sz.item() == 4097 and torch.equal(A.bits(out.cpu()), A.bits(x))


# ------------------------------------------------------- other call forms ----

@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, pb):
    """9 and 11 probability bits; K = 4 at 11 bits is the LDS-heaviest launch
    (four 16 KB tables, the largest instance shipped)."""
    ms = [member(2, n, 4, seed=500 + pb, pb=pb, out_off=i) for i, n in enumerate((70001, 9))]
    run("codec", C, ws, 2, ms, "T", "T", pb=pb)
    run("capi", C, ws, 2, ms, "none", "f32", pb=pb)


def test_checksummed_archives_reduce(C, ws):
    pairs = [source(2, 12345, 510 + k, checksum=True) for k in range(2)]
    assert pairs[0][1][8:12].view(np.uint32)[0] != 2  # the type word carries the checksum flag
    m = M([a for _, a in pairs], [x for x, _ in pairs])
    for api in ("codec", "op"):
        run(api, C, ws, 2, [m, m], "f32", "T")


@pytest.mark.parametrize("ft", R.FTS, ids=[A.FT_IDS[ft] for ft in R.FTS])
def test_gpu_compressed_archives(C, ws, ft):
    xs = R.sources(ft, 3, 70001, seed=520)
    comp, sizes = C.float_compress_pointer([x.to(DEV) for x in xs], ft=ft, ws=ws)
    archs = [comp[i, : int(sizes[i])].cpu().numpy() for i in range(3)]
    run("codec", C, ws, ft, [M(archs, xs)], "T", "T")


def test_side_stream(C, ws):
    m = member(1, 32769, 3, seed=530)
    views = pack_bytes(m.archs, [0, 0, 0])
    out = torch.zeros(32769, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ok, sz = C.float_reduce([[v] for v in views], [out], ft=1, ws=ws)
    s.synchronize()
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [32769]
    want = R.model(m.xs)
    assert A.same_bits(out.cpu(), want), A.mismatch_report(out.cpu(), want)


def test_401_member_batch(C, ws):
    """More members than ride in the kernel arguments: the tables are uploaded."""
    ms = []
    for i in range(401):
        ms.append(member(2, 1 + (37 * i) % 700, 2, seed=540 + 2 * (i % 8), out_off=i % 2))
    run("codec", C, ws, 2, ms, "T", "f32")
    run("op", C, ws, 2, ms, "none", "T")


@pytest.mark.parametrize("temp_mem", [True, False], ids=["temp_mem", "no-temp_mem"])
@pytest.mark.parametrize("ft,init_form,out_form", [(1, "T", "T"), (2, "none", "T"), (2, "f32", "T"), (2, "T", "f32"),
                                                   (2, "none", "f32"), (2, "f32", "f32"), (3, "f32", "f32"),
                                                   (3, "none", "f32")],
                         ids=["fp16", "bf16-no-init", "bf16-f32-init", "bf16-f32-out", "bf16-header-no-init",
                              "bf16-header", "fp32", "fp32-no-init"])
def test_torch_operator(C, ws, ft, init_form, out_form, temp_mem):
    """The operator takes the archives' type from the 16-bit outs or inits, or
    from the first archive's header."""
    ms = [member(ft, n, 3, seed=550 + n % 7, out_off=i % 2) for i, n in enumerate((4097, 9, 32768))]
    run("op", C, ws, ft, ms, init_form, out_form, temp_mem=temp_mem)
    run("op", C, ws, ft, ms, init_form, out_form, temp_mem=temp_mem, with_status=False)


def test_operator_chained_passes_need_room(C, ws):
    """K = 9 through the operator: the fp32 partial comes from temp_mem (or,
    without it, from the arena's overflow)."""
    pairs = [source(2, 4200, 450 + k) for k in range(9)]
    m = M([a for _, a in pairs], [x for x, _ in pairs])
    run("op", C, ws, 2, [m, m], "T", "T")
    run("op", C, ws, 2, [m], "T", "T", temp_mem=False)


def test_operator_rejections_on_device_tensors(C, ws):
    D = torch.ops.dietgpu
    a = torch.from_numpy(source(2, 4097, 1)[1].copy()).to(DEV)
    out = torch.zeros(4097, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="must be uint8"):
        D.reduce_data([a.view(torch.int8)], 1, [out])
    with pytest.raises(RuntimeError, match="archive header"):
        D.reduce_data([a[:16]], 1, [out])
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        D.reduce_data([a[1:]], 1, [out])
    with pytest.raises(RuntimeError, match="contiguous"):
        D.reduce_data([a], 1, [torch.zeros(2 * 4097, dtype=torch.float32, device=DEV)[::2]])
    with pytest.raises(RuntimeError, match="out_status must have 1 entries"):
        D.reduce_data([a], 1, [out], None, None, torch.zeros(2, dtype=torch.uint8, device=DEV))
    a64 = torch.from_numpy(O.float_compress(np.arange(100, dtype=np.uint64), 4, 10).copy()).to(DEV)
    with pytest.raises(RuntimeError, match="float64 one"):
        D.reduce_data([a64], 1, [out])
    assert not bool(out.any())


def test_graph_capture_replay(C):
    """One K = 3 reduce captured in a hipGraph and replayed twice, new archive
    bytes copied into the same buffers in between."""
    ws = C.Workspace(16 << 20)
    n = 40000
    rounds = [[source(2, n, 600 + 3 * r + k) for k in range(3)] for r in range(3)]
    room = max(a.size for row in rounds for _, a in row)
    slots = [torch.zeros(room, dtype=torch.uint8, device=DEV) for _ in range(3)]
    init = A.random_acc(2, 2, n, seed=4)
    init_d = init.to(DEV)
    out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)

    def load(r):
        for slot, (_, a) in zip(slots, rounds[r]):
            slot[: a.size].copy_(torch.from_numpy(a.copy()))

    load(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.float_reduce([[s] for s in slots], [out], inits=[init_d], ft=2, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        ok, sz = C.float_reduce([[s] for s in slots], [out], inits=[init_d], ft=2, ws=ws)
    for r in (1, 2):
        load(r)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [n]
        want = R.model([x for x, _ in rounds[r]], init=init, out_dtype=torch.bfloat16)
        assert A.same_bits(out.cpu(), want), f"replay {r}: " + A.mismatch_report(out.cpu(), want)


def test_several_chunks_per_workgroup(C):
    """256 x 524,288 bf16 words (the c2 shape) at K = 3: every workgroup takes
    several chunks, so the double-buffered loads cross a chunk boundary.  Four
    distinct members repeat through the batch; every row is compared."""
    nb, n, kinds = 256, 524288, 4
    ws = C.Workspace(16 << 20)
    rows = [[source(2, n, 700 + 3 * j + k) for k in range(3)] for j in range(kinds)]
    arch = [[torch.from_numpy(a.copy()).to(DEV) for _, a in row] for row in rows]
    init = [A.random_acc(2, 1, n, seed=720 + j) for j in range(kinds)]
    want = torch.stack([R.model([x for x, _ in rows[j]], init=init[j], out_dtype=torch.bfloat16)
                        for j in range(kinds)])
    assert not bool(torch.isnan(want).any())
    buf = torch.stack(init).to(DEV).repeat(nb // kinds, 1).contiguous()  # row i holds member i % kinds
    outs = [buf[i] for i in range(nb)]
    ok, sz = C.float_reduce([[arch[i % kinds][k] for i in range(nb)] for k in range(3)], outs, inits=outs, ft=2, ws=ws)
    assert bool((ok == 1).all()) and bool((sz == n).all())
    got = A.bits(buf).view(nb // kinds, kinds, n)
    assert bool((got == A.bits(want).to(DEV)[None]).all())


# ----------------------------------------------------------- collectives ----

class LoopOnly:
    """A codec without `reduce`: reduce_archives keeps the per-peer loop."""

    def __init__(self, codec):
        self.compress, self.decompress, self.accumulate, self.info = (codec.compress, codec.decompress,
                                                                      codec.accumulate, codec.info)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_reduce_archives_fused_equals_model_and_loop(pg, C, dtype):
    """own + 7 GPU-compressed peers, n = 70,001: the model's bits, and the
    per-peer loop's; with profiling on, the fused call launches the "reduce"
    family and no "decode_accumulate"."""
    from dietgpu_fork_amd import dist as D

    ft = FT_OF[dtype]
    xs = R.sources(ft, 8, 70001, seed=800)
    own, peers = xs[0], xs[1:]
    codec = D.GpuFloatCodec()
    comp, sizes = codec.compress([p.to(DEV) for p in peers])
    archives = [comp[i, : int(sizes[i])] for i in range(7)]
    C.profile(True)
    try:
        C.profile_reset()
        got = D.reduce_archives(own.to(DEV), archives, codec)
        torch.cuda.synchronize()
        assert C.profile_query("reduce")[1] >= 1 and C.profile_query("decode_accumulate")[1] == 0
        C.profile_reset()
        loop = D.reduce_archives(own.to(DEV), archives, LoopOnly(codec))
        torch.cuda.synchronize()
        assert C.profile_query("reduce")[1] == 0 and C.profile_query("decode_accumulate")[1] == 7
    finally:
        C.profile(False)
    want = R.model(peers, init=own, out_dtype=dtype)
    assert not bool(torch.isnan(want).any())
    assert got.dtype == dtype and A.same_bits(got.cpu(), want), A.mismatch_report(got.cpu(), want)
    assert torch.equal(A.bits(got), A.bits(loop))
    # own=None: the first archive stands in for it
    got = D.reduce_archives(None, archives, codec)
    want = R.model(peers, out_dtype=dtype)
    assert got.dtype == dtype and A.same_bits(got.cpu(), want), A.mismatch_report(got.cpu(), want)
    assert torch.equal(A.bits(got), A.bits(D.reduce_archives(None, archives, LoopOnly(codec))))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_world_of_one_still_returns_its_input(pg, dtype):
    from dietgpu_fork_amd import dist as D

    x = A.random_acc(FT_OF[dtype], 1, 12345, seed=7)
    x[::5] = -0.0
    x = x.to(DEV)
    y = D.reduce_scatter_compressed([x])
    assert y.dtype == dtype and torch.equal(A.bits(y), A.bits(x))
    z = D.all_reduce_compressed(x.view(3, 4115))
    assert z.shape == (3, 4115) and torch.equal(A.bits(z.view(-1)), A.bits(x))
