"""GPU tests of the three compressed matmuls on inputs
whose result is known to the bit: codec.matmul_rows, codec.matmul_tile and
codec.matmul_grouped on the exact-sum tables of tests/matmul_cases.py (out is the
int64 product, so every weight word counts), on tables that are a prefix of
their archive, on special and non-finite values, and with the main kernels'
grid capped (codec.set_matmul_grid) so that a workgroup takes several task
groups.  Archives come from the CPU oracle.  Every call's out lies inside
canary rows and columns, and its status must be 1."""
from itertools import accumulate

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import matmul_cases as MC
from tests.gpu_harness import C, DEV, Cache, workspace_fixture  # noqa: F401
from tests.test_gpu_matmul_rows import FILL, acts, table
from tests.util import FT_NAME, TORCH_FLOAT

pytestmark = pytest.mark.gpu

ROUTINGS = [[5, 0, 17, 1], [70, 0, 64, 1]]
ROWS_M, TILE_M = (1, 3, 4), (1, 17, 64)
FTS = {"rows": (1, 2, 3), "tile": (1, 2), "grouped": (1, 2)}  # the types an entry takes
ENTRIES = ("rows", "tile", "grouped")

ws = workspace_fixture(16 << 20)
_MADE = Cache()


def ft_ids(fts):
    return [FT_NAME[ft] for ft in fts]


def archives(W, ft, pb=10):
    """(the oracle's archive of table W 16 B-aligned, the same 4 B off)"""
    a = torch.from_numpy(np.asarray(O.float_compress(MC.words_of(W, ft), ft, pb, False), dtype=np.uint8).copy()).to(DEV)
    room = torch.zeros([a.numel() + 32], dtype=torch.uint8, device=DEV)
    room[4: 4 + a.numel()] = a
    assert a.data_ptr() % 16 == 0 and room.data_ptr() % 16 == 0
    return a, room[4: 4 + a.numel()]


def exact(ft, rw, R, const=False, seed=0):
    """(a, e, W, archive, archive 4 B off) of an exact-sum table, made once"""
    def make():
        a, e, W = MC.exact_table(ft, rw, R, seed, *((0, 0) if const else (None, None)))
        return (a, e, W) + archives(W, ft)
    return _MADE.get(("exact", ft, rw, R, const, seed), make)


def exact_x(ft, M, rw, e):
    """(b, x on the device) of M rows, made once"""
    def make():
        b, x = MC.exact_acts(ft, M, rw, e)
        return b, x.to(DEV)
    return _MADE.get(("x", ft, M, rw, int(e.min()), int(e.max())), make)


def call(C, ws, entry, arch, rw, x, R, ft, counts=None):
    """out [T, R] (fp32, a copy) of one entry: arch an archive, or for "grouped"
    the experts' archives with `counts` rows of x each.  out lies at a stride of
    R + 3 inside a buffer of FILL bytes, one row above and below it: all of
    that must be untouched, and every status 1."""
    T, dt = x.size(0), TORCH_FLOAT[ft]
    buf = torch.full([T + 2, 4 * (R + 3)], FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    out = buf[1:T + 1, :R]
    if entry == "rows":
        ok = C.matmul_rows(arch, rw, x, dt, out=out, ws=ws)[1]
    elif entry == "tile":
        ok = C.matmul_tile(arch, rw, x, dt, out=out, ws=ws)[1]
    else:
        assert sum(counts) == T
        offs = torch.tensor([0] + list(accumulate(counts)), dtype=torch.int64, device=DEV)
        ok = C.matmul_grouped(C.archive_ptrs(arch), rw, x, offs, dt, out=out, ws=ws)[1]
    assert ok.tolist() == [1] * ok.numel(), (entry, ok.tolist())
    edge = torch.cat([buf[0], buf[-1], buf[:, R:].reshape(-1)])
    assert bool((edge.view(torch.uint8) == FILL).all()), entry
    return out.clone()


def same_bits(got, want):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.cpu().contiguous().view(torch.int32))


def grouped_want(b, tabs, counts, R=None):
    """the int64 products of a grouped call: expert e's rows against its table"""
    lo, parts = 0, []
    for (a, *_), cnt in zip(tabs, counts):
        parts.append(MC.exact_product(b[lo:lo + cnt], a[:R]) if cnt else torch.empty([0, len(a[:R])]))
        lo += cnt
    return torch.cat(parts)


# ------------------------------------------------------------ every word counts ----

WORD_CASES = [(rw, R, const) for rw, R in MC.WORD_SHAPES for const in (False, True)]
WORD_IDS = [f"{rw}x{R}-{'const' if const else 'wide'}" for rw, R, const in WORD_CASES]


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("rw,R,const", WORD_CASES, ids=WORD_IDS)
def test_rows_every_word_counts(C, ws, rw, R, const, ft):
    a, e, _, a16, a4 = exact(ft, rw, R, const)
    assert MC.A_MAX * MC.b_max(rw) * rw < 1 << 24
    b, x = exact_x(ft, max(ROWS_M), rw, e)
    for arch in (a16, a4):
        for M in ROWS_M:
            assert same_bits(call(C, ws, "rows", arch, rw, x[:M], R, ft), MC.exact_product(b[:M], a)), M


@pytest.mark.parametrize("ft", FTS["tile"], ids=ft_ids(FTS["tile"]))
@pytest.mark.parametrize("rw,R,const", WORD_CASES, ids=WORD_IDS)
def test_tile_every_word_counts(C, ws, rw, R, const, ft):
    a, e, _, a16, a4 = exact(ft, rw, R, const)
    assert MC.A_MAX * MC.b_max(rw) * rw < 1 << 24
    b, x = exact_x(ft, max(TILE_M), rw, e)
    for arch in (a16, a4):
        for M in TILE_M:
            assert same_bits(call(C, ws, "tile", arch, rw, x[:M], R, ft), MC.exact_product(b[:M], a)), M


@pytest.mark.parametrize("ft", FTS["grouped"], ids=ft_ids(FTS["grouped"]))
@pytest.mark.parametrize("rw,R,const", WORD_CASES, ids=WORD_IDS)
def test_grouped_every_word_counts_and_the_entries_agree(C, ws, rw, R, const, ft):
    tabs = [exact(ft, rw, R, const, seed=s) for s in range(4)]
    assert MC.A_MAX * MC.b_max(rw) * rw < 1 << 24
    for counts in ROUTINGS:
        b, x = exact_x(ft, sum(counts), rw, tabs[0][1])
        want = grouped_want(b, tabs, counts)
        for off in (None, 2):  # expert 2's archive 4 B off 16 B
            arch = [t[4] if s == off else t[3] for s, t in enumerate(tabs)]
            got = call(C, ws, "grouped", arch, rw, x, R, ft, counts)
            assert same_bits(got, want), (counts, off)
        # the three entries give one another's bits
        assert same_bits(call(C, ws, "tile", tabs[0][3], rw, x[:5], R, ft), got[:5])
        assert same_bits(call(C, ws, "rows", tabs[0][3], rw, x[:4], R, ft), got[:4])


# ------------------------------------------------------------------ new periods ----

@pytest.mark.parametrize("ft", FTS["tile"], ids=ft_ids(FTS["tile"]))
@pytest.mark.parametrize("rw,R", MC.PERIOD_SHAPES)
def test_periods_5_7_and_43(C, ws, rw, R, ft):
    tabs = [exact(ft, rw, R, seed=s) for s in range(4)]
    a, e, _, a16, a4 = tabs[0]
    assert MC.A_MAX * MC.b_max(rw) * rw < 1 << 24
    b, x = exact_x(ft, max(TILE_M), rw, e)
    for M in TILE_M:
        assert same_bits(call(C, ws, "tile", a16, rw, x[:M], R, ft), MC.exact_product(b[:M], a)), M
    assert same_bits(call(C, ws, "tile", a4, rw, x[:17], R, ft), MC.exact_product(b[:17], a))
    counts = ROUTINGS[0]
    got = call(C, ws, "grouped", [t[3] for t in tabs], rw, x[:sum(counts)], R, ft, counts)
    assert same_bits(got, grouped_want(b, tabs, counts))
    if (rw, R) == MC.PERIOD_SHAPES[0]:
        for M in ROWS_M:
            assert same_bits(call(C, ws, "rows", a16, rw, x[:M], R, ft), MC.exact_product(b[:M], a)), M


# --------------------------------------------------------------- prefix tables ----

PREFIX_IDS = [f"{rw}x{R}-first{Rp}" for rw, R, Rp in MC.PREFIXES]


def prefix_calls(C, ws, ft, rw, Rp, archs, x):
    """[(entry, out)] of every entry that takes the type, on the first Rp rows;
    the grouped call routes x over four experts"""
    counts = [5, 0, x.size(0) - 6, 1]
    outs = [("rows", call(C, ws, "rows", archs[0], rw, x[:4], Rp, ft))]
    if ft in FTS["tile"]:
        outs.append(("tile", call(C, ws, "tile", archs[0], rw, x, Rp, ft)))
        outs.append(("grouped", call(C, ws, "grouped", archs, rw, x, Rp, ft, counts)))
    return outs, counts


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("rw,R,Rp", MC.PREFIXES, ids=PREFIX_IDS)
def test_prefix_of_an_exact_table(C, ws, rw, R, Rp, ft):
    """out is the int64 product of the first R' rows; the canaries right of R' stay (call())."""
    assert Rp < R
    tabs = [exact(ft, rw, R, seed=s) for s in range(4 if ft in FTS["grouped"] else 1)]
    b, x = exact_x(ft, 23, rw, tabs[0][1])
    outs, counts = prefix_calls(C, ws, ft, rw, Rp, [t[3] for t in tabs], x)
    for entry, got in outs:
        want = grouped_want(b, tabs, counts, Rp) if entry == "grouped" else MC.exact_product(b, tabs[0][0][:Rp])
        assert same_bits(got, want[:got.size(0)]), entry
    if ft in FTS["tile"]:  # ... and from the archive 4 B off
        assert same_bits(call(C, ws, "tile", tabs[0][4], rw, x, Rp, ft), outs[1][1])
    assert same_bits(call(C, ws, "rows", tabs[0][4], rw, x[:4], Rp, ft), outs[0][1])


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("rw,R,Rp", MC.PREFIXES, ids=PREFIX_IDS)
def test_prefix_of_a_normal_table(C, ws, rw, R, Rp, ft):
    """N(0, 1) weights: out is [:, :R'] of the full call, bit for bit."""
    archs = [table(ft, rw, R, seed=s)[1] for s in range(4 if ft in FTS["grouped"] else 1)]
    x = acts(ft, 23, rw).to(DEV)
    part, _ = prefix_calls(C, ws, ft, rw, Rp, archs, x)
    full, _ = prefix_calls(C, ws, ft, rw, R, archs, x)
    for (entry, got), (_, whole) in zip(part, full):
        assert same_bits(got, whole[:, :Rp].contiguous()), entry


# -------------------------------------------------------------- special values ----

def special(ft):
    def make():
        W = MC.special_table(ft)
        return (W,) + archives(W, ft)
    return _MADE.get(("special", ft), make)


def special_runs(C, ws, entry, ft):
    """(got, want) fp32 on the CPU of the two special-value runs of an entry:
    unit rows on the special columns (want: W[r, k] widened) and denormal
    activations on the mirror columns (want: the exact product, an fp32 number)"""
    rw, R = MC.SPECIAL_SHAPE
    W, a16, _ = special(ft)
    runs = []
    for x in (MC.unit_acts(ft, MC.SPECIAL_KS, rw), MC.unit_acts(ft, MC.MIRROR_KS, rw, MC.mirror_scales(ft))):
        if entry == "grouped":  # two experts on one table: the rows split between them
            n = x.size(0)
            got = call(C, ws, entry, [a16, a16], rw, x.to(DEV), R, ft, [n // 2, n - n // 2])
        else:
            got = call(C, ws, entry, a16, rw, x.to(DEV), R, ft)
        want = (x.double() @ W.double().T).float()
        assert torch.equal(want.double(), x.double() @ W.double().T)
        runs.append((got.cpu(), want))
    return runs


def report(entry, ft, name, got, want):
    """print what became of the outputs whose exact value is an fp32 denormal, or comes from a denormal operand"""
    tiny = float(torch.finfo(torch.float32).tiny)
    den = (want != 0) & (want.abs() < tiny)
    lost = den & (got == 0)
    print(f"{entry} {FT_NAME[ft]} {name}: {int(den.sum())} denormal results wanted, {int(lost.sum())} came out zero "
          f"({int((lost & torch.signbit(got)).sum())} of them -0.0); "
          f"{int((got.view(torch.int32) != want.view(torch.int32)).sum())} of {got.numel()} outputs differ in bits")


SPECIAL_CASES = [(entry, ft) for entry in ENTRIES for ft in FTS[entry]]


@pytest.mark.parametrize("entry,ft", SPECIAL_CASES, ids=[f"{entry}-{FT_NAME[ft]}" for entry, ft in SPECIAL_CASES])
def test_denormals_zeros_and_the_largest_finite_are_kept(C, ws, entry, ft):
    """x[m] = e_k on the special columns: out[m, r] is W[r, k] widened -- denormal,
    +-max or (numerically) zero; denormal activations against 2^10 and 1: the exact
    product, a normal fp32 number or a denormal one.  matmul_rows keeps them by its
    fmaf contract; the matrix pipe of gfx950 was observed to keep denormal operands
    and denormal results too, and this holds it to that."""
    (got, want), (got_m, want_m) = special_runs(C, ws, entry, ft)
    report(entry, ft, "special columns", got, want)
    report(entry, ft, "denormal activations", got_m, want_m)
    nz = want != 0
    assert torch.equal(got[nz].view(torch.int32), want[nz].view(torch.int32))
    assert bool((got[~nz] == 0).all())
    assert torch.equal(got_m.view(torch.int32), want_m.view(torch.int32))


# ------------------------------------------------------------ non-finite values ----

POISON_M = 19
INF = float("inf")


def clean_tables(ft):
    return [table(ft, 768, 50, seed=s) for s in range(4 if ft in FTS["grouped"] else 1)]


def poison_calls(C, ws, ft, Rp, one, four, x):
    """[(entry, out [19, Rp], the expert of every row)]: matmul_rows (five passes)
    and matmul_tile on archive `one`, matmul_grouped on the experts `four`"""
    counts = [5, 0, 13, 1]
    outs = [("rows", call(C, ws, "rows", one, 768, x, Rp, ft), [0] * POISON_M)]
    if ft in FTS["tile"]:
        outs.append(("tile", call(C, ws, "tile", one, 768, x, Rp, ft), [0] * POISON_M))
        owner = [s for s, cnt in enumerate(counts) for _ in range(cnt)]
        outs.append(("grouped", call(C, ws, "grouped", four, 768, x, Rp, ft, counts), owner))
    return outs


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("Rp", [50, 7], ids=["whole", "first7"])
def test_nonfinite_activations_stay_in_their_rows(C, ws, Rp, ft):
    """x[3, k0] = +Inf: out[3, r] = sign(W[r, k0]) * Inf, also where zero segments
    past a prefix table meet the Inf before the live ones; x[18, k1] = NaN: out[18]
    is NaN; every other row has the bits of the clean call."""
    tabs = clean_tables(ft)
    Ws, archs = [t[0] for t in tabs], [t[1] for t in tabs]
    k0 = next(k for k in range(40, 768) if all(bool((W[:, k] != 0).all()) for W in Ws))
    x = acts(ft, POISON_M, 768)
    bad = x.clone()
    bad[3, k0], bad[18, 701] = INF, float("nan")
    clean = poison_calls(C, ws, ft, Rp, archs[0], archs, x.to(DEV))
    for (entry, got, owner), (_, ref, _) in zip(poison_calls(C, ws, ft, Rp, archs[0], archs, bad.to(DEV)), clean):
        got, ref = got.cpu(), ref.cpu()
        assert bool(torch.isfinite(ref).all())
        assert torch.equal(got[3], torch.sign(Ws[owner[3]][:Rp, k0].float()) * INF), entry
        assert bool(torch.isnan(got[18]).all()), entry
        keep = [m for m in range(POISON_M) if m not in (3, 18)]
        assert same_bits(got[keep], ref[keep]), entry


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("Rp", [50, 7], ids=["whole", "first7"])
def test_nonfinite_weights_stay_in_their_columns(C, ws, Rp, ft):
    """W[5, 100] = +Inf (row 5 straddles blocks 0 and 1) and W[6, 700] = NaN in a
    re-compressed archive: column 5 of out is sign(x[m, 100]) * Inf, column 6 NaN,
    every other column has the bits of the clean table's call; in the grouped call
    expert 2 alone is poisoned, and the others' rows keep their bits."""
    tabs = clean_tables(ft)
    x = acts(ft, POISON_M, 768)
    assert bool((x != 0).all())

    def make():
        W = tabs[0][0].clone()
        W[5, 100], W[6, 700] = INF, float("nan")
        return archives(W, ft)[0]
    poisoned = _MADE.get(("poisoned", ft), make)
    archs = [t[1] for t in tabs]
    four = lambda third: archs[:2] + [third] + archs[3:]  # noqa: E731  (expert 2 holds table 0, clean or poisoned)
    clean = poison_calls(C, ws, ft, Rp, archs[0], four(archs[0]), x.to(DEV))
    hit = poison_calls(C, ws, ft, Rp, poisoned, four(poisoned), x.to(DEV))
    for (entry, got, owner), (_, ref, _) in zip(hit, clean):
        got, ref = got.cpu(), ref.cpu()
        rows = [m for m in range(POISON_M) if entry != "grouped" or owner[m] == 2]
        rest = [m for m in range(POISON_M) if m not in rows]
        assert torch.equal(got[rows, 5], torch.sign(x[rows, 100].float()) * INF), entry
        assert bool(torch.isnan(got[rows, 6]).all()), entry
        cols = [r for r in range(Rp) if r not in (5, 6)]
        assert same_bits(got[rows][:, cols], ref[rows][:, cols]), entry
        assert same_bits(got[rest], ref[rest]), entry


# --------------------------------------------------------------------- grid caps ----

CAP_IDS = [f"{rw}x{R}-first{Rp}" for rw, R, Rp in MC.CAP_SHAPES]


@pytest.mark.parametrize("ft", FTS["rows"], ids=ft_ids(FTS["rows"]))
@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("rw,R,Rp", MC.CAP_SHAPES, ids=CAP_IDS)
def test_a_workgroup_takes_several_task_groups(C, ws, rw, R, Rp, kind, ft):
    """1, 2 and 3 workgroups for k_matmulRows (M = 4) and k_matmulTile (M = 17, 64):
    the bits of the uncapped call, and on the exact table the int64 product."""
    if kind == "exact":
        a, e, _, arch, _ = exact(ft, rw, R)
        b, x = exact_x(ft, 64, rw, e)
    else:
        arch, x = table(ft, rw, R)[1], acts(ft, 64, rw).to(DEV)
    runs = [("rows", 4)] + ([("tile", 17), ("tile", 64)] if ft in FTS["tile"] else [])
    free = [call(C, ws, entry, arch, rw, x[:M], Rp, ft) for entry, M in runs]
    try:
        for cap in (1, 2, 3):
            C.set_matmul_grid(cap)
            for (entry, M), want in zip(runs, free):
                assert same_bits(call(C, ws, entry, arch, rw, x[:M], Rp, ft), want), (cap, entry, M)
    finally:
        C.set_matmul_grid(0)
    if kind == "exact":
        for (entry, M), got in zip(runs, free):
            assert same_bits(got, MC.exact_product(b[:M], a[:Rp])), (entry, M)
