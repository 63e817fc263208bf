"""GPU tests of the pooled row gather with a mode, weights and a padding index
(DESIGN.md 5.2n): codec.gather_rows_pool, torch.ops.dietgpu.gather_rows_pool
and the C ABI's dietgpu_float_gather_rows_pool over k_gatherPool.  The
reference is a plain fp64 computation on the table's values; the tolerances are
the fmaf-chain bounds of the issue, n_b * 2^-23 * sum |w| |x| (mean: n_b + 2,
divided by n_b), plus half an ulp of the result for a 16-bit out.  Max, the
integer tables and the bit comparisons are exact.  Destinations are
test_gpu_gather_sum's: a 0xA5-filled buffer with canaries, compared whole."""
import numpy as np
import pytest
import torch

from tests.gpu_harness import C, DEV, N, Cache, workspace_fixture  # noqa: F401
from tests.test_gpu_gather_sum import Dest, oracle_archive, tensors
from tests.util import FT_NAME, NP_WORD, TORCH_FLOAT

pytestmark = pytest.mark.gpu

# (R, row_words): rows straddle 4096-word blocks, one partial tile; three
# tiles, the last 44 columns wide, and a tile that spans two blocks
SHAPES = [(70, 96), (40, 300)]
FORMS = [(1, torch.float16), (1, torch.float32), (2, torch.bfloat16), (2, torch.float32), (3, torch.float32)]
FORM_IDS = [f"{FT_NAME[ft]}-to-{str(dt)[6:]}" for ft, dt in FORMS]
PAD = 7  # the padding row of the shared bag list
# (significand bits, least normal exponent) of a 16-bit out
PREC = {torch.float16: (11, -14), torch.bfloat16: (8, -126)}

ws = workspace_fixture(1 << 20)
_TABLES = Cache()


def bag_list(R):
    """Empty, one row, two rows (the special rows of max), 37 rows with repeats
    and both ends of the table, all padding, padding first, padding between."""
    long = np.random.default_rng(R).integers(8, R, 35).tolist()
    return [[], [5], [3, 4], [0] + long + [R - 1], [PAD] * 3, [PAD, 9, 11], [12, PAD, 3, PAD, 14]]


def flat(bags):
    return [r for b in bags for r in b], [0] + np.cumsum([len(b) for b in bags]).tolist()


def table(ft, shape, kind="normal", pb=10):
    """(words [R, rw], values as fp64, archive, archive 4 B off), made once.
    "special": row 3 holds a NaN in columns 1 and 5, -0.0 where row 4 holds
    +0.0 and a denormal above row 4's -1.0; "ints": small integers."""
    def make():
        R, rw = shape
        rng = np.random.default_rng(100 * ft + R)
        v = rng.integers(-8, 9, (R, rw)).astype(np.float32) if kind == "ints" else \
            rng.standard_normal((R, rw)).astype(np.float32)
        t = torch.from_numpy(v).to(TORCH_FLOAT[ft])
        if kind == "special":
            t[3, [1, 5]] = float("nan")
            t[3, 2], t[4, 2], t[4, 7] = -0.0, 0.0, -1.0
            ints = t.view(torch.int32 if ft == 3 else torch.int16)
            ints[3, 7] = 1  # the least denormal
            ints[3, 5] = {1: 0xfe01, 2: 0xffc1, 3: 0xffc00001}[ft] - (1 << 8 * ints.element_size())  # -NaN, payload 1
        words = t.view(torch.int32 if ft == 3 else torch.int16).numpy().view(NP_WORD[ft])
        return (words, t.double().numpy()) + oracle_archive(words.reshape(-1), ft, pb)
    return _TABLES.get((ft, shape, kind, pb), make)


def reference(x, bags, mode, w=None, pad=None):
    """fp64 -> (result [B, rw], sum |w| |x| [B, rw], n_b [B]); max by the
    compare rule of the contract, -> (result, winning row of each column)."""
    B, rw = len(bags), x.shape[1]
    out, mag, nb, who = np.zeros((B, rw)), np.zeros((B, rw)), np.zeros(B), np.zeros((B, rw), dtype=np.int64)
    at = 0
    for b, bag in enumerate(bags):
        for r in bag:
            wt = 1.0 if w is None else float(w[at])
            at += 1
            if r == pad:
                continue
            if mode == "max":
                take = (x[r] > out[b]) | np.isnan(x[r]) if nb[b] else np.ones(rw, dtype=bool)
                out[b], who[b] = np.where(take, x[r], out[b]), np.where(take, r, who[b])
            else:
                out[b] += wt * x[r]
                mag[b] += abs(wt) * np.abs(x[r])
            nb[b] += 1
        if mode == "mean" and nb[b]:
            out[b] /= nb[b]
    return (out, who, nb) if mode == "max" else (out, mag, nb)


def run(C, ws, ft, arch, rw, bags, out_dtype, bits=64, pb=10, want=None, ok=None, off=0, stride_pad=0, **kw):
    """One call into a canaried destination -> (out on the CPU, status list, dest)."""
    idx, offsets = flat(bags)
    it, ot = tensors(idx, offsets, bits)
    want = want if want is not None else torch.zeros([len(bags), rw], dtype=out_dtype)
    dest = Dest(out_dtype, want, ok if ok is not None else [1] * len(bags), off, stride_pad)
    status = torch.full([len(bags)], 7, dtype=torch.uint8, device=DEV)
    C.gather_rows_pool(arch, rw, it, ot, TORCH_FLOAT[ft], out=dest.out, out_status=status, prob_bits=pb, ws=ws, **kw)
    torch.cuda.synchronize()
    return dest.out.cpu(), status.cpu().tolist(), dest


def within(got, ref, bound, out_dtype):
    got = got.double().numpy()
    if out_dtype != torch.float32:  # half an ulp of the result
        p, emin = PREC[out_dtype]
        e = np.frexp(np.maximum(np.abs(ref), np.abs(got)))[1] - 1
        bound = bound + np.ldexp(1.0, np.maximum(e, emin) - p)
    err = np.abs(got - ref)
    assert (err <= bound).all(), f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}"


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", ["fp32-weights", "own-weights", "mean"])
def test_weighted_sum_and_mean(C, ws, form, shape, kind):
    (ft, out_dtype), (R, rw) = form, shape
    _, x, a16, _ = table(ft, shape)
    bags = bag_list(R)
    w, kw = None, dict(mode="mean")
    if kind != "mean":
        w = torch.from_numpy(np.random.default_rng(5).standard_normal(len(flat(bags)[0])).astype(np.float32))
        w = w.to(TORCH_FLOAT[ft] if kind == "own-weights" else torch.float32)
        kw = dict(per_sample_weights=w.to(DEV))
    ref, mag, nb = reference(x, bags, "sum" if w is not None else "mean", None if w is None else w.double().numpy(), PAD)
    got, status, _ = run(C, ws, ft, a16, rw, bags, out_dtype, padding_idx=PAD, **kw)
    assert status == [1] * len(bags)
    steps = nb if w is not None else (nb + 2) / np.maximum(nb, 1)  # the issue's bounds
    within(got, ref, steps[:, None] * 2.0 ** -23 * mag, out_dtype)
    assert not got[0].any() and not got[4].any() and not torch.signbit(got[[0, 4]]).any()  # +0.0


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_max_is_the_compare_rule_bit_for_bit(C, ws, form, shape):
    """A NaN anywhere in the bag wins, -0.0 before +0.0 stays, the denormal
    beats -1.0; a 16-bit out is the table's word."""
    (ft, out_dtype), (R, rw) = form, shape
    words, x, a16, _ = table(ft, shape, "special")
    bags = bag_list(R)
    ref, who, nb = reference(x, bags, "max", None, PAD)
    won = torch.from_numpy(np.take_along_axis(words, who, 0).view(words.dtype.str.replace("u", "i")).copy())
    want = won.view(TORCH_FLOAT[ft]).to(out_dtype)  # exact: the same type, or a widening
    want[torch.from_numpy(nb == 0)] = 0.0
    assert np.isnan(ref[2, [1, 5]]).all() and np.isnan(ref[6, [1, 5]]).all() and np.signbit(ref[2, 2])
    assert ref[2, 7] == x[3, 7] > 0
    got, status, dest = run(C, ws, ft, a16, rw, bags, out_dtype, want=want, mode="max", padding_idx=PAD)
    dest.check(torch.tensor(status), "max")
    ints = torch.int32 if out_dtype == torch.float32 else torch.int16  # (check() takes any NaN for a NaN)
    assert torch.equal(got.view(ints)[[2, 6]][:, [1, 5]], want.view(ints)[[2, 6]][:, [1, 5]]), "NaN sign and payload"


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("mode", ["sum", "weighted", "mean", "max"])
def test_small_integers_pool_exactly(C, ws, form, mode):
    (ft, out_dtype), (R, rw) = form, SHAPES[1]
    _, x, a16, _ = table(ft, SHAPES[1], "ints")
    bags = bag_list(R)
    w = torch.from_numpy(np.random.default_rng(6).integers(-4, 5, len(flat(bags)[0])).astype(np.float32))
    weighted = mode == "weighted"
    kind = "sum" if weighted else mode
    ref = reference(x, bags, kind, w.numpy() if weighted else None, PAD)[0]
    want = torch.from_numpy(ref.astype(np.float32)).to(out_dtype)  # integers, or one rounding of an exact quotient
    kw = dict(per_sample_weights=w.to(DEV)) if weighted else {}
    got, status, _ = run(C, ws, ft, a16, rw, bags, out_dtype, mode=kind, padding_idx=PAD, **kw)
    # (by value: a first product of -1 * 0 is -0.0, the integer 0 all the same)
    assert status == [1] * len(bags) and bool((got.double() == want.double()).all())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_the_plain_sum_has_gather_rows_sum_bits(C, ws, form):
    """Without weights and padding; with weights of 1.0; and a bag's bits stay
    when the other bags are permuted."""
    (ft, out_dtype), (R, rw) = form, SHAPES[1]
    a16 = table(ft, SHAPES[1])[2]
    bags = bag_list(R)
    idx, offsets = flat(bags)
    it, ot = tensors(idx, offsets, 64)
    want = C.gather_rows_sum(a16, rw, it, ot, TORCH_FLOAT[ft], out_dtype=out_dtype, ws=ws)[0].cpu()
    _, status, dest = run(C, ws, ft, a16, rw, bags, out_dtype, want=want)
    dest.check(torch.tensor(status), "plain sum")
    for wdt in {torch.float32, TORCH_FLOAT[ft]}:
        ones = torch.ones([len(idx)], dtype=wdt, device=DEV)
        _, status, dest = run(C, ws, ft, a16, rw, bags, out_dtype, want=want, per_sample_weights=ones)
        dest.check(torch.tensor(status), "weights of 1.0")
    order = [3, 6, 0, 5, 2, 4, 1]
    _, status, dest = run(C, ws, ft, a16, rw, [bags[k] for k in order], out_dtype, want=want[order])
    dest.check(torch.tensor(status), "permuted bags")


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_padding_and_failure(C, ws, mode):
    """A padding index outside the table fails no bag; another index outside
    it fails its bag alone, whose row keeps its canary.  A negative
    padding_idx names the row its positive twin names."""
    (R, rw), ft = SHAPES[0], 2
    _, x, a16, _ = table(ft, SHAPES[0])
    far = R + 5
    bags = [[far, 2, far], [far], [1, R, 2], [R - 1, far]]
    want = C.gather_rows_pool(a16, rw, *tensors(*flat([[2], [], [], [R - 1]]), 64), torch.bfloat16, mode=mode,
                              ws=ws)[0].cpu()
    _, status, dest = run(C, ws, ft, a16, rw, bags, torch.bfloat16, want=want, ok=[1, 1, 0, 1], mode=mode,
                          padding_idx=far)
    dest.check(torch.tensor(status), "padding outside the table")
    bags = bag_list(R)
    want = run(C, ws, ft, a16, rw, bags, torch.bfloat16, mode=mode, padding_idx=PAD)[0]
    _, status, dest = run(C, ws, ft, a16, rw, bags, torch.bfloat16, want=want, mode=mode, padding_idx=PAD - R,
                          num_rows=R)
    dest.check(torch.tensor(status), "negative padding_idx")


@pytest.mark.parametrize("case", ["int32", "shifted-archive", "pb9", "pb11", "wide-stride"])
def test_one_case_each(C, ws, case):
    (R, rw), ft = SHAPES[1], 1
    pb = {"pb9": 9, "pb11": 11}.get(case, 10)
    _, x, a16, a4 = table(ft, SHAPES[1], pb=pb)
    bags = bag_list(R)
    w = torch.from_numpy(np.random.default_rng(7).standard_normal(len(flat(bags)[0])).astype(np.float32))
    ref, mag, nb = reference(x, bags, "sum", w.double().numpy(), PAD)
    got, status, dest = run(C, ws, ft, a4 if case == "shifted-archive" else a16, rw, bags, torch.float32,
                            bits=32 if case == "int32" else 64, pb=pb, off=1, stride_pad=5 if case == "wide-stride" else 0,
                            per_sample_weights=w.to(DEV), padding_idx=PAD)
    assert status == [1] * len(bags)
    within(got, ref, nb[:, None] * 2.0 ** -23 * mag, torch.float32)
    dest.rows(dest.want, len(bags), rw).copy_(dest.rows(dest.buf, len(bags), rw))
    dest.check(None, "canaries and gaps")  # nothing but the rows was written


@pytest.mark.parametrize("form", [FORMS[2], FORMS[4]], ids=[FORM_IDS[2], FORM_IDS[4]])
def test_operator_and_c_abi_give_the_wrapper_bits(C, N, ws, form):
    (ft, out_dtype), (R, rw) = form, SHAPES[0]
    a16 = table(ft, SHAPES[0])[2]
    bags = bag_list(R) + [[1, R, 2]]
    ok = [1] * 7 + [0]
    it, ot = tensors(*flat(bags), 64)
    w = torch.from_numpy(np.random.default_rng(8).standard_normal(it.numel()).astype(np.float32)).to(DEV)
    for mode, wt in (("sum", w), ("mean", None), ("max", None)):
        want = run(C, ws, ft, a16, rw, bags, out_dtype, ok=ok, mode=mode, per_sample_weights=wt, padding_idx=PAD)[0]
        dest = Dest(out_dtype, want, ok, 1, 3)
        status = torch.full([len(bags)], 7, dtype=torch.uint8, device=DEV)
        used = torch.ops.dietgpu.gather_rows_pool(a16, rw, it, ot, dest.out, mode, wt, PAD - R, R, None, status)
        assert isinstance(used, int)
        dest.check(status, f"operator {mode}")
        dest = Dest(out_dtype, want, ok, 1, 3)
        rc = N.lib().dietgpu_float_gather_rows_pool(
            ws.h, ft, 10, a16.data_ptr(), rw, len(bags), it.numel(), it.data_ptr(), ot.data_ptr(), 1,
            C.POOL_MODE[mode], wt.data_ptr() if wt is not None else None, 3 if wt is not None else 0, PAD,
            dest.out.data_ptr(), int(out_dtype == torch.float32), dest.stride, status.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        assert rc == N.DIETGPU_OK, N.lib().dietgpu_last_error()
        dest.check(status, f"C ABI {mode}")
    with pytest.raises(ValueError, match="constant stride of at least row_words"):  # (behind the wrapper's device check)
        C.gather_rows_pool(a16, rw, it, ot, TORCH_FLOAT[ft], out=dest.out.as_strided((len(bags), rw), (rw - 1, 1)), ws=ws)


def test_graph_capture_replay(C):
    """Captured once, replayed on new indices, offsets and weights: several
    replays against the eager result."""
    (R, rw), B, m = SHAPES[1], 9, 60
    a16 = table(2, SHAPES[1])[2]
    ws = C.Workspace(1 << 20)
    idx = torch.zeros([m], dtype=torch.int64, device=DEV)
    offsets = torch.zeros([B + 1], dtype=torch.int64, device=DEV)
    w = torch.zeros([m], dtype=torch.float32, device=DEV)
    out = torch.empty([B, rw], dtype=torch.float32, device=DEV)
    ok = torch.empty([B], dtype=torch.uint8, device=DEV)

    def call(o, s):
        C.gather_rows_pool(a16, rw, idx, offsets, torch.bfloat16, per_sample_weights=w, padding_idx=PAD, out=o,
                           out_status=s, ws=ws)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        call(out, ok)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        call(out, ok)
    for rep in range(3):
        rng = np.random.default_rng(rep)
        rows = rng.integers(0, R, m)
        rows[rep] = R + rep  # one failing bag
        idx.copy_(torch.from_numpy(rows))
        offsets.copy_(torch.tensor([0] + np.sort(rng.integers(0, m + 1, B - 1)).tolist() + [m]))
        w.copy_(torch.from_numpy(rng.standard_normal(m).astype(np.float32)))
        eager, eager_ok = torch.full_like(out, 9.0), torch.full_like(ok, 7)
        call(eager, eager_ok)
        out.fill_(9.0)
        ok.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert 0 in ok.cpu().tolist() and torch.equal(ok, eager_ok), f"replay {rep}"
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), f"replay {rep}"
