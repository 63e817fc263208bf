"""GPU tests of the pooled row gather: codec.gather_rows_sum,
torch.ops.dietgpu.gather_rows_sum and the C ABI's dietgpu_float_gather_rows_sum
over k_gatherSum.  The expected rows come from the sequential fp32 model of
tests/gather_sum_cases.py and are compared bit for bit wherever the model is
not NaN, and as NaN where it is.  Archives come from the CPU oracle.  Every
destination lies inside a 0xA5-filled buffer with 16 canary words on each
side; the whole buffer is compared, so a stray write, a write into the gap of
a wider stride or any write to a failing bag's row fails the test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gather_cases as G
from tests import gather_sum_cases as S
from tests.gpu_harness import C, DEV, N, Cache, compress_one, retyped, workspace_fixture  # noqa: F401
from tests.util import FT_NAME, NP_WORD, TORCH_FLOAT

pytestmark = pytest.mark.gpu

# (archive float type, output dtype)
FORMS = [(1, torch.float16), (1, torch.float32), (2, torch.bfloat16), (2, torch.float32), (3, torch.float32)]
FORM_IDS = [f"{FT_NAME[ft]}-to-{str(dt)[6:]}" for ft, dt in FORMS]
CANARY = 16  # words on each side of the destination
FILL = 0xA5  # byte pattern of canaries, gaps and untouched rows
IDX_T = {32: torch.int32, 64: torch.int64}
INT_OF = {2: torch.int16, 4: torch.int32}

ws = workspace_fixture(16 << 20)
_TABLES = Cache()
_MODELS = Cache()


def oracle_archive(words, ft, pb=10, checksum=False):
    """(archive 16 B-aligned, the same archive 4 bytes off) on the device."""
    a = torch.from_numpy(np.asarray(O.float_compress(words, ft, pb, checksum), dtype=np.uint8).copy())
    room = torch.zeros([a.numel() + 32], dtype=torch.uint8, device=DEV)
    assert room.data_ptr() % 16 == 0
    room[4: 4 + a.numel()] = a.to(DEV)
    a16 = a.to(DEV)
    assert a16.data_ptr() % 16 == 0
    return a16, room[4: 4 + a.numel()]


def table(ft, pb=10):
    """(the table as a CPU float tensor, archive, archive 4 B off), computed
    once per key and left unchanged."""
    def make():
        w = S.table_words(ft)
        return (S.as_ints(w).view(TORCH_FLOAT[ft]),) + oracle_archive(w, ft, pb)
    return _TABLES.get((ft, pb), make)


def raw_bags(idx, offsets, rw, n_rows):
    """-> (bags, ok) of raw index / offset lists: a bag whose offsets are out
    of order or outside [0, len(idx)], or that holds a row outside the table,
    fails (its bag is then [])."""
    bags, ok = [], []
    for lo, up in zip(offsets, offsets[1:]):
        good = 0 <= lo <= up <= len(idx) and all(0 <= r < n_rows for r in idx[lo:up])
        ok.append(int(good))
        bags.append(list(idx[lo:up]) if good else [])
    return bags, ok


class Dest:
    """B rows of rw words of out_dtype at `stride`, starting `off` words past a
    16 B boundary inside a FILL-ed buffer, 16 canary words on each side; and
    the buffer as it must look afterwards: `want` rows where ok, FILL
    elsewhere."""

    def __init__(self, out_dtype, want, ok, off=0, pad=0):
        wb = want.element_size()
        per16 = 16 // wb
        B, rw = want.shape
        self.out_dtype, self.ok = out_dtype, list(ok)
        self.stride = rw + pad
        self.start = -(-CANARY // per16) * per16 + off
        total = self.start + B * self.stride + CANARY + per16
        self.buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(INT_OF[wb])
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.rows(self.buf, B, rw).view(out_dtype)
        assert B == 0 or (self.out.data_ptr() % 16 == 0) == (off % per16 == 0)
        self.want = self.buf.clone()
        good = torch.tensor(self.ok, dtype=torch.bool, device=DEV)
        if B and bool(good.any()):
            self.rows(self.want, B, rw)[good] = S.bits(want).to(DEV)[good]

    def rows(self, buf, B, rw):
        return buf.as_strided((B, rw), (self.stride, 1), self.start)

    def check(self, status=None, what=""):
        torch.cuda.synchronize()
        if status is not None:
            assert status.cpu().reshape(-1).tolist() == self.ok, what
        got_f, want_f = self.buf.view(self.out_dtype), self.want.view(self.out_dtype)
        same = (self.buf == self.want) | (torch.isnan(want_f) & torch.isnan(got_f))
        if not bool(same.all()):
            bad = torch.nonzero(~same).reshape(-1)
            at = int(bad[0])
            raise AssertionError(f"{what}: {bad.numel()} words differ, first at buffer word {at} "
                                 f"(got {int(self.buf[at]):#x}, want {int(self.want[at]):#x}; rows start at "
                                 f"{self.start}, stride {self.stride})")


def tensors(idx, offsets, bits):
    return (torch.tensor(idx, dtype=IDX_T[bits], device=DEV).reshape(len(idx)),
            torch.tensor(offsets, dtype=IDX_T[bits], device=DEV))


def pool(C, ws, ft, arch, rw, idx, offsets, bits, dest, pb=10, **kw):
    it, ot = tensors(idx, offsets, bits)
    status = torch.full([len(offsets) - 1], 7, dtype=torch.uint8, device=DEV)
    out, ok = C.gather_rows_sum(arch, rw, it, ot, TORCH_FLOAT[ft], out=dest.out, out_status=status, prob_bits=pb,
                                ws=ws, **kw)
    assert out is dest.out and ok is status
    return status


def c_abi(N, ws, ft, arch, rw, it, ot, dest, status, pb=10):
    rc = N.lib().dietgpu_float_gather_rows_sum(
        ws.h, ft, pb, arch.data_ptr(), rw, ot.numel() - 1, it.numel(), it.data_ptr(), ot.data_ptr(),
        int(it.dtype == torch.int64), dest.out.data_ptr(), int(dest.out_dtype == torch.float32), dest.stride,
        status.data_ptr() if status is not None else None, torch.cuda.current_stream().cuda_stream)
    assert rc == N.DIETGPU_OK, N.lib().dietgpu_last_error()


# (output offset in words, stride padding, archive 4 B off)
PLACEMENTS = [(off, pad, shifted) for off in (0, 1) for pad in (0, 3) for shifted in (False, True)]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rw", S.ROW_WORDS)
def test_bag_lists(C, ws, form, rw):
    """Every bag list of the width in one call, int32 and int64, on every
    placement: output base 16 B-aligned and one word off, stride rw and
    rw + 3, archive 16 B-aligned and 4 B off.  Then every list alone (the odd
    task counts)."""
    ft, out_dtype = form
    t, a16, a4 = table(ft)
    bags = S.all_bags(rw)
    want = _MODELS.get((form, rw), lambda: S.pooled(t, rw, bags, out_dtype))
    idx, offsets = S.flatten(bags)
    for off, pad, shifted in PLACEMENTS:
        for bits in (32, 64):
            dest = Dest(out_dtype, want, [1] * len(bags), off, pad)
            status = pool(C, ws, ft, a4 if shifted else a16, rw, idx, offsets, bits, dest)
            dest.check(status, f"all lists off {off} pad {pad} shifted {shifted} int{bits}")
    at = 0
    for name, (some, _) in sorted(S.bag_lists(rw).items()):
        idx, offsets = S.flatten(some)
        dest = Dest(out_dtype, want[at: at + len(some)], [1] * len(some), 1, 3)
        status = pool(C, ws, ft, a4, rw, idx, offsets, 64, dest)
        dest.check(status, name)
        at += len(some)


@pytest.mark.parametrize("bits", [32, 64])
def test_more_task_groups_than_resident_workgroups(C, ws, bits):
    """70,000 bags of one or two 8-word rows: the workgroups stride over the
    task groups, the half-waves take one task after another."""
    t, a16, _ = table(2)
    bags = _MODELS.get("long-bags", S.long_bags)
    want = _MODELS.get("long", lambda: S.pooled(t, S.LONG_RW, bags, torch.bfloat16))
    idx, offsets = S.flatten(bags)
    dest = Dest(torch.bfloat16, want, [1] * len(bags))
    status = pool(C, ws, 2, a16, S.LONG_RW, idx, offsets, bits, dest)
    dest.check(status, "long list")


# ------------------------------------------------------------ value cases ----

@pytest.mark.parametrize("form", FORMS[:4], ids=FORM_IDS[:4])
def test_every_16_bit_pattern_pooled_in_pairs(C, ws, form):
    ft, out_dtype = form
    t = S.all_patterns(TORCH_FLOAT[ft])
    a16, a4 = oracle_archive(S.bits(t).numpy().view(np.uint16), ft)
    bags = S.pattern_pairs()
    want = S.pooled(t, 64, bags, out_dtype)
    idx, offsets = S.flatten(bags)
    for arch, off, bits in ((a16, 0, 32), (a4, 1, 64)):
        dest = Dest(out_dtype, want, [1] * len(bags), off)
        status = pool(C, ws, ft, arch, 64, idx, offsets, bits, dest)
        dest.check(status, "patterns")
    # and alone: a one-row bag returns the row, -0.0 and every NaN included
    alone = [[r] for r in range(1024)]
    idx, offsets = S.flatten(alone)
    dest = Dest(out_dtype, S.pooled(t, 64, alone, out_dtype), [1] * 1024)
    status = pool(C, ws, ft, a16, 64, idx, offsets, 32, dest)
    dest.check(status, "patterns alone")
    if out_dtype != torch.float32:
        got = S.bits(dest.out.cpu()).view(-1)
        nan = torch.isnan(t[:65536])
        assert torch.equal(got[~nan], S.bits(t[:65536])[~nan])


def test_fp32_special_values(C, ws):
    t, bags = S.fp32_specials()
    a16, a4 = oracle_archive(S.bits(t).numpy().view(np.uint32), 3)
    want = S.pooled(t, 8, bags, torch.float32)
    idx, offsets = S.flatten(bags)
    for arch, off, bits in ((a16, 0, 64), (a4, 1, 32)):
        dest = Dest(torch.float32, want, [1] * len(bags), off)
        status = pool(C, ws, 3, arch, 8, idx, offsets, bits, dest)
        dest.check(status, "fp32 specials")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_order_probe(C, ws, form):
    """The adds are in list order: each permutation of {1, 2^-24, 2^-24, -1}
    gives the sum its own order gives."""
    ft, out_dtype = form
    t, bags = S.order_probe(TORCH_FLOAT[ft])
    a16, _ = oracle_archive(S.bits(t).numpy().view(NP_WORD[ft]), ft)
    want = S.pooled(t, 8, bags, out_dtype)
    assert len({float(v) for v in want[:, 0].float()}) == 3
    idx, offsets = S.flatten(bags)
    dest = Dest(out_dtype, want, [1] * len(bags))
    status = pool(C, ws, ft, a16, 8, idx, offsets, 64, dest)
    dest.check(status, "order probe")


# ---------------------------------------------------------- failure cases ----

@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rw", [8, 257, 4097])
@pytest.mark.parametrize("bits", [32, 64])
def test_bags_with_a_bad_index(C, N, ws, form, rw, bits):
    """-1, R, R + 5 (and 2^31, 2^40, INT64_MIN as int64) among good rows:
    status 0, the row untouched, the neighbours exact.  With and without a
    status array."""
    ft, out_dtype = form
    t, a16, a4 = table(ft)
    bags, ok = S.failing_bags(rw, wide=bits == 64)
    idx, offsets = S.flatten(bags)
    good_bags, ok2 = raw_bags(idx, offsets, rw, G.rows_of(rw))
    assert ok2 == ok and 0 in ok
    want = S.pooled(t, rw, good_bags, out_dtype)
    for off, pad, arch in ((0, 0, a16), (1, 3, a4)):
        dest = Dest(out_dtype, want, ok, off, pad)
        status = pool(C, ws, ft, arch, rw, idx, offsets, bits, dest)
        dest.check(status, "with status")
        dest = Dest(out_dtype, want, ok, off, pad)
        c_abi(N, ws, ft, arch, rw, *tensors(idx, offsets, bits), dest, None)
        dest.check(None, "without status")


@pytest.mark.parametrize("form", [FORMS[2], FORMS[4]], ids=[FORM_IDS[2], FORM_IDS[4]])
@pytest.mark.parametrize("bits", [32, 64])
def test_bad_offsets(C, N, ws, form, bits):
    """A decreasing offset, a negative offset and a final offset past numIdx
    fail the bags they bound, and only those."""
    ft, out_dtype = form
    t, a16, _ = table(ft)
    rw = 64
    R = G.rows_of(rw)
    idx = [5, R - 1, 0, 17, 3, 9, 11, 2]
    cases = {
        "decreasing": [0, 2, 5, 4, 6, 8],      # bag 2 runs backwards; bags 1 and 3 are fine
        "negative": [-1, 2, 4, 4, 8],          # bag 0 starts before idx
        "negative_middle": [0, 2, -3, 4, 8],   # bags 1 and 2
        "past_the_end": [0, 3, 6, 9],          # the last bag ends past numIdx
        "all_past_the_end": [9, 9, 12],        # an empty bag out of range fails too
        "huge": [0, 4, (1 << 31) - 1 if bits == 32 else 1 << 40],
    }
    for name, offsets in cases.items():
        bags, ok = raw_bags(idx, offsets, rw, R)
        assert 0 in ok, name
        want = S.pooled(t, rw, bags, out_dtype)
        dest = Dest(out_dtype, want, ok, 1, 3)
        status = pool(C, ws, ft, a16, rw, idx, offsets, bits, dest)
        dest.check(status, name)
        dest = Dest(out_dtype, want, ok)
        c_abi(N, ws, ft, a16, rw, *tensors(idx, offsets, bits), dest, None)
        dest.check(None, name + " without status")
    assert raw_bags(idx, cases["decreasing"], rw, R)[1] == [1, 1, 0, 1, 1]
    assert raw_bags(idx, cases["all_past_the_end"], rw, R)[1] == [0, 0]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("how", ["other_type", "other_prob_bits", "corrupt_magic"])
def test_failing_archive(C, ws, form, how):
    """Every status is 0, an empty bag's too, and nothing is written."""
    ft, out_dtype = form
    t, a16, _ = table(ft)
    call_ft, pb, arch = ft, 10, a16
    if how == "other_type":
        # (the header names another type; the layout stays, so every header
        # read stays inside the archive)
        arch = retyped(a16, ft)
    elif how == "other_prob_bits":
        pb = 11
    else:
        arch = a16.clone()
        arch[0] ^= 1
    for rw, bags in ((8, [[0, 1], [], [5000]]), (4097, [[0, 6, 3]]), (1, [[0]])):
        idx, offsets = S.flatten(bags)
        for bits in (32, 64):
            dest = Dest(out_dtype, torch.zeros([len(bags), rw], dtype=out_dtype), [0] * len(bags))
            status = pool(C, ws, call_ft, arch, rw, idx, offsets, bits, dest, pb=pb)
            dest.check(status, f"{how} rw {rw}")


# ------------------------------------------------------------ other cases ----

@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("pb", [9, 11])
def test_prob_bits(C, ws, form, pb):
    ft, out_dtype = form
    t, a16, a4 = table(ft, pb)
    for rw in (64, 257):
        bags = S.bag_lists(rw)["edges"][0] + S.bag_lists(rw)["lengths"][0][:5]
        want = S.pooled(t, rw, bags, out_dtype)
        idx, offsets = S.flatten(bags)
        for arch, off in ((a16, 0), (a4, 1)):
            dest = Dest(out_dtype, want, [1] * len(bags), off)
            status = pool(C, ws, ft, arch, rw, idx, offsets, 64, dest, pb=pb)
            dest.check(status, f"pb {pb} rw {rw}")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_gpu_compressed_archive(C, ws, form):
    ft, out_dtype = form
    t = table(ft)[0]
    arch = compress_one(C, ws, S.table_words(ft), ft)
    rw = 257
    bags = S.all_bags(rw)
    want = _MODELS.get((form, rw), lambda: S.pooled(t, rw, bags, out_dtype))
    idx, offsets = S.flatten(bags)
    dest = Dest(out_dtype, want, [1] * len(bags), 1, 3)
    status = pool(C, ws, ft, arch, rw, idx, offsets, 32, dest)
    dest.check(status, "GPU archive")


def test_side_stream(C, ws):
    t, a16, _ = table(2)
    rw = 257
    bags = S.all_bags(rw)
    want = _MODELS.get((FORMS[3], rw), lambda: S.pooled(t, rw, bags, torch.float32))
    idx, offsets = S.flatten(bags)
    dest = Dest(torch.float32, want, [1] * len(bags), 1, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        status = pool(C, ws, 2, a16, rw, idx, offsets, 64, dest)
    side.synchronize()
    dest.check(status, "side stream")


@pytest.mark.parametrize("bits", [32, 64])
def test_no_bags_and_only_empty_bags(C, N, ws, bits):
    t, a16, _ = table(2)
    # B = 0: one offset, nothing written, nothing launched
    dest = Dest(torch.bfloat16, torch.zeros([0, 64], dtype=torch.bfloat16), [])
    it, ot = tensors([3, 4], [0], bits)
    out, ok = C.gather_rows_sum(a16, 64, it, ot, torch.bfloat16, ws=ws)
    assert tuple(out.shape) == (0, 64) and tuple(ok.shape) == (0,)
    c_abi(N, ws, 2, a16, 64, it, ot, dest, None)
    dest.check(None, "no bags")
    # all bags empty, with and without indices behind them
    for idx, offsets in (([], [0, 0, 0, 0]), ([1, 2, 3], [3, 3, 3]), ([1, 2, 3], [0, 0])):
        B = len(offsets) - 1
        for out_dtype in (torch.bfloat16, torch.float32):
            dest = Dest(out_dtype, torch.zeros([B, 64], dtype=out_dtype), [1] * B, 1, 3)
            status = pool(C, ws, 2, a16, 64, idx, offsets, bits, dest)
            dest.check(status, "empty bags")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_torch_operator(C, ws, form):
    """With and without temp_mem / out_status; float32 outputs read the
    archive's type from its header."""
    ft, out_dtype = form
    t, a16, a4 = table(ft)
    op = torch.ops.dietgpu.gather_rows_sum
    rw = 257
    bags, ok = S.failing_bags(rw, wide=True)
    idx, offsets = S.flatten(bags)
    want = S.pooled(t, rw, raw_bags(idx, offsets, rw, G.rows_of(rw))[0], out_dtype)
    it, ot = tensors(idx, offsets, 64)
    tmp = torch.empty([1 << 20], dtype=torch.uint8, device=DEV)
    for temp_mem, with_status, arch, off, pad in ((None, False, a16, 0, 0), (tmp, True, a4, 1, 3),
                                                  (None, True, a16, 0, 3), (tmp, False, a4, 1, 0)):
        dest = Dest(out_dtype, want, ok, off, pad)
        status = torch.full([len(bags)], 7, dtype=torch.uint8, device=DEV) if with_status else None
        used = op(arch, rw, it, ot, dest.out, temp_mem, status)
        assert isinstance(used, int) and used >= 0
        dest.check(status, "operator")
    # the guards that need device tensors, each with its own message
    o = torch.empty([len(bags), rw], dtype=out_dtype, device=DEV)
    with pytest.raises(RuntimeError, match="compressed inputs must be 4-byte aligned"):
        shifted = torch.empty([a16.numel() + 16], dtype=torch.uint8, device=DEV)
        op(shifted[1: 1 + a16.numel()], rw, it, ot, o)
    with pytest.raises(RuntimeError, match="at least the 32-byte archive header"):
        op(a16[:16], rw, it, ot, o)
    with pytest.raises(RuntimeError, match="compressed inputs must be contiguous GPU tensors on one device"):
        op(a16.cpu(), rw, it, ot, o)
    with pytest.raises(RuntimeError, match="t_out must be on the archive's device"):
        op(a16, rw, it, ot, o.cpu())
    with pytest.raises(RuntimeError, match="t_idx and t_offsets must be contiguous GPU tensors"):
        op(a16, rw, it.cpu(), ot, o)
    with pytest.raises(RuntimeError, match=f"out_status must have {len(bags)} entries"):
        op(a16, rw, it, ot, o, None, torch.empty([len(bags) + 1], dtype=torch.uint8, device=DEV))


def test_torch_operator_refuses_an_fp64_archive_for_float32_outputs(C, ws):
    w = np.random.default_rng(3).standard_normal(4096).view(np.uint64)
    a = torch.from_numpy(np.asarray(O.float_compress(w, 4), dtype=np.uint8).copy()).to(DEV)
    it, ot = tensors([0, 1], [0, 2], 64)
    o = torch.full([1, 64], 3.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="gather_rows_sum takes float16, bfloat16 or float32 archives"):
        torch.ops.dietgpu.gather_rows_sum(a, 64, it, ot, o)
    torch.cuda.synchronize()
    assert bool((o == 3.0).all())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_c_abi_through_ctypes(C, N, ws, form):
    ft, out_dtype = form
    t, a16, a4 = table(ft)
    for rw, bits, arch, off, pad in ((64, 32, a16, 0, 0), (4097, 64, a4, 1, 3)):
        bags, ok = S.failing_bags(rw, wide=bits == 64)
        idx, offsets = S.flatten(bags)
        want = S.pooled(t, rw, raw_bags(idx, offsets, rw, G.rows_of(rw))[0], out_dtype)
        dest = Dest(out_dtype, want, ok, off, pad)
        status = torch.full([len(bags)], 7, dtype=torch.uint8, device=DEV)
        c_abi(N, ws, ft, arch, rw, *tensors(idx, offsets, bits), dest, status)
        dest.check(status, "C ABI")
    # an archive off 4 B alignment is refused by the call, nothing is launched
    odd = torch.empty([a16.numel() + 16], dtype=torch.uint8, device=DEV)[2: 2 + a16.numel()]
    dest = Dest(out_dtype, torch.zeros([1, 64], dtype=out_dtype), [0])
    it, ot = tensors([0, 1], [0, 2], 32)
    rc = N.lib().dietgpu_float_gather_rows_sum(ws.h, ft, 10, odd.data_ptr(), 64, 1, 2, it.data_ptr(), ot.data_ptr(), 0,
                                               dest.out.data_ptr(), int(out_dtype == torch.float32), 64, None, None)
    assert rc == N.DIETGPU_ERR_INVALID and b"must be 4-byte aligned" in N.lib().dietgpu_last_error()
    dest.check(None, "refused call")


def test_the_c_plus_plus_entry_point_rejects_through_the_test_hook(C, N, ws):
    """A config with useChecksum set, an fp64 archive type, and a 16-bit out
    of an fp32 archive (the C ABI and the layers above carry no checksum flag
    and refuse the types themselves)."""
    t, a16, _ = table(2)
    T = N.testlib()
    bags = [[3, 0], [5]]
    idx, offsets = S.flatten(bags)
    it, ot = tensors(idx, offsets, 64)
    stream = torch.cuda.current_stream().cuda_stream
    want = S.pooled(t, 64, bags, torch.bfloat16)

    def hook(ft, checksum, out32, dest, status):
        return T.dietgpu_test_gather_sum_config(ws.h, ft, checksum, a16.data_ptr(), 64, 2, 3, it.data_ptr(),
                                                ot.data_ptr(), dest.out.data_ptr(), out32, status.data_ptr(), stream)

    for ft, checksum, out32, msg in ((2, 1, 0, b"a pooled row gather cannot verify a checksum"),
                                     (4, 0, 1, b"a pooled row gather takes fp16, bf16 or fp32 archives"),
                                     (3, 0, 0, b"the pooled rows of an fp32 archive are fp32")):
        dest = Dest(torch.bfloat16, want, [0, 0])
        status = torch.full([2], 7, dtype=torch.uint8, device=DEV)
        assert hook(ft, checksum, out32, dest, status) == N.DIETGPU_ERR_INVALID
        assert msg in T.dietgpu_test_last_error()
        dest.check(None, "rejected config")
        assert status.cpu().tolist() == [7, 7]
    # the same call without the flag pools
    dest = Dest(torch.bfloat16, want, [1, 1])
    status = torch.full([2], 7, dtype=torch.uint8, device=DEV)
    assert hook(2, 0, 0, dest, status) == N.DIETGPU_OK, T.dietgpu_test_last_error()
    dest.check(status, "accepted config")


def test_check_raises(C, N, ws):
    t, a16, _ = table(2)
    R = G.rows_of(64)
    it, ot = tensors([0, R - 1, 5], [0, 2, 3], 32)
    out, ok = C.gather_rows_sum(a16, 64, it, ot, torch.bfloat16, ws=ws, check=True)
    assert bool(ok.all()) and out.dtype == torch.bfloat16
    assert bool(S.same(out.cpu(), S.pooled(t, 64, [[0, R - 1], [5]], torch.bfloat16)).all())
    out, ok = C.gather_rows_sum(a16, 64, it, ot, torch.bfloat16, out_dtype=torch.float32, ws=ws, check=True)
    assert out.dtype == torch.float32
    assert bool(S.same(out.cpu(), S.pooled(t, 64, [[0, R - 1], [5]], torch.float32)).all())
    with pytest.raises(N.DietGpuError, match="lie outside idx or the table"):
        C.gather_rows_sum(a16, 64, *tensors([0, R], [0, 2], 64), torch.bfloat16, ws=ws, check=True)
    with pytest.raises(N.DietGpuError, match="does not match dtype"):
        C.gather_rows_sum(a16, 64, it, ot, torch.float16, ws=ws, check=True)
    _, ok = C.gather_rows_sum(a16, 64, *tensors([0, R, 1], [0, 1, 2, 3], 64), torch.bfloat16, ws=ws)
    assert ok.cpu().tolist() == [1, 0, 1]


def test_python_wrapper_rejects_a_bad_out_or_status(C, ws):
    """The wrapper's checks that sit behind its device check: an `out` too
    small for B rows at its stride, of another width, shape, dtype or device,
    rows that overlap or a strided last dimension, and an out_status of the
    wrong length, dtype or layout.  Each is matched to its message; nothing is
    launched, so `out` and `out_status` keep their contents."""
    _, a16, _ = table(2)
    bf, rw = torch.bfloat16, 64
    it, ot = tensors([0, 1, 2, 3, 4, 5], [0, 2, 3, 5, 6], 64)  # B = 4

    def filled(shape, dtype=bf, device=DEV):
        return torch.full(shape, 3, dtype=dtype, device=device)

    shape_msg = r"out must be a torch.bfloat16 tensor of shape \[4, 64\] on idx's device"
    stride_msg = "out's last dimension must be contiguous and its rows must lie at a constant stride of at least"
    status_msg = "out_status must be a contiguous uint8 tensor of 4 entries"
    cases = {
        "too-few-rows": (filled([3, rw]), None, shape_msg),
        "too-many-rows": (filled([5, rw]), None, shape_msg),
        "other-width": (filled([4, rw + 1]), None, shape_msg),
        "flat": (filled([4 * rw]), None, shape_msg),
        "extra-dim": (filled([1, 4, rw]), None, shape_msg),
        "on-the-host": (filled([4, rw], device="cpu"), None, shape_msg),
        "rows-overlap": (filled([rw]).as_strided((4, rw), (0, 1)), None, stride_msg),
        "rows-too-close": (filled([4 * rw]).as_strided((4, rw), (rw - 1, 1)), None, stride_msg),
        "last-dim-strided": (filled([4, 2 * rw])[:, ::2], None, stride_msg),
        "status-too-short": (filled([4, rw]), filled([3], torch.uint8), status_msg),
        "status-too-long": (filled([4, rw]), filled([5], torch.uint8), status_msg),
        "status-int8": (filled([4, rw]), filled([4], torch.int8), status_msg),
        "status-bool": (filled([4, rw]), filled([4], torch.bool), status_msg),
        "status-2d": (filled([4, rw]), filled([2, 2], torch.uint8), status_msg),
        "status-strided": (filled([4, rw]), filled([8], torch.uint8)[::2], status_msg),
        "status-on-the-host": (filled([4, rw]), filled([4], torch.uint8, "cpu"), status_msg),
    }
    for name, (out, status, msg) in cases.items():
        keep_out = out.clone()
        keep_status = status.clone() if status is not None else None
        with pytest.raises(ValueError, match=msg):
            C.gather_rows_sum(a16, rw, it, ot, bf, out=out, out_status=status, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(out, keep_out), name
        assert status is None or torch.equal(status, keep_status), name
    # a wrong dtype of `out` is named as the out dtype it implies; out_dtype given, it is a shape error
    with pytest.raises(ValueError, match="out dtype torch.float16 does not go with torch.bfloat16"):
        C.gather_rows_sum(a16, rw, it, ot, bf, out=filled([4, rw], torch.float16), ws=ws)
    with pytest.raises(ValueError, match=r"out must be a torch.float32 tensor of shape \[4, 64\]"):
        C.gather_rows_sum(a16, rw, it, ot, bf, out=filled([4, rw]), out_dtype=torch.float32, ws=ws)
    # idx and offsets on the device but one of them not: still the device check
    with pytest.raises(ValueError, match="idx and offsets must be CUDA tensors on one device"):
        C.gather_rows_sum(a16, rw, it.cpu(), ot, bf, ws=ws)
    # the same tensors, well-formed, pool
    out, status = filled([4, rw]), filled([4], torch.uint8)
    got, ok = C.gather_rows_sum(a16, rw, it, ot, bf, out=out, out_status=status, ws=ws)
    assert got is out and ok is status and bool(ok.all())


def test_graph_capture_replay(C):
    """Captured once; replayed after new indices, new offsets and new archive
    bytes were written into the same buffers.  The same bits on every replay
    of the same inputs."""
    n, rw, B, m = S.N_TABLE, 257, 40, 300
    R = n // rw
    ws = C.Workspace(16 << 20)
    abuf = torch.zeros([C.max_float_compressed_size(2, n)], dtype=torch.uint8, device=DEV)
    idx = torch.zeros([m], dtype=torch.int64, device=DEV)
    offsets = torch.zeros([B + 1], dtype=torch.int64, device=DEV)
    out = torch.empty([B, rw], dtype=torch.float32, device=DEV)
    ok = torch.empty([B], dtype=torch.uint8, device=DEV)

    def load(seed):
        """New table, new archive bytes in abuf, new bags (one of them bad)."""
        w = S.table_words(2, seed=seed)
        a = torch.from_numpy(np.asarray(O.float_compress(w, 2), dtype=np.uint8).copy())
        abuf.zero_()
        abuf[: a.numel()] = a.to(DEV)
        rng = np.random.default_rng(seed)
        rows = rng.integers(0, R, m)
        rows[seed % m] = R + seed
        cuts = np.sort(rng.integers(0, m + 1, B - 1))
        offs = [0] + cuts.tolist() + [m]
        idx.copy_(torch.from_numpy(rows))
        offsets.copy_(torch.tensor(offs))
        bags, good = raw_bags(rows.tolist(), offs, rw, R)
        return S.pooled(S.as_ints(w).view(torch.bfloat16), rw, bags, torch.float32), good

    load(1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # warm-up outside the capture
        C.gather_rows_sum(abuf, rw, idx, offsets, torch.bfloat16, out=out, out_status=ok, ws=ws)
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        C.gather_rows_sum(abuf, rw, idx, offsets, torch.bfloat16, out=out, out_status=ok, ws=ws)
    for rep in range(3):
        want, good = load(100 + rep)
        assert 0 in good
        runs = []
        for _ in range(2):
            out.view(torch.int32).fill_(0x5A5A5A5A)
            ok.fill_(7)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            runs.append(out.view(torch.int32).clone())
        assert ok.cpu().tolist() == good, f"replay {rep}"
        keep = torch.tensor(good, dtype=torch.bool)
        expect = torch.full([B, rw], 0x5A5A5A5A, dtype=torch.int32)
        expect[keep] = S.bits(want)[keep]
        assert torch.equal(runs[0].cpu(), expect), f"replay {rep}"
        assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_equals_the_row_gather_then_the_sequential_sum(C, ws, form):
    """Bit for bit the rows gather_rows_device returns, summed in list order
    in fp32 on the device and rounded once."""
    ft, out_dtype = form
    _, a16, _ = table(ft)
    rw = 257
    bags = S.bag_lists(rw)["lengths"][0][:5] + S.bag_lists(rw)["edges"][0]
    idx, offsets = S.flatten(bags)
    it, ot = tensors(idx, offsets, 64)
    rows, ok = C.gather_rows_device(a16, rw, it, TORCH_FLOAT[ft], ws=ws)
    fused, ok2 = C.gather_rows_sum(a16, rw, it, ot, TORCH_FLOAT[ft], out_dtype=out_dtype, ws=ws)
    torch.cuda.synchronize()
    assert bool(ok.all()) and bool(ok2.all())
    for b, (lo, up) in enumerate(zip(offsets, offsets[1:])):
        acc = torch.zeros([rw], dtype=torch.float32, device=DEV)
        for k in range(lo, up):
            acc = rows[k].float() if k == lo else acc + rows[k].float()
        assert torch.equal(S.bits(acc.to(out_dtype)), S.bits(fused[b])), b


def test_profiling_counts_one_launch_of_its_own_family(C, ws):
    _, a16, _ = table(2)
    it, ot = tensors([0, 1, 2, 3], [0, 2, 4], 64)
    C.profile(True)
    try:
        C.profile_reset()
        C.gather_rows_sum(a16, 64, it, ot, torch.bfloat16, ws=ws)
        torch.cuda.synchronize()
        assert C.profile_query("decode_gather_sum")[1] == 1
        assert C.profile_query("decode_gather")[1] == 0 and C.profile_query("decode")[1] == 0
    finally:
        C.profile(False)
