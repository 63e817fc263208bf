"""GPU tests of the torch.ops.dietgpu layer (csrc/torch_ops.cpp): every
operator, argument form and rejection.

References are the CPU oracle for archives (compared byte for byte) and the
input words for roundtrips (compared on integer views); there is no
tolerance anywhere.  Inputs come from the seeded generators of tests/util.py.
Every destination and caller buffer is carved from a buffer of 0xA5 bytes with
at least 16 canary words on each side, and the whole buffer is compared: a
stray write, or any write for a failing member, fails the test.

Groups: (a) byte mode on uint8, wider and mixed dtypes; (b) caller-supplied
out_compressed / out_compressed_bytes; (c) the split-size operators per
split; (d) batches with failing members through the full decoder; (e) the
_simple operators and their integer temp_mem; (f) input forms (n-d, offset
views, empty members, a side stream); (g) the size operators; (h) the
rejections, the argument guards among them.  tests/test_torch_ops_args.py
holds the rejections that fire without a device."""
import types
from functools import partial

import numpy as np
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from oracle import oracle as O
from tests.gpu_harness import (C, DEV, Cache, compress_one, retyped, to_dev, to_host_words,  # noqa: F401
                               workspace_fixture)
from tests.test_gpu_adversarial import byte_members, float_members, ref_archives
from tests.util import FT_IDS, NP_SIGNED, TORCH_OUT, WORD_BYTES, exp_bytes, float_words

pytestmark = pytest.mark.gpu

D = torch.ops.dietgpu
ALL_FT = [0, 1, 2, 3, 4]  # ft 0 = the byte codec
FILL = 0xA5
PAD = 128  # canary bytes on each side of a carved region: 16 words of the widest type
I32 = torch.int32

ws = workspace_fixture(64 << 20)
dev = partial(to_dev, as_float=True)  # a device tensor of the codec's dtype holding the words


@pytest.fixture(scope="module")
def tmp():
    return torch.empty([64 << 20], dtype=torch.uint8, device=DEV)


# ---------------------------------------------------------------------------
# inputs and oracle archives: computed once, shared, left unchanged
# ---------------------------------------------------------------------------
_CACHE = Cache()


def elem(ft, n, seed=0):
    """n words of type ft (bytes for ft 0), seeded by (ft, n, seed)."""
    def make():
        s = 1000 * seed + 10 * (n % 97) + ft
        return exp_bytes(n, lam=20.0, seed=s + 1) if ft == 0 else float_words(ft, n, seed=s)
    return _CACHE.get(("elem", ft, n, seed), make)


def oracle(ft, words, checksum=False):
    """The oracle's archive of `words` (as bytes when ft == 0)."""
    key = ("oracle", ft, words.dtype.str, words.size, hash(words.tobytes()), checksum)
    if ft == 0:
        return _CACHE.get(key, lambda: O.ans_encode(words.view(np.uint8), 10, checksum))
    return _CACHE.get(key, lambda: O.float_compress(words, ft, 10, checksum))


class Carved:
    """Regions of given byte sizes inside one 0xA5 buffer, each starting
    `off` bytes after a 16 B boundary with PAD canary bytes on each side."""

    def __init__(self, specs):
        self.spans, cur = [], 0
        for nbytes, off in specs:
            st = -(-(cur + PAD) // 16) * 16 + off
            self.spans.append((st, nbytes))
            cur = st + nbytes + PAD
        total = -(-cur // 16) * 16
        self.buf = torch.full([total], FILL, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.expect = np.full(total, FILL, dtype=np.uint8)

    def region(self, i, dtype=torch.uint8):
        st, nbytes = self.spans[i]
        return self.buf[st: st + nbytes].view(dtype)

    def expect_words(self, i, words, at=0):
        """`words` are expected from byte `at` of region i on."""
        st, nbytes = self.spans[i]
        b = np.ascontiguousarray(words).view(np.uint8)
        assert at + b.size <= nbytes
        self.expect[st + at: st + at + b.size] = b

    def check(self, what=""):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.expect)
        assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first at buffer byte {bad[0]} "
                               f"(regions {self.spans})")


def check_rows(comp, sizes, refs):
    """Reported sizes first, then the bytes of every row."""
    sizes_h = sizes.cpu().tolist()
    host = comp.cpu().numpy()
    assert [sizes_h[i] for i in range(len(refs))] == [r.size for r in refs]
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(host[i, : ref.size], ref, err_msg=f"archive {i}")
    return sizes_h


def check_list(archives, refs):
    assert len(archives) == len(refs)
    for i, (a, ref) in enumerate(zip(archives, refs)):
        assert a.dtype == torch.uint8 and a.numel() == ref.size, (i, a.numel(), ref.size)
        np.testing.assert_array_equal(a.cpu().numpy(), ref, err_msg=f"archive {i}")


def status_tensors(n):
    return (torch.full([n], 7, dtype=torch.uint8, device=DEV), torch.full([n], -1, dtype=I32, device=DEV))


def float_max(ft, n):
    return D.max_float_compressed_size(torch.empty(0, dtype=TORCH_OUT[ft]), n)


# ---------------------------------------------------------------------------
# a. byte mode against the oracle
# ---------------------------------------------------------------------------
U8, I32T, F32, F64 = torch.uint8, torch.int32, torch.float32, torch.float64
# (dtype, numel).  mixed: the widest member in bytes (fp64, 32,760 B) is
# neither the first tensor nor the one of the most elements (4097)
BYTE_LISTS = {
    "uint8": [(U8, n) for n in (1, 7, 4095, 4096, 4097, 12345, 70001)],
    "int32": [(I32T, n) for n in (1, 7, 4095, 4097)],
    "fp32": [(F32, n) for n in (4096, 1, 4097)],
    "mixed": [(U8, 4097), (I32T, 4096), (F64, 4095), (U8, 7), (I32T, 1), (F64, 1)],
}
FT_OF_SIZE = {1: 0, 2: 2, 4: 3, 8: 4}


def member_bytes(dtype, n, seed):
    return elem(FT_OF_SIZE[dtype.itemsize], n, seed).view(np.uint8)


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
@pytest.mark.parametrize("kind", BYTE_LISTS)
def test_byte_mode(C, tmp, kind, checksum):
    """compress_data(False, ...) encodes every tensor as its bytes; the rows
    are sized for the widest member in bytes; decompress_data(False, ...)
    restores outputs of the original dtypes."""
    spec = BYTE_LISTS[kind]
    hb = [member_bytes(dt, n, seed=i) for i, (dt, n) in enumerate(spec)]
    ts = [torch.from_numpy(b.copy()).to(DEV).view(dt) for b, (dt, _) in zip(hb, spec)]
    widest = max(b.size for b in hb)
    if kind == "mixed":
        assert widest > ts[0].numel() * ts[0].element_size()
        assert widest > max(t.numel() for t in ts) * ts[0].element_size()
    rc = tuple(D.max_any_compressed_output_size(ts))
    assert rc == (len(ts), C.max_compressed_size(widest))
    comp, sizes, used = D.compress_data(False, ts, checksum, tmp)
    assert tuple(comp.shape) == rc and comp.dtype == torch.uint8 and isinstance(used, int)
    refs = [oracle(0, b, checksum) for b in hb]
    sizes_h = check_rows(comp, sizes, refs)
    # outputs of the original dtypes, at word offsets 0 and 1 from 16 B
    cv = Carved([(b.size, (i % 2) * dt.itemsize) for i, (b, (dt, _)) in enumerate(zip(hb, spec))])
    outs = [cv.region(i, dt) for i, (dt, _) in enumerate(spec)]
    for i, b in enumerate(hb):
        cv.expect_words(i, b)
    st, sz = status_tensors(len(ts))
    D.decompress_data(False, [comp[i, : sizes_h[i]] for i in range(len(ts))], outs, checksum, tmp, st, sz)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [1] * len(ts)
    assert sz.cpu().tolist() == [b.size for b in hb]
    cv.check(kind)


# ---------------------------------------------------------------------------
# b. caller-supplied out_compressed / out_compressed_bytes
# ---------------------------------------------------------------------------
EXTRA_ROWS, EXTRA_COLS = 2, 48


@pytest.mark.parametrize("op", ["compress_data", "compress_data_split_size"])
@pytest.mark.parametrize("ft", ALL_FT, ids=FT_IDS.get)
def test_caller_supplied_outputs(tmp, ft, op):
    """The archives land in the caller's matrix, row i at the caller's
    stride; rows >= n, columns >= the required width and size entries >= n
    stay as they were.  (Bytes between an archive's end and the required
    width belong to the encoders.)"""
    ns = [4096, 8, 12345] if ft == 0 else [4097, 7, 12345]
    words = [elem(ft, n, seed=2) for n in ns]
    refs = [oracle(ft, w) for w in words]
    n = len(ns)
    if op == "compress_data":
        ts = [dev(w, ft) for w in words]
        cols = (D.max_float_compressed_output_size(ts) if ft else D.max_any_compressed_output_size(ts))[1]
    else:
        t_in = dev(np.concatenate(words), ft)
        cols = float_max(ft, max(ns)) if ft else D.max_any_compressed_size(max(ns))
    width = cols + EXTRA_COLS
    mat = torch.full([n + EXTRA_ROWS, width], FILL, dtype=torch.uint8, device=DEV)
    szs = torch.full([n + EXTRA_ROWS], -1, dtype=I32, device=DEV)
    if op == "compress_data":
        comp, sizes, _ = D.compress_data(bool(ft), ts, False, tmp, mat, szs)
        assert comp.data_ptr() == mat.data_ptr() and comp.shape == mat.shape
    else:
        lst, sizes, _ = D.compress_data_split_size(bool(ft), t_in, torch.tensor(ns, dtype=I32), False, tmp, mat, szs)
        # views of the caller's matrix, not copies
        for i, (a, ref) in enumerate(zip(lst, refs)):
            assert a.data_ptr() == mat.data_ptr() + i * width and a.numel() == ref.size
            assert a.untyped_storage().data_ptr() == mat.untyped_storage().data_ptr()
        check_list(lst, refs)
    assert sizes.data_ptr() == szs.data_ptr() and sizes.shape == szs.shape
    torch.cuda.synchronize()
    check_rows(mat, szs, refs)
    host = mat.cpu().numpy()
    assert (host[n:] == FILL).all(), "a row past the batch was written"
    assert (host[:, cols:] == FILL).all(), "a column past the required width was written"
    assert szs.cpu().tolist()[n:] == [-1] * EXTRA_ROWS


def test_split_size_returns_views_and_simple_returns_copies(tmp):
    words = [elem(2, n, seed=3) for n in (4097, 7, 4096)]
    refs = [oracle(2, w) for w in words]
    t_in = dev(np.concatenate(words), 2)
    lst, sizes, _ = D.compress_data_split_size(True, t_in, torch.tensor([w.size for w in words], dtype=I32),
                                               False, tmp)
    check_list(lst, refs)
    cols = float_max(2, 4097)
    assert len({a.untyped_storage().data_ptr() for a in lst}) == 1
    assert [a.storage_offset() for a in lst] == [i * cols for i in range(3)]
    simple = D.compress_data_simple(True, [dev(w, 2) for w in words], False)
    check_list(simple, refs)
    assert len({a.untyped_storage().data_ptr() for a in simple}) == 3
    assert all(a.storage_offset() == 0 for a in simple)


# ---------------------------------------------------------------------------
# c. split-size operators against the oracle, per split
# ---------------------------------------------------------------------------
# words.  odd: every split but the first starts off 16 B alignment (the
# three-kernel route); aligned: every split is a multiple of 16 B in all four
# types; single: one split
FLOAT_SPLITS = {"odd": [7, 4095, 1, 4097, 12345], "aligned": [4096, 8, 8192, 64], "single": [70001]}
# bytes: interior splits are multiples of 4, the last one is ragged
BYTE_SPLITS = {"ragged-last": [4096, 4, 12348, 4092, 4097], "single": [70001]}
SPLIT_CASES = [(ft, k) for ft in (1, 2, 3, 4) for k in FLOAT_SPLITS] + [(0, k) for k in BYTE_SPLITS] + \
              [(0, "int32-t_in")]
# (temp_mem, checksum)
COMBOS = [(True, False), (False, True), (True, True), (False, False)]


@pytest.mark.parametrize("ft,kind", SPLIT_CASES, ids=[f"{FT_IDS[f]}-{k}" for f, k in SPLIT_CASES])
def test_split_size_operators(tmp, ft, kind):
    """compress_data_split_size: archive i is the oracle's archive of split
    i.  decompress_data_split_size: the splits land back to back in a
    canaried t_out (one word off 16 B alignment for the odd splits), with
    status and sizes."""
    as_int32 = kind == "int32-t_in"
    splits = BYTE_SPLITS["ragged-last"][:-1] if as_int32 else (FLOAT_SPLITS if ft else BYTE_SPLITS)[kind]
    wb = WORD_BYTES[ft]
    words = elem(ft, sum(splits), seed=4)
    ends = np.cumsum(splits)
    parts = [words[e - s: e] for s, e in zip(splits, ends)]
    t_in = dev(words, ft)
    if as_int32:  # byte mode on a wider dtype: the splits are still bytes
        t_in = t_in.view(torch.int32)
    sp = torch.tensor(splits, dtype=I32)
    for use_tmp, checksum in COMBOS:
        what = f"temp_mem={use_tmp} checksum={checksum}"
        refs = [oracle(ft, p, checksum) for p in parts]
        lst, sizes, used = D.compress_data_split_size(bool(ft), t_in, sp, checksum, tmp if use_tmp else None)
        assert sizes.cpu().tolist() == [r.size for r in refs], what
        check_list(lst, refs)
        assert isinstance(used, int)
        off = (1 if kind == "odd" else 0) * wb if ft else (4 if kind == "ragged-last" else 0)
        cv = Carved([(words.size * wb, off)])
        cv.expect_words(0, words)
        t_out = cv.region(0, torch.int32 if as_int32 else TORCH_OUT[ft])
        st, sz = status_tensors(len(splits))
        D.decompress_data_split_size(bool(ft), lst, t_out, sp, checksum, tmp if use_tmp else None, st, sz)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [1] * len(splits), what
        assert sz.cpu().tolist() == splits, what
        cv.check(what)


# ---------------------------------------------------------------------------
# d. failing members through the full decoder
# ---------------------------------------------------------------------------
def failing_batch(C, ws, ft):
    """[(archive, words, capacity in words, offset in words, status, size)]:
    good members first, last and between the failures."""
    def good(n, seed):
        w = elem(ft, n, seed)
        return w, D.compress_data_simple(bool(ft), [dev(w, ft)], False)[0]
    w0, a0 = good(4097, 5)
    w1, a1 = good(7, 6)
    w2, a2 = good(12345, 7)
    w3, a3 = good(4096, 8)
    # (for the byte codec: a float archive, whose magic differs)
    wrong_type = D.compress_data_simple(True, [dev(elem(2, 4096, 9), 2)], False)[0] if ft == 0 else retyped(a3, ft)
    wrong_pb = compress_one(C, ws, w3, ft, pb=9, clone=True)
    return [
        (a0, w0, 4097, 0, 1, 4097),
        (a3, None, 4095, 0, 0, 4096),       # one word short: the size is still reported
        (a1, w1, 7, 1, 1, 7),
        (wrong_type, None, 4096, 1, 0, 0),
        (wrong_pb, None, 4096, 0, 0, 0),
        (a3, None, 4095, 1, 0, 4096),
        (a2, w2, 12345, 1, 1, 12345),
    ]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("ft", ALL_FT, ids=FT_IDS.get)
def test_failing_members_through_decompress_data(C, ws, tmp, ft, with_status):
    """One batch per format: an output one word short (status 0, size n), an
    archive of another type and one of other prob bits (status 0, size 0)
    between good members.  The good members decode exactly; every failing
    member's destination and all canaries stay untouched."""
    members = failing_batch(C, ws, ft)
    wb = WORD_BYTES[ft]
    cv = Carved([(cap * wb, off * wb) for (_, _, cap, off, _, _) in members])
    outs = [cv.region(i, TORCH_OUT[ft]) for i in range(len(members))]
    for i, (_, w, cap, off, ok, _) in enumerate(members):
        assert outs[i].data_ptr() % 16 == off * wb % 16
        if ok:
            cv.expect_words(i, w)
    archives = [m[0] for m in members]
    if with_status:
        st, sz = status_tensors(len(members))
        D.decompress_data(bool(ft), archives, outs, False, tmp, st, sz)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [m[4] for m in members]
        assert sz.cpu().tolist() == [m[5] for m in members]
    else:
        assert isinstance(D.decompress_data(bool(ft), archives, outs, False, tmp), int)
        torch.cuda.synchronize()
    cv.check(FT_IDS[ft])


@pytest.mark.parametrize("ft", [2, 3], ids=FT_IDS.get)
def test_checksum_mismatch_raises(tmp, ft):
    """One byte of the raw section of an archive written with a checksum is
    changed (no size or offset field: the decode runs as before and yields
    one other word).  Every decompress operator raises with checksum=True;
    without it the batch decodes, that word aside."""
    w, w7 = elem(ft, 4097, seed=19), elem(ft, 7, seed=19)
    a, good = D.compress_data_simple(True, [dev(w, ft), dev(w7, ft)], True)
    bad = a.clone()
    bad[40] ^= 0xFF
    out, out7 = filled(4097, TORCH_OUT[ft]), filled(7, TORCH_OUT[ft])
    for op, args in ((D.decompress_data, (True, [good, bad], [out7, out], True, tmp)),
                     (D.decompress_data_simple, (True, [good, bad], True)),
                     (D.decompress_data_split_size, (True, [bad], out, isplit(4097), True, tmp))):
        with pytest.raises(RuntimeError, match="checksum mismatch"):
            op(*args)
    st, sz = status_tensors(2)
    D.decompress_data(True, [good, bad], [out7, out], False, tmp, st, sz)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [1, 1] and sz.cpu().tolist() == [7, 4097]
    np.testing.assert_array_equal(to_host_words(out7, ft), w7)
    assert int((to_host_words(out, ft) != w).sum()) == 1


# ---------------------------------------------------------------------------
# e. the _simple operators
# ---------------------------------------------------------------------------
# None: no arena; 0 / 15 / 16 / 255: below kSDMAlignment (256), where
# decompress_data_simple allocates no scratch and an arena over a smaller
# tensor is empty; 256: an arena of one allocation unit; 1 << 20: a real one
TEMP_MEM = [None, 0, 15, 16, 255, 256, 1 << 20]


@pytest.mark.parametrize("tm", TEMP_MEM, ids=[f"tm{t}" for t in TEMP_MEM])
@pytest.mark.parametrize("ft", ALL_FT, ids=FT_IDS.get)
def test_simple_operators(ft, tm):
    checksum = tm in (None, 16, 256)
    words = [elem(ft, n, seed=11) for n in (1, 4097, 12345)]
    refs = [oracle(ft, w, checksum) for w in words]
    cts = D.compress_data_simple(bool(ft), [dev(w, ft) for w in words], checksum, tm)
    check_list(cts, refs)
    dts = D.decompress_data_simple(bool(ft), cts, checksum, tm)
    torch.cuda.synchronize()
    assert len(dts) == len(words)
    for w, t in zip(words, dts):
        assert t.dtype == TORCH_OUT[ft] and t.dim() == 1 and t.numel() == w.size
        np.testing.assert_array_equal(to_host_words(t, ft), w)


def test_simple_rejects_archives_of_two_float_types():
    a = D.compress_data_simple(True, [dev(elem(2, 4097, 12), 2)], False)
    b = D.compress_data_simple(True, [dev(elem(1, 4097, 12), 1)], False)
    with pytest.raises(RuntimeError, match="same float type"):
        D.decompress_data_simple(True, a + b, False)
    with pytest.raises(RuntimeError, match="same float type"):
        D.decompress_data_simple(True, b + a + b, False, 1 << 20)


# ---------------------------------------------------------------------------
# f. input forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ft", [0, 2, 3], ids=FT_IDS.get)
def test_input_forms(tmp, ft):
    """One list of a 2-d and a 3-d contiguous tensor (numel() is the
    element), a view that starts one word after a 16 B boundary, and an empty
    tensor between non-empty ones."""
    wb = WORD_BYTES[ft]
    w2, w3, wv, we, w1 = (elem(ft, n, seed=13 + i) for i, n in enumerate((12345, 12345, 4097, 0, 7)))
    x2 = dev(w2, ft).view(3, 4115)
    x3 = dev(w3, ft).view(5, 3, 823)
    xv = dev(np.concatenate([wv[:1], wv]), ft)[1:]
    assert xv.data_ptr() % 16 == wb and xv.is_contiguous()
    xe = torch.empty([0], dtype=TORCH_OUT[ft], device=DEV)
    ts = [x2, x3, xv, xe, dev(w1, ft)]
    words = [w2, w3, wv, we, w1]
    refs = [oracle(ft, w) for w in words]
    comp, sizes, _ = D.compress_data(bool(ft), ts, False, tmp)
    sizes_h = check_rows(comp, sizes, refs)
    check_list(D.compress_data_simple(bool(ft), ts, False), refs)
    # decode into outputs of the same shapes
    cv = Carved([(w.size * wb, (i % 2) * wb) for i, w in enumerate(words)])
    outs = [cv.region(i, TORCH_OUT[ft]).view(t.shape) for i, t in enumerate(ts)]
    for i, w in enumerate(words):
        cv.expect_words(i, w)
    st, sz = status_tensors(len(ts))
    D.decompress_data(bool(ft), [comp[i, : sizes_h[i]] for i in range(len(ts))], outs, False, tmp, st, sz)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [1] * len(ts)
    assert sz.cpu().tolist() == [w.size for w in words]
    cv.check(FT_IDS[ft])


@pytest.mark.parametrize("ft", [0, 2], ids=FT_IDS.get)
def test_side_stream(tmp, ft):
    """The operators run on the current stream: inputs produced on a side
    stream are compressed and decompressed there without a synchronize in
    between, and compared once the side stream has finished.  Twenty passes
    over a 256 MiB buffer are queued on the side stream ahead of the inputs'
    producers (a few milliseconds of work, enqueued in a fraction of one), so
    an operator that launched on another stream would read the inputs before
    they exist."""
    words = [elem(ft, n, seed=17) for n in (70001, 4097, 7)]
    refs = [oracle(ft, w) for w in words]
    pinned = [torch.from_numpy(w.view(NP_SIGNED[ft]).copy()).pin_memory() for w in words]
    key = 0x5A
    ahead = torch.zeros([256 << 20], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            ahead.add_(1)
        ts = []
        for p in pinned:
            raw = p.to(DEV, non_blocking=True)
            ts.append(((raw ^ key) ^ key).view(TORCH_OUT[ft]))
        comp, sizes, _ = D.compress_data(bool(ft), ts, False, tmp)
        rows = [comp[i, : r.size] for i, r in enumerate(refs)]
        outs = [torch.empty_like(t) for t in ts]
        st, sz = status_tensors(len(ts))
        D.decompress_data(bool(ft), rows, outs, False, tmp, st, sz)
    side.synchronize()
    check_rows(comp, sizes, refs)
    assert st.cpu().tolist() == [1] * len(ts)
    for w, o in zip(words, outs):
        np.testing.assert_array_equal(to_host_words(o, ft), w)


# ---------------------------------------------------------------------------
# g. size operators
# ---------------------------------------------------------------------------
SIZES = [0, 1, 7, 4095, 4096, 4097, 12345, 70001]


def test_size_operators_equal_the_codec_bounds(C):
    for n in SIZES:
        assert D.max_any_compressed_size(n) == C.max_compressed_size(n)
        for ft in (1, 2, 3, 4):
            assert float_max(ft, n) == C.max_float_compressed_size(ft, n)
    for ft in ALL_FT:
        ts = [torch.empty(n, dtype=TORCH_OUT[ft], device=DEV) for n in (7, 12345, 4097)]
        if ft:
            assert tuple(D.max_float_compressed_output_size(ts)) == (3, C.max_float_compressed_size(ft, 12345))
        assert tuple(D.max_any_compressed_output_size(ts)) == (3, C.max_compressed_size(12345 * WORD_BYTES[ft]))


def test_size_bounds_cover_max_rate_archives():
    """The bounds are at least the oracle's archive sizes of the rate-extreme
    elements (blocks at the maximum 4096 * 10 / 16 words)."""
    datas = byte_members()
    for d, ref in zip(datas, ref_archives(0, "members", datas, 10)):
        assert D.max_any_compressed_size(d.size) >= ref.size
        assert D.max_any_compressed_output_size([torch.empty(d.size, dtype=torch.uint8)])[1] >= ref.size
    for ft in (1, 2, 3, 4):
        words = float_members(ft)
        for w, ref in zip(words, ref_archives(ft, "members", words, 10)):
            assert float_max(ft, w.size) >= ref.size
            assert D.max_float_compressed_output_size([torch.empty(w.size, dtype=TORCH_OUT[ft])])[1] >= ref.size


@pytest.mark.parametrize("size", [-1, 1 << 32, 1 << 40])
def test_size_operators_reject_sizes_outside_u32(size):
    with pytest.raises(RuntimeError, match="size out of range"):
        D.max_any_compressed_size(size)
    with pytest.raises(RuntimeError, match="size out of range"):
        D.max_float_compressed_size(torch.empty(0, dtype=torch.float16, device=DEV), size)


def test_float_size_operator_rejects_an_integer_dtype():
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
        with pytest.raises(RuntimeError, match="unsupported dtype"):
            D.max_float_compressed_size(torch.empty(0, dtype=dt, device=DEV), 4096)


# ---------------------------------------------------------------------------
# h. rejections
# ---------------------------------------------------------------------------
def filled(n, dtype):
    """A device tensor of n elements whose every byte is 0xA5."""
    return torch.full([n * dtype.itemsize], FILL, dtype=torch.uint8, device=DEV).view(dtype)


def isplit(*v, dtype=I32):
    return torch.tensor(list(v), dtype=dtype)


@pytest.fixture(scope="module")
def K(tmp):
    """Valid arguments that the rejection cases bend in one place each."""
    k = types.SimpleNamespace(tmp=tmp)
    k.bf = dev(elem(2, 4097, 20), 2)
    k.h = dev(elem(1, 4097, 20), 1)
    k.u8 = dev(elem(0, 4096, 20), 0)
    k.i32 = dev(elem(3, 1024, 20), 3).view(torch.int32)
    k.bf_wide = dev(elem(2, 2 * 4097, 21), 2)
    k.f32a = dev(elem(3, 100, 22), 3)
    k.f32b = dev(elem(3, 100, 23), 3)
    k.u1000 = dev(elem(0, 1000, 24), 0)
    k.i1100 = dev(elem(3, 1100, 24), 3).view(torch.int32)
    k.a_bf = D.compress_data_simple(True, [k.bf], False)[0]
    k.a_u8 = D.compress_data_simple(False, [k.u8], False)[0]
    k.a_f32a, k.a_f32b = D.compress_data_simple(True, [k.f32a, k.f32b], False)
    # the bf16 archive one byte after a 16 B boundary, and every other byte of a buffer
    room = torch.zeros([k.a_bf.numel() + 16], dtype=torch.uint8, device=DEV)
    assert room.data_ptr() % 16 == 0
    k.a_bf_off1 = room[1: 1 + k.a_bf.numel()]
    k.a_bf_off1.copy_(k.a_bf)
    k.a_bf_strided = torch.zeros([2 * k.a_bf.numel()], dtype=torch.uint8, device=DEV)[::2]
    k.cols_bf = D.max_float_compressed_output_size([k.bf])[1]
    k.cols_u8 = D.max_any_compressed_output_size([k.u8])[1]
    k.o_bf = filled(4097, torch.bfloat16)
    k.o_bf_wide = filled(2 * 4097, torch.bfloat16)
    k.o_i16 = filled(4097, torch.int16)
    k.o_u8 = filled(4096, torch.uint8)
    k.o_f32 = filled(100, torch.float32)
    k.o_bf100 = filled(100, torch.bfloat16)
    k.o_bf_8193 = filled(8193, torch.bfloat16)
    k.o_u8_8191 = filled(8191, torch.uint8)
    k.cpu_tmp = torch.zeros([1 << 20], dtype=torch.uint8)
    torch.cuda.synchronize()
    return k


def mat(rows, cols, dtype=torch.uint8):
    return filled(rows * cols, dtype).view(rows, cols)


def vec(n, dtype):
    return filled(n, dtype)


# name: (k -> (operator, arguments), the check's message)
REJECTIONS = {
    "empty-list": (lambda k: (D.compress_data, (True, [])), "ts_in must not be empty"),
    "empty-list-decompress": (lambda k: (D.decompress_data, (True, [], [])), "ts_in must not be empty"),
    "cpu-input": (lambda k: (D.compress_data, (True, [k.bf.cpu()])), "inputs must be GPU tensors"),
    "cpu-input-second": (lambda k: (D.compress_data, (True, [k.bf, k.bf.cpu()])), "inputs must be GPU tensors"),
    "cpu-t_in": (lambda k: (D.compress_data_split_size, (True, k.bf.cpu(), isplit(4097))),
                 "t_in must be a contiguous GPU tensor"),
    "cpu-ts_out": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf.cpu()])), "ts_out must be contiguous GPU"),
    "cpu-archive-second": (lambda k: (D.decompress_data, (True, [k.a_bf, k.a_bf.cpu()], [k.o_bf, k.o_bf])),
                           "compressed inputs must be contiguous GPU"),
    "non-contiguous-input": (lambda k: (D.compress_data, (True, [k.bf_wide[::2]])), "inputs must be contiguous"),
    "non-contiguous-t_in": (lambda k: (D.compress_data_split_size, (True, k.bf_wide[::2], isplit(4097))),
                            "t_in must be a contiguous GPU tensor"),
    "non-contiguous-ts_out": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf_wide[::2]])),
                              "ts_out must be contiguous GPU"),
    "non-contiguous-t_out": (lambda k: (D.decompress_data_split_size,
                                        (True, [k.a_bf], k.o_bf_wide[::2], isplit(4097))),
                             "t_out must be a contiguous GPU tensor"),
    "non-contiguous-archive": (lambda k: (D.decompress_data, (True, [k.a_bf_strided], [k.o_bf])),
                               "compressed inputs must be contiguous GPU"),
    "integer-as-float": (lambda k: (D.compress_data, (True, [k.i32])), "unsupported dtype"),
    "integer-as-float-simple": (lambda k: (D.compress_data_simple, (True, [k.u8])), "unsupported dtype"),
    "integer-as-float-split": (lambda k: (D.compress_data_split_size, (True, k.i32, isplit(1024))),
                               "unsupported dtype"),
    "integer-ts_out-as-float": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_i16])),
                                "float outputs must be float16"),
    "integer-t_out-as-float": (lambda k: (D.decompress_data_split_size, (True, [k.a_bf], k.o_i16, isplit(4097))),
                               "float outputs must be float16"),
    "mixed-float-dtypes": (lambda k: (D.compress_data, (True, [k.bf, k.h])), "float inputs must share a dtype"),
    "mixed-float-dtypes-simple": (lambda k: (D.compress_data_simple, (True, [k.h, k.bf])),
                                  "float inputs must share a dtype"),
    "temp_mem-cpu-compress": (lambda k: (D.compress_data, (True, [k.bf], False, k.cpu_tmp)),
                              "temp_mem must be a GPU tensor"),
    "temp_mem-cpu-split": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4097), False, k.cpu_tmp)),
                           "temp_mem must be a GPU tensor"),
    "temp_mem-cpu-decompress": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf], False, k.cpu_tmp)),
                                "temp_mem must be a GPU tensor"),
    "temp_mem-cpu-decompress-split": (lambda k: (D.decompress_data_split_size,
                                                 (True, [k.a_bf], k.o_bf, isplit(4097), False, k.cpu_tmp)),
                                      "temp_mem must be a GPU tensor"),
    "temp_mem-non-contiguous": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp[: 1 << 20][::2])),
                                "temp_mem must be contiguous"),
    "out_compressed-dtype": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp, mat(1, k.cols_bf, torch.int8))),
                             "out_compressed must be a contiguous uint8 GPU tensor"),
    "out_compressed-cpu": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp,
                                                        torch.zeros([1, k.cols_bf], dtype=torch.uint8))),
                           "out_compressed must be a contiguous uint8 GPU tensor"),
    "out_compressed-1d": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp, vec(k.cols_bf, torch.uint8))),
                          "out_compressed must be 2-d"),
    "out_compressed-row-short": (lambda k: (D.compress_data, (True, [k.bf, k.bf], False, k.tmp, mat(1, k.cols_bf))),
                                 "out_compressed must be 2-d, at least"),
    "out_compressed-column-short": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp,
                                                                 mat(1, k.cols_bf - 1))),
                                    "out_compressed must be 2-d, at least"),
    "out_compressed-column-short-bytes": (lambda k: (D.compress_data, (False, [k.u8], False, k.tmp,
                                                                       mat(1, k.cols_u8 - 1))),
                                          "out_compressed must be 2-d, at least"),
    "out_compressed-non-contiguous": (lambda k: (D.compress_data, (True, [k.bf, k.bf], False, k.tmp,
                                                                   mat(2, 2 * k.cols_bf)[:, : k.cols_bf])),
                                      "out_compressed must be a contiguous uint8 GPU tensor"),
    "out_compressed-row-short-split": (lambda k: (D.compress_data_split_size,
                                                  (True, k.bf, isplit(4096, 1), False, k.tmp, mat(1, k.cols_bf))),
                                       "out_compressed must be 2-d, at least"),
    "out_compressed-column-short-split": (lambda k: (D.compress_data_split_size,
                                                     (True, k.bf, isplit(4097), False, k.tmp,
                                                      mat(1, k.cols_bf - 1))),
                                          "out_compressed must be 2-d, at least"),
    # (the next five come from the codec library's own checks, before any launch)
    "out_compressed-width-not-16": (lambda k: (D.compress_data, (True, [k.bf, k.bf], False, k.tmp,
                                                                 mat(2, k.cols_bf + 8))),
                                    "must be 16-byte aligned"),
    "out_compressed-width-not-16-split": (lambda k: (D.compress_data_split_size,
                                                     (True, k.bf, isplit(4096, 1), False, k.tmp,
                                                      mat(2, k.cols_bf + 8))),
                                          "outStride must be a multiple of 16"),
    "out_compressed-base-not-16": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp,
                                                                vec(k.cols_bf + 16, torch.uint8)[8: 8 + k.cols_bf]
                                                                .view(1, k.cols_bf))),
                                   "must be 16-byte aligned"),
    "byte-t_out-unaligned": (lambda k: (D.decompress_data_split_size,
                                        (False, [k.a_u8], k.o_u8_8191[1: 4097], isplit(4096))),
                             "out_dev must be 4-byte aligned"),
    "byte-t_out-interior-split": (lambda k: (D.decompress_data_split_size,
                                             (False, [k.a_u8, k.a_u8], k.o_u8_8191, isplit(4094, 4096))),
                                  "interior split sizes must be multiples of 4"),
    "out_compressed_bytes-dtype": (lambda k: (D.compress_data, (True, [k.bf], False, k.tmp, None,
                                                                vec(1, torch.int64))),
                                   "out_compressed_bytes must be a 1-d int32 GPU tensor"),
    "out_compressed_bytes-short": (lambda k: (D.compress_data, (True, [k.bf, k.bf], False, k.tmp, None,
                                                                vec(1, torch.int32))),
                                   "out_compressed_bytes must be contiguous"),
    "out_compressed_bytes-short-split": (lambda k: (D.compress_data_split_size,
                                                    (True, k.bf, isplit(4096, 1), False, k.tmp, None,
                                                     vec(1, torch.int32))),
                                         "out_compressed_bytes must be contiguous"),
    "splits-on-gpu": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4097).to(DEV))),
                      "t_in_split_sizes must be a contiguous CPU int32"),
    "splits-int64": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4097, dtype=torch.int64))),
                     "t_in_split_sizes must be a contiguous CPU int32"),
    "splits-zero": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4000, 0, 97))),
                    "split sizes must be > 0"),
    "splits-negative": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4000, -1))),
                        "split sizes must be > 0"),
    "out-splits-on-gpu": (lambda k: (D.decompress_data_split_size, (True, [k.a_bf], k.o_bf, isplit(4097).to(DEV))),
                          "t_out_split_sizes must be a contiguous CPU int32"),
    "out-splits-int64": (lambda k: (D.decompress_data_split_size,
                                    (True, [k.a_bf], k.o_bf, isplit(4097, dtype=torch.int64))),
                         "t_out_split_sizes must be a contiguous CPU int32"),
    "out-splits-zero": (lambda k: (D.decompress_data_split_size, (True, [k.a_bf, k.a_bf], k.o_bf, isplit(4097, 0))),
                        "split sizes must be > 0"),
    "out-splits-negative": (lambda k: (D.decompress_data_split_size,
                                       (True, [k.a_bf, k.a_bf], k.o_bf, isplit(-4097, 4097))),
                            "split sizes must be > 0"),
    "out-splits-count": (lambda k: (D.decompress_data_split_size, (True, [k.a_bf], k.o_bf, isplit(4000, 97))),
                         "one split size per compressed input"),
    "byte-t_in-unaligned": (lambda k: (D.compress_data_split_size, (False, k.u8[1:], isplit(4095))),
                            "start pointer is not aligned"),
    "byte-interior-split": (lambda k: (D.compress_data_split_size, (False, k.u8, isplit(6, 10))),
                            "size of an interior split"),
    "length-mismatch": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf, k.o_bf])),
                        "ts_in and ts_out must have the same"),
    "length-mismatch-range": (lambda k: (D.decompress_data_range,
                                         (True, [k.a_bf, k.a_bf], [k.o_bf], torch.zeros(2, dtype=torch.int64))),
                              "ts_in and ts_out must have the same"),
    "archive-not-uint8": (lambda k: (D.decompress_data, (True, [k.a_bf.view(torch.int8)], [k.o_bf])),
                          "compressed inputs must be uint8"),
    "archive-not-uint8-simple": (lambda k: (D.decompress_data_simple, (True, [k.a_bf.view(torch.int8)])),
                                 "compressed inputs must be uint8"),
    "archive-not-uint8-split": (lambda k: (D.decompress_data_split_size,
                                           (True, [k.a_bf.view(torch.int8)], k.o_bf, isplit(4097))),
                                "compressed inputs must be uint8"),
    "out_status-dtype": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf], False, k.tmp,
                                                        vec(1, torch.int32))),
                         "out_status must be a contiguous uint8 GPU tensor"),
    "out_status-length": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf], False, k.tmp,
                                                         vec(2, torch.uint8))),
                          "out_status must have 1 entries"),
    "out_status-length-split": (lambda k: (D.decompress_data_split_size,
                                           (True, [k.a_bf], k.o_bf, isplit(4097), False, k.tmp, vec(2, torch.uint8))),
                                "out_status must have 1 entries"),
    "out_words-dtype": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf], False, k.tmp, None,
                                                       vec(1, torch.int64))),
                        "out_decompressed_words must be a contiguous int32 GPU tensor"),
    "out_words-length": (lambda k: (D.decompress_data, (True, [k.a_bf], [k.o_bf], False, k.tmp, None,
                                                        vec(3, torch.int32))),
                         "out_decompressed_words must have 1 entries"),
    # the argument guards
    "guard-byte-row-capacity": (lambda k: (D.compress_data,
                                           (False, [k.u1000, k.i1100], False, k.tmp,
                                            mat(2, D.max_any_compressed_size(1000)))),
                                "out_compressed must be 2-d, at least"),
    "guard-split-sum-t_in-float": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4096, 2))),
                                   "split sizes sum to 4098 words but t_in holds 4097"),
    "guard-split-sum-t_in-bytes": (lambda k: (D.compress_data_split_size, (False, k.u8, isplit(4092, 5))),
                                   "split sizes sum to 4097 bytes but t_in holds 4096"),
    "guard-split-sum-t_in-bytes-int32": (lambda k: (D.compress_data_split_size, (False, k.i32, isplit(4096, 1))),
                                         "split sizes sum to 4097 bytes but t_in holds 4096"),
    "guard-split-sum-t_in-single": (lambda k: (D.compress_data_split_size, (True, k.bf, isplit(4098))),
                                    "split sizes sum to 4098 words but t_in holds 4097"),
    "guard-split-sum-t_out-float": (lambda k: (D.decompress_data_split_size,
                                               (True, [k.a_bf, k.a_bf], k.o_bf_8193, isplit(4097, 4097))),
                                    "split sizes sum to 8194 words but t_out holds 8193"),
    "guard-split-sum-t_out-bytes": (lambda k: (D.decompress_data_split_size,
                                               (False, [k.a_u8, k.a_u8], k.o_u8_8191, isplit(4096, 4096))),
                                    "split sizes sum to 8192 bytes but t_out holds 8191"),
    "guard-ts_out-two-dtypes": (lambda k: (D.decompress_data, (True, [k.a_f32a, k.a_f32b], [k.o_f32, k.o_bf100])),
                                "must share a dtype"),
    "guard-archive-unaligned": (lambda k: (D.decompress_data, (True, [k.a_bf_off1], [k.o_bf])),
                                "compressed inputs must be 4-byte aligned"),
    "guard-archive-unaligned-simple": (lambda k: (D.decompress_data_simple, (True, [k.a_bf, k.a_bf_off1])),
                                       "compressed inputs must be 4-byte aligned"),
    "guard-archive-unaligned-split": (lambda k: (D.decompress_data_split_size,
                                                 (True, [k.a_bf_off1], k.o_bf, isplit(4097))),
                                      "compressed inputs must be 4-byte aligned"),
    "guard-archive-below-header": (lambda k: (D.decompress_data, (True, [k.a_bf[:31]], [k.o_bf])),
                                   "at least the 32-byte archive header"),
    "guard-archive-empty-simple": (lambda k: (D.decompress_data_simple, (False, [k.a_u8, k.a_u8[:0]])),
                                   "at least the 32-byte archive header"),
    "guard-archive-below-header-split": (lambda k: (D.decompress_data_split_size,
                                                    (False, [k.a_u8[:16]], k.o_u8, isplit(4096))),
                                         "at least the 32-byte archive header"),
}


def tensors_in(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            yield a
        elif isinstance(a, (list, tuple)):
            yield from tensors_in(a)


def raw_bytes(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).clone() if t.numel() else None


@pytest.mark.parametrize("case", REJECTIONS)
def test_rejections(K, case):
    """A RuntimeError from the named check; the caller's tensors, temp_mem
    aside, are as they were."""
    make, message = REJECTIONS[case]
    op, args = make(K)
    held = [t for t in tensors_in(args) if t.numel() <= (1 << 20)]
    before = [raw_bytes(t) for t in held]
    with pytest.raises(RuntimeError) as e:
        op(*args)
    assert message in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for i, (t, b) in enumerate(zip(held, before)):
        if b is not None:
            assert torch.equal(raw_bytes(t), b), f"tensor argument {i} changed"
