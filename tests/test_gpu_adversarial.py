"""GPU parity on adversarial content (generators: tests/util.py, pinned by
tests/test_adversarial_inputs.py).

Rate extremes: elements whose blocks encode to the maximum 4096 * pb / 16
words (every symbol at pdf 1, all 32 lanes emitting on the same steps) beside
blocks that emit almost nothing, in the same wave's block pair, in another
workgroup and as a partial tail -- through every compression route, decoded
from aligned and unaligned archives into aligned and unaligned outputs, by
range decode, as float symbol streams and as a sparse element's nonzero
list.  Hard histograms: every branch of the table normalisation (many
decrement rounds with a shrinking group, a round cut inside equal pdfs, the
bump of absent symbol ids, float32 quotients that are not the exact floor,
counts above 2^24) through each of its callers.

Every archive is compared with the oracle's, the reported size first and then
the bytes; every decode is bit-exact."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, N, Cache, to_dev, workspace_fixture  # noqa: F401
from tests.util import (BLOCK, FT_IDS, LARGE_FAMILIES, NP_W, NP_WORD, STD_BLOCKS, STD_RARE_C1, TORCH_FLOAT, TORCH_WORD,
                        WORD_BYTES, bytes_from_histogram, exp_bytes, hard_histograms, rate_extreme_bytes,
                        small_extreme_bytes, std_extreme_bytes, std_mirror_bytes, words_from_symbols)

pytestmark = pytest.mark.gpu

PBS = [9, 10, 11]
CANARY = 16
FILL = 0xA5
N_STD = STD_BLOCKS * BLOCK + 1000

ws = workspace_fixture(512 << 20)
# inputs and oracle archives: computed once, shared, left unchanged
_CACHE = Cache()


def byte_members():
    return _CACHE.get("bytes", lambda: [std_extreme_bytes(), small_extreme_bytes(), std_mirror_bytes(),
                                    exp_bytes(33, lam=10.0, seed=3)])


def float_members(ft):
    def make():
        c1 = std_extreme_bytes(STD_RARE_C1) if ft == 4 else None
        c1s = rate_extreme_bytes(5, [3], 0) if ft == 4 else None
        return [words_from_symbols(ft, std_extreme_bytes(), c1, seed=ft),
                words_from_symbols(ft, small_extreme_bytes(), c1s, seed=10 + ft)]
    return _CACHE.get(("words", ft), make)


def ref_archives(ft, key, words, pb, checksum=False):
    """The oracle's archives of a member list (ft 0: the byte codec)."""
    def make():
        if ft == 0:
            return [O.ans_encode(w, pb, checksum) for w in words]
        return [O.float_compress(w, ft, pb, checksum) for w in words]
    return _CACHE.get(("ref", ft, key, pb, checksum), make)


def encode_bytes(C, N, ws, ts, pb, checksum, hist=None):
    """ans_encode_batch_pointer, with an optional [nb, 256] histogram."""
    nb = len(ts)
    cols = C.max_compressed_size(max(t.numel() for t in ts))
    out = torch.empty([nb, cols], dtype=torch.uint8, device=DEV)
    sizes = torch.empty([nb], dtype=torch.int32, device=DEV)
    rc = N.lib().dietgpu_ans_encode_batch_pointer(
        ws.h, pb, int(checksum), nb, N.ptr_array([t.data_ptr() for t in ts]),
        N.u32_array([t.numel() for t in ts]), hist.data_ptr() if hist is not None else None,
        N.ptr_array([out.data_ptr() + i * cols for i in range(nb)]), sizes.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    N.check(rc)
    return out, sizes


def check_archives(C, out, sizes, refs, section=None):
    """Sizes, then (a readable failure first) one section, then all bytes."""
    assert C.device_error_count(reset=True) == 0
    sizes_h = sizes.cpu().tolist()
    host = out.cpu().numpy()
    for i, ref in enumerate(refs):
        assert sizes_h[i] == ref.size, (i, sizes_h[i], ref.size)
    for i, ref in enumerate(refs):
        if section is not None:
            name, lo, hi, dt = section(i)
            np.testing.assert_array_equal(host[i, lo:hi].view(dt), ref[lo:hi].view(dt),
                                          err_msg=f"member {i}: {name}")
        np.testing.assert_array_equal(host[i, : ref.size], ref, err_msg=f"member {i}")
    return sizes_h


def decode_three_ways(C, ws, ft, out, sizes_h, words, pb, checksum=False):
    """Bit-exact decode from exactly-sized clones, from copies 8 bytes off
    16 B alignment (scalar loads of the compressed words) and into outputs one
    word off alignment; the bytes around every output stay untouched."""
    nb = len(words)
    wb = WORD_BYTES[ft]
    for arch_off, out_off in ((0, 0), (8, 0), (0, 1)):
        arch = []
        for i in range(nb):
            buf = torch.empty(sizes_h[i] + 16, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            a = buf[arch_off: arch_off + sizes_h[i]]
            a.copy_(out[i, : sizes_h[i]])
            arch.append(a)
        bufs = [torch.full([(w.size + 2 * CANARY) * wb], FILL, dtype=torch.uint8, device=DEV).view(TORCH_WORD[ft])
                for w in words]
        outs = [b[CANARY + out_off: CANARY + out_off + w.size] for b, w in zip(bufs, words)]
        assert all(o.data_ptr() % 16 == out_off * wb for o in outs)
        if ft == 0:
            ok, sz = C.ans_decode_pointer(arch, outs, prob_bits=pb, checksum=checksum, ws=ws)
        else:
            ok, sz = C.float_decompress_pointer(arch, outs, ft=ft, prob_bits=pb, checksum=checksum, ws=ws)
        assert ok.cpu().tolist() == [1] * nb, (arch_off, out_off)
        assert sz.cpu().tolist() == [w.size for w in words]
        for i, (w, b) in enumerate(zip(words, bufs)):
            expect = np.full((w.size + 2 * CANARY) * wb, FILL, dtype=np.uint8).view(NP_W[ft]).copy()
            expect[CANARY + out_off: CANARY + out_off + w.size] = w
            bad = np.flatnonzero(b.cpu().numpy().view(NP_W[ft]) != expect)
            assert bad.size == 0, (f"member {i}, archive offset {arch_off}, output offset {out_off}: "
                                   f"{bad.size} words differ, first at {bad[0] - CANARY - out_off}")


# ---------------------------------------------------------------------------
# rate extremes: bytes
# ---------------------------------------------------------------------------

BYTE_ROUTES = ["single-pass", "single-pass-checksum", "three-kernel-prologue", "three-kernel-checksum",
               "user-histogram", "input-offset-1"]


@pytest.mark.parametrize("pb", PBS)
@pytest.mark.parametrize("route", BYTE_ROUTES)
def test_rate_extreme_bytes(C, N, ws, route, pb):
    """The standard element, the 5-block element, the uniform / constant mirror
    and a 33-byte element as one batch through each compression route:
    k_pcompress; k_hist -> k_encode with the prologue normalisation; with a
    checksum k_hist -> k_histReduce (the standard element is 65 histogram
    chunks, more than the 64 rows one normalisation sums), which normalises
    in its last workgroup; with the caller's histogram (k_normalize); and
    from inputs one byte off alignment."""
    datas = byte_members()
    checksum = route.endswith("checksum")
    refs = ref_archives(0, "members", datas, pb, checksum)
    ts = [to_dev(d, 0, offset=1 if route == "input-offset-1" else 0) for d in datas]
    hist = None
    if route == "user-histogram":
        hist = torch.from_numpy(np.stack([O.histogram(d) for d in datas]).astype(np.int32)).to(DEV)
    path = "single-pass" if route.startswith("single-pass") else "auto" if route == "input-offset-1" \
        else "three-kernel"
    with C.compress_path(path):
        out, sizes = encode_bytes(C, N, ws, ts, pb, checksum, hist)
    sizes_h = check_archives(C, out, sizes, refs)
    decode_three_ways(C, ws, 0, out, sizes_h, datas, pb, checksum)


def run_ranges(C, ws, ft, arch, words, ranges, pb):
    """One batched range decode of (first, count) ranges of one archive, each
    at destination offsets of 0 and 1 words from a 16 B boundary, 16 canary
    words on each side; the whole buffer is compared."""
    wb = WORD_BYTES[ft]
    per16 = 16 // wb
    members = [(f, c, off) for f, c in ranges for off in (0, 1)]
    starts, cur = [], 0
    for (_, c, off) in members:
        st = -(-(cur + CANARY) // per16) * per16 + off
        starts.append(st)
        cur = st + c + CANARY
    total = cur + per16
    buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(TORCH_WORD[ft])
    assert buf.data_ptr() % 16 == 0
    expect = np.full(total * wb, FILL, dtype=np.uint8).view(NP_W[ft]).copy()
    outs = []
    for (f, c, _), st in zip(members, starts):
        outs.append(buf[st: st + c] if ft == 0 else buf[st: st + c].view(TORCH_FLOAT[ft]))
        expect[st: st + c] = words[f: f + c]
    firsts, counts = [m[0] for m in members], [m[1] for m in members]
    if ft == 0:
        _, ok, sz = C.ans_decode_range([arch] * len(members), firsts, counts, outs, prob_bits=pb, ws=ws)
    else:
        _, ok, sz = C.float_decompress_range([arch] * len(members), firsts, counts, outs,
                                             dtype=TORCH_FLOAT[ft], prob_bits=pb, ws=ws)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1] * len(members)
    assert sz.cpu().tolist() == counts
    bad = np.flatnonzero(buf.cpu().numpy().view(NP_W[ft]) != expect)
    assert bad.size == 0, f"{bad.size} words differ, first at buffer word {bad[0]} (member starts {starts})"


@pytest.mark.parametrize("pb", PBS)
def test_rate_extreme_byte_ranges(C, ws, pb):
    """Range decode of the standard element: ranges that end and start inside
    a pair of maximum-rate blocks, one in the middle of a rare block beside a
    quiet one, and the end of the rare tail block."""
    d = byte_members()[0]
    ref = ref_archives(0, "members", byte_members(), pb)[0]
    out, sizes = C.ans_encode_pointer([to_dev(d, 0)], prob_bits=pb, ws=ws)
    check_archives(C, out, sizes, [ref])
    arch = out[0, : ref.size].clone()
    run_ranges(C, ws, 0, arch, d, [(22 * BLOCK - 300, 300), (20 * BLOCK, 300), (6 * BLOCK + 2000, 64),
                                   (N_STD - 300, 300)], pb)


# ---------------------------------------------------------------------------
# rate extremes: float symbol streams
# ---------------------------------------------------------------------------

FLOAT_CASES = [(1, "three-kernel"), (2, "three-kernel"), (3, "three-kernel"), (4, "three-kernel"),
               (1, "single-pass"), (2, "single-pass"), (3, "single-pass")]


@pytest.mark.parametrize("pb", PBS)
@pytest.mark.parametrize("ft,path", FLOAT_CASES, ids=[f"{FT_IDS[f]}-{p}" for f, p in FLOAT_CASES])
def test_rate_extreme_floats(C, ws, ft, path, pb):
    """Float words whose symbol streams are the rate-extreme layouts (fp64:
    the two streams rare in different blocks; its archive goes through
    k_coalesce).  bf16 and fp64 also decode a range over rare blocks."""
    words = float_members(ft)
    refs = ref_archives(ft, "members", words, pb)
    ts = [to_dev(w, ft) for w in words]
    with C.compress_path(path):
        out, sizes = C.float_compress_pointer(ts, ft=ft, prob_bits=pb, ws=ws)
    sizes_h = check_archives(C, out, sizes, refs)
    decode_three_ways(C, ws, ft, out, sizes_h, words, pb)
    if ft in (2, 4) and path == "three-kernel":
        arch = out[0, : sizes_h[0]].clone()
        # bf16: quiet block 19 into the rare pair 20, 21; fp64: blocks 6 .. 9,
        # where first one stream is rare, then the other, then the first
        rng = (20 * BLOCK - 10, BLOCK + 300) if ft == 2 else (6 * BLOCK + 4000, 3 * BLOCK + 200)
        run_ranges(C, ws, ft, arch, words[0], [rng], pb)


def sparse_words(ft):
    """90 % zeros; the nonzero list, in order, is the standard rate-extreme
    layout (263,144 words, a length only the device knows)."""
    def make():
        nz = words_from_symbols(ft, std_extreme_bytes(), seed=20 + ft, nonzero=True)
        rng = np.random.default_rng(30 + ft)
        n = 10 * nz.size
        w = np.zeros(n, dtype=NP_WORD[ft])
        # (the last two words stay zero: no n - 2 quirk of the reference)
        w[np.sort(rng.choice(n - 2, nz.size, replace=False))] = nz
        return w
    return _CACHE.get(("sparse", ft), make)


@pytest.mark.parametrize("pb", PBS)
@pytest.mark.parametrize("ft", [2, 3], ids=FT_IDS.get)
def test_rate_extreme_sparse(C, ws, ft, pb):
    w = sparse_words(ft)
    assert int((w != 0).sum()) == N_STD
    ref = _CACHE.get(("sparse-ref", ft, pb), lambda: O.sparse_compress(w, ft, pb))
    t = to_dev(w, ft)
    out, sizes = C.sparse_compress([t], ft=ft, prob_bits=pb, ws=ws)
    sizes_h = check_archives(C, out, sizes, [ref])
    dec = torch.empty(w.size, dtype=TORCH_WORD[ft], device=DEV)
    ok, sz = C.sparse_decompress([out[0, : sizes_h[0]].clone()], [dec], ft=ft, prob_bits=pb, ws=ws)
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [w.size]
    np.testing.assert_array_equal(dec.cpu().numpy().view(NP_WORD[ft]), w)


# ---------------------------------------------------------------------------
# normalisation through each of its callers
# ---------------------------------------------------------------------------

def family_bytes():
    def make():
        fams = hard_histograms(0)
        names = [n for n in fams if n not in LARGE_FAMILIES]
        return names, [bytes_from_histogram(fams[n], seed=40 + i) for i, n in enumerate(names)]
    return _CACHE.get("families", make)


def pdf_section(names):
    return lambda i: (f"pdf table of {names[i]}", 32, 544, np.uint16)


NORM_ROUTES = ["single-pass", "three-kernel-prologue", "three-kernel-checksum", "user-histogram"]


@pytest.mark.parametrize("pb", PBS)
@pytest.mark.parametrize("route", NORM_ROUTES)
def test_hard_histograms_bytes(C, N, ws, route, pb):
    """Every family but the 32 MiB ones as one pointer batch: normalised by
    k_pcompress, by k_encode's prologue (proNormalize), by normalizeElement
    in k_hist's last workgroup (checksum: at most 25 histogram chunks per
    element, no k_histReduce), and by normalizeElement in k_normalize from
    the caller's histogram."""
    names, datas = family_bytes()
    checksum = route.endswith("checksum")
    refs = ref_archives(0, "families", datas, pb, checksum)
    ts = [to_dev(d, 0) for d in datas]
    hist = None
    if route == "user-histogram":
        hist = torch.from_numpy(np.stack([O.histogram(d) for d in datas]).astype(np.int32)).to(DEV)
    with C.compress_path("single-pass" if route == "single-pass" else "three-kernel"):
        out, sizes = encode_bytes(C, N, ws, ts, pb, checksum, hist)
    sizes_h = check_archives(C, out, sizes, refs, pdf_section(names))
    arch = [out[i, : sizes_h[i]].clone() for i in range(len(ts))]
    outs = [torch.empty(d.size, dtype=torch.uint8, device=DEV) for d in datas]
    ok, _ = C.ans_decode_pointer(arch, outs, prob_bits=pb, checksum=checksum, ws=ws)
    assert ok.cpu().tolist() == [1] * len(ts)
    for name, d, o in zip(names, datas, outs):
        np.testing.assert_array_equal(o.cpu().numpy(), d, err_msg=name)


@pytest.mark.parametrize("pb", PBS)
def test_hard_histograms_sparse(C, ws, pb):
    """fp16 words whose high bytes are a family's symbols and whose low byte
    is 1 (no word is zero), each family as a sparse_compress call of its own
    on the three-kernel path.  Only for a single element does the sparse
    compressor count the list's histogram itself (k_sparseCount) and
    normalise it in k_sparseGather's extra workgroup, the symbol total taken
    from the histogram because the list's length exists only on the device;
    a batch of several elements would go through the dense codec's k_hist
    and prologue instead."""
    names, datas = family_bytes()
    words = _CACHE.get("family-words", lambda: [(d.astype(np.uint16) << 8) | np.uint16(1) for d in datas])
    refs = _CACHE.get(("family-sparse-ref", pb), lambda: [O.sparse_compress(w, 1, pb) for w in words])
    for name, w, ref in zip(names, words, refs):
        # sparse header, bitmap, float header, raw low bytes, ANS header
        at = 16 + -(-((w.size + 7) // 8) // 16) * 16 + 32 + -(-w.size // 16) * 16 + 32
        with C.compress_path("three-kernel"):
            out, sizes = C.sparse_compress([to_dev(w, 1)], ft=1, prob_bits=pb, ws=ws)
        sizes_h = check_archives(C, out, sizes, [ref], lambda i: (f"pdf table of {name}", at, at + 512, np.uint16))
        dec = torch.empty(w.size, dtype=torch.int16, device=DEV)
        ok, sz = C.sparse_decompress([out[0, : sizes_h[0]].clone()], [dec], ft=1, prob_bits=pb, ws=ws)
        assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [w.size], name
        np.testing.assert_array_equal(dec.cpu().numpy().view(np.uint16), w, err_msg=name)


LARGE_ROUTES = ["plain", "checksum", "user-histogram"]


@pytest.mark.parametrize("route", LARGE_ROUTES)
@pytest.mark.parametrize("pb", [10, 11])
def test_hard_histograms_large_totals(C, N, ws, pb, route):
    """The two 32 MiB elements (counts above 2^24; a float32 quotient that
    rounds up across an integer) on the three-kernel path.  checksum: k_hist
    -> k_histReduce (1025 chunks per element), whose last workgroup runs
    normalizeElement.  user-histogram: normalizeElement in k_normalize, from
    the caller's counts.  plain: the same as checksum when the encode grid
    (2050 workgroups) exceeds two generations of resident workgroups, and
    otherwise, as on an MI355X, k_encode's prologue (proNormalize) over
    rows that k_hist accumulated with atomics."""
    def make():
        fams = hard_histograms(0)
        return [bytes_from_histogram(fams[n], seed=60 + i) for i, n in enumerate(LARGE_FAMILIES)]
    datas = _CACHE.get("large", make)
    checksum = route == "checksum"
    refs = ref_archives(0, "large", datas, pb, checksum)
    ts = [to_dev(d, 0) for d in datas]
    hist = None
    if route == "user-histogram":
        fams = hard_histograms(0)
        hist = torch.from_numpy(np.stack([fams[n] for n in LARGE_FAMILIES]).astype(np.int32)).to(DEV)
    with C.compress_path("three-kernel"):
        out, sizes = encode_bytes(C, N, ws, ts, pb, checksum, hist)
    sizes_h = check_archives(C, out, sizes, refs, pdf_section(LARGE_FAMILIES))
    arch = [out[i, : sizes_h[i]].clone() for i in range(len(ts))]
    del out
    outs = [torch.empty(d.size, dtype=torch.uint8, device=DEV) for d in datas]
    ok, _ = C.ans_decode_pointer(arch, outs, prob_bits=pb, checksum=checksum, ws=ws)
    assert ok.cpu().tolist() == [1, 1]
    for d, o in zip(datas, outs):
        assert torch.equal(o.cpu(), torch.from_numpy(d))
