"""GPU tests of the sparse codec (csrc/sparse.hip) at every edge of its index
arithmetic: sizes around the 64-word ballot step, the 1024-word chunk, the
4096-word tile and the 262,144-word scan workgroup with all four zero /
nonzero combinations of the last two words (the reference's n-2 quirk),
inputs and outputs off 16 B alignment, special bit patterns (-0.0 is
nonzero), an element past 65 scan workgroups, archives the reference may emit
and this compressor never does (garbage in the n-2 slot and in the bitmap's
padding), and the failure contract.

Every archive is compared byte for byte with the CPU oracle's
(tests/test_sparse_inputs.py pins the oracle against tests/pyref.py on the same
elements).  Every decode goes into a view of a buffer filled with 0xA5, 16
canary words on each side of every destination; the whole buffer is compared,
so a stray write, or any write to a failing member's destination, fails."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import pyref
from tests.gpu_harness import C, DEV, Cache, dense_at, retyped, workspace_fixture  # noqa: F401
from tests.util import (FT_NAME, NP_SIGNED, NP_WORD, SPARSE_BLOCK_EDGE, SPARSE_LARGE_B, TORCH_WORD, WORD_BYTES,
                        sparse_edge_elements, sparse_far_element, sparse_special_words)

pytestmark = pytest.mark.gpu

FTS = [1, 2, 3, 4]
CANARY = 16  # words on each side of every destination
FILL = 0xA5  # byte pattern of canaries and untouched destinations
GARBAGE = {1: 0xDEAD, 2: 0xBEEF, 3: 0xDEADBEEF, 4: 0xFFFFFFFFFFFFFFFF}

ws = workspace_fixture(1 << 30)
_ELEMENTS, _ORACLE = Cache(), Cache()


def elements(ft):
    """{name: (group, words)} of sparse_edge_elements(ft), generated once."""
    return _ELEMENTS.get(ft, lambda: {name: (group, w) for group, name, w in sparse_edge_elements(ft)})


def oracle_archive(ft, name, w, pb=10, checksum=False):
    """The CPU oracle's archive, computed once per key and left unchanged."""
    return _ORACLE.get((ft, name, pb, checksum), lambda: O.sparse_compress(w, ft, pb, checksum))


def place(words, ft, off):
    """The word arrays as views of ONE device buffer, each starting `off` words
    past a 16 B boundary (off = 1: every input is only word aligned)."""
    per16 = 16 // WORD_BYTES[ft]
    starts, cur = [], 0
    for w in words:
        st = -(-cur // per16) * per16 + off
        starts.append(st)
        cur = st + w.size
    host = np.zeros(cur + per16, dtype=NP_WORD[ft])
    for w, st in zip(words, starts):
        host[st: st + w.size] = w
    buf = torch.from_numpy(host.view(NP_SIGNED[ft])).to(DEV)
    assert buf.data_ptr() % 16 == 0
    views = [buf[st: st + w.size] for w, st in zip(words, starts)]
    for v in views:
        assert v.numel() == 0 or v.data_ptr() % 16 == off * WORD_BYTES[ft]
    return views


def compress_and_compare(C, ws, ft, named, off, pb=10, checksum=False):
    """One batched sparse_compress of named = [(name, words)]; every archive is
    byte-identical to the oracle's.  -> the archives, rows of one tensor."""
    ts = place([w for _, w in named], ft, off)
    out, sizes = C.sparse_compress(ts, ft=ft, prob_bits=pb, checksum=checksum, ws=ws)
    torch.cuda.synchronize()
    sizes_h = sizes.cpu().tolist()
    host = out.cpu().numpy()
    for i, (name, w) in enumerate(named):
        ref = oracle_archive(ft, name, w, pb, checksum)
        assert sizes_h[i] == ref.size, (name, sizes_h[i], ref.size)
        bad = np.flatnonzero(host[i, : ref.size] != ref)
        assert bad.size == 0, f"{FT_NAME[ft]} {name}: {bad.size} archive bytes differ, first at {bad[0]}"
    return [out[i, : sizes_h[i]] for i in range(len(named))]


def decode_members(C, ws, ft, members, pb=10, checksum=False):
    """members: (archive, words, capacity, offset words, expect ok).  One
    batched sparse decode; every destination is `capacity` words starting
    `offset` words past a 16 B boundary inside one buffer of FILL bytes,
    CANARY words on each side.  Checks ok, sz (the archive's n for every
    member, fill_in_nonzeros :118-121) and the whole buffer: a failing
    member's destination stays untouched."""
    wb = WORD_BYTES[ft]
    per16 = 16 // wb
    starts, cur = [], 0
    for (_, _, cap, off, _) in members:
        st = -(-(cur + CANARY) // per16) * per16 + off
        starts.append(st)
        cur = st + cap + CANARY
    total = cur + per16
    buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(TORCH_WORD[ft])
    assert buf.data_ptr() % 16 == 0
    expect = np.full(total * wb, FILL, dtype=np.uint8).view(NP_WORD[ft]).copy()
    for (_, w, cap, _, good), st in zip(members, starts):
        if good:
            assert cap >= w.size
            expect[st: st + w.size] = w
    # The C ABI directly, with every destination's address inside `buf`: an
    # empty tensor view has a null data pointer, and a write to a member of
    # capacity 0 must land in the compared buffer, not at address 0.
    nb = len(members)
    ok = torch.empty([nb], dtype=torch.uint8, device=DEV)
    sz = torch.empty([nb], dtype=torch.int32, device=DEV)
    N = C.N
    rc = N.lib().dietgpu_float_decompress_sparse(
        ws.h, ft, pb, int(checksum), nb, N.ptr_array([m[0].data_ptr() for m in members]),
        N.ptr_array([buf.data_ptr() + st * wb for st in starts]), N.u32_array([m[2] for m in members]),
        ok.data_ptr(), sz.data_ptr(), torch.cuda.current_stream().cuda_stream)
    N.check(rc)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [int(m[4]) for m in members]
    assert sz.cpu().tolist() == [m[1].size for m in members]
    got = buf.cpu().numpy().view(NP_WORD[ft])
    bad = np.flatnonzero(got != expect)
    if bad.size:
        k = int(np.searchsorted(np.asarray(starts) - CANARY, bad[0], side="right")) - 1
        raise AssertionError(f"{FT_NAME[ft]}: {bad.size} words differ, first at buffer word {bad[0]} "
                             f"(member {k}, n {members[k][1].size}, its words start at {starts[k]})")


def roundtrip(C, ws, ft, named, in_off, out_off, pb=10, checksum=False, clone=True):
    arch = compress_and_compare(C, ws, ft, named, in_off, pb, checksum)
    if clone:  # exact-size archives: nothing of ours lies behind them
        arch = [a.clone() for a in arch]
    decode_members(C, ws, ft, [(a, w, w.size, out_off, True) for a, (_, w) in zip(arch, named)], pb, checksum)
    return arch


@pytest.mark.parametrize("in_off", [0, 1], ids=["in16", "in_word"])
@pytest.mark.parametrize("path", ["single-pass", "three-kernel"])
@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_edge_sweep(C, ws, ft, path, in_off):
    """Every element of sparse_edge_elements(): the small group as one pointer
    batch of over 900 elements (its tables are uploaded, the histogram is not
    counted with the bitmap), the 262,144 +- 2 group as a second batch.  in_off
    1: every input is one word off 16 B alignment (k_sparseCount<kVec=false>,
    the word branch of loadTile).  Each batch is decoded twice: from exact-size
    clones of the archives into 16 B-aligned destinations, and into
    destinations one word off."""
    for group in ("small", "large"):
        named = [(name, w) for name, (g, w) in elements(ft).items() if g == group]
        assert len(named) > 900 if group == "small" else len(named) == 20
        with C.compress_path(path):
            arch = compress_and_compare(C, ws, ft, named, in_off)
        clones = [a.clone() for a in arch]
        decode_members(C, ws, ft, [(a, w, w.size, 0, True) for a, (_, w) in zip(clones, named)])
        decode_members(C, ws, ft, [(a, w, w.size, 1, True) for a, (_, w) in zip(arch, named)])


def single_route_names(ft):
    names = [f"n{B + d}_{('zero', 'half', 'dense')[(B + d) % 3]}_t{a}{b}"
             for B in (64, 1024, 4096) for d in (-1, 0, 1, 2) for a in (0, 1) for b in (0, 1)]
    names += [f"n{n}_all_{fill}" for n in SPARSE_BLOCK_EDGE for fill in ("dense", "zero")]
    assert all(n in elements(ft) for n in names)
    return names


@pytest.mark.parametrize("in_off", [0, 1], ids=["in16", "in_word"])
@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_single_element_route(C, ws, ft, in_off):
    """One element per call under the three-kernel path: the only route through
    k_sparseCount<kHist=true> (the list's histogram counted with the bitmap)
    and k_sparseGather's normalising workgroup.  Sizes B-1 .. B+2 for B = 64,
    1024, 4096 with all four tails, and the elements whose list length falls
    on the dense codec's block edge (all nonzero) or is the n-2 slot alone
    (all zero)."""
    with C.compress_path("three-kernel"):
        for name in single_route_names(ft):
            w = elements(ft)[name][1]
            roundtrip(C, ws, ft, [(name, w)], in_off, in_off, clone=False)


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_special_words(C, ws, ft):
    """-0.0, denormals, NaN and Inf patterns and (fp64) words with one zero
    half: only +0.0 leaves the list.  As a batch and as single calls."""
    named = [(f"special_{k}", w) for k, w in sparse_special_words(ft).items()]
    for ck in (False, True):
        roundtrip(C, ws, ft, named, 0, 0, checksum=ck)
    roundtrip(C, ws, ft, named, 1, 1)
    with C.compress_path("three-kernel"):
        for nw in named:
            roundtrip(C, ws, ft, [nw], 0, 0)
            roundtrip(C, ws, ft, [nw], 1, 1)


def test_far_element(C, ws):
    """bf16, 66 * 262,144 + 1102 words, x[n-2] == 0 != x[n-1].  The only case in
    the suite whose chunks belong to scan workgroups above 64, i.e. that takes
    the second round of the blockTot loop of k_sparseExpand (words from
    65 * 262,144 on); its 4,225 tiles also take tilePrefix's second round."""
    w = sparse_far_element()
    assert w.size > 65 * SPARSE_LARGE_B
    roundtrip(C, ws, 2, [("far", w)], 0, 1, clone=False)


def legal_names():
    names = []
    for B in (64, 256, 1024, 4096, 8192):
        names += [f"n{B + 1}_{('zero', 'half', 'dense')[(B + 1) % 3]}_t01",
                  f"n{B}_{('zero', 'half', 'dense')[B % 3]}_t00"]
    # (the all-zero large elements: pyref's byte loops stay short)
    names += [f"n{SPARSE_LARGE_B + 2}_zero_t01", f"n{SPARSE_LARGE_B - 1}_zero_t00"]
    return names


@pytest.mark.parametrize("ft", [2, 4], ids=FT_NAME.get)
def test_reference_legal_archives(C, ws, ft):
    """Archives as the reference may emit them: the n-2 slot of the list and
    the bitmap's padding bytes are uninitialised there.  Twelve elements with
    x[n-2] == 0 across the size edges, each as the oracle's archive, with a
    garbage slot and 0xFF padding, and (sizes that are no multiple of 8) with
    the bits past n of the last bitmap byte set too; one batch."""
    members = []
    for name in legal_names():
        w = elements(ft)[name][1]
        n = w.size
        assert w[n - 2] == 0
        plain = oracle_archive(ft, name, w)
        variants = [plain, pyref.sparse_compress(ft, w, 10, gap_fill=GARBAGE[ft], pad_fill=0xFF)]
        if n % 8:
            variants.append(pyref.sparse_compress(ft, w, 10, gap_fill=GARBAGE[ft] - 1, pad_fill=0xFF,
                                                  pad_bits=True))
        prefix = dense_at(n)
        for v in variants[1:]:
            assert not np.array_equal(v[prefix:], plain[prefix:])
        if len(variants) == 3:  # the last bitmap byte itself differs
            at = 16 + (n + 7) // 8 - 1
            assert variants[2][at] == plain[at] | ((1 << (8 - n % 8)) - 1) != plain[at]
        if ((n + 7) // 8) % 16:
            assert (variants[1][16 + (n + 7) // 8: prefix] == 0xFF).all()
        for k, v in enumerate(variants):
            members.append((torch.from_numpy(v.copy()).to(DEV), w, n, k % 2, True))
    assert len(members) >= 30
    decode_members(C, ws, ft, members)


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_failure_contract(C, ws, ft):
    """outSuccess = the dense decode succeeded and capacity >= n; outSize = n
    always; nothing is written on failure (sparse.hip k_sparseExpand,
    fill_in_nonzeros :118-121, or_sparse_float_decompress).  One mixed batch:
    good members first, last and between the failing ones."""
    els = elements(ft)
    pick = ["n4097_dense_t01", "n1025_dense_t01", "n200_dense_t10", "n8193_zero_t01", "n2049_zero_t01"]
    ws_ = {k: els[k][1] for k in pick}
    arch = dict(zip(pick, compress_and_compare(C, ws, ft, [(k, ws_[k]) for k in pick], 0)))
    with_pb9 = compress_and_compare(C, ws, ft, [("n1025_dense_t01", ws_["n1025_dense_t01"])], 0, pb=9)[0]
    a, b, c, d, e = pick
    members = [
        (arch[a], ws_[a], ws_[a].size, 0, True),
        (arch[b], ws_[b], ws_[b].size - 1, 0, False),        # capacity n-1
        (arch[c], ws_[c], ws_[c].size, 1, True),
        (arch[a], ws_[a], 0, 0, False),                      # capacity 0
        (retyped(arch[d], ft, at=dense_at(ws_[d].size) + 8), ws_[d], ws_[d].size, 0, False),
        (arch[e], ws_[e], ws_[e].size + 3, 0, True),         # room to spare
        (with_pb9, ws_[b], ws_[b].size, 1, False),           # compressed at pb 9
        (retyped(arch[b], ft, at=dense_at(ws_[b].size) + 8), ws_[b], ws_[b].size, 0, False),
        (arch[b], ws_[b], ws_[b].size, 0, True),
    ]
    decode_members(C, ws, ft, members)
    # the oracle reports the same members as failing
    for (arc, w, cap, _, good) in members:
        st, _ = O.sparse_decompress(arc.cpu().numpy(), ft, 10, capacity=max(cap, 0))
        assert (st == 0) == good


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_checksum_mismatch_is_reported(C, ws, ft):
    """A flipped byte in the raw (non-ANS) section of a sparse archive's dense
    archive: the batch raises ChecksumMismatch, the intact element alone
    decodes."""
    from dietgpu_fork_amd import ChecksumMismatch

    els = elements(ft)
    named = [(k, els[k][1]) for k in ("n4097_dense_t01", "n1025_dense_t01")]
    arch = roundtrip(C, ws, ft, named, 0, 0, checksum=True)
    n = named[1][1].size
    bad = arch[1].clone()
    bad[dense_at(n) + 40] ^= 0xFF
    outs = [torch.empty(w.size, dtype=TORCH_WORD[ft], device=DEV) for _, w in named]
    with pytest.raises(ChecksumMismatch):
        C.sparse_decompress([arch[0], bad], outs, ft=ft, prob_bits=10, checksum=True, ws=ws)
    torch.cuda.synchronize()
    decode_members(C, ws, ft, [(arch[0], named[0][1], named[0][1].size, 0, True)], checksum=True)
