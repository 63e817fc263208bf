"""GPU tests of the sparse range decode (csrc/sparse.hip: k_sparseRangeChunks,
k_sparseRangePlan, the dense range decode of the list slice,
k_sparseExpandRange).

The expected value is always x[first : first + count] of the original words,
bitwise.  Archives come from the CPU oracle (or tests/pyref.py for what only
the reference may emit), uploaded.  Every destination sits in a buffer of 0xA5
bytes with 16 canary words on each side and the whole buffer is compared, so
a write outside out[0 .. count), or any write for a failing member, fails.
The inputs and ranges are those of tests/sparse_range_cases.py, which
tests/test_sparse_range_inputs.py checks on the CPU."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import pyref
from tests import sparse_range_cases as K
from tests.gpu_harness import C, DEV, Cache, dense_at, retyped, workspace_fixture  # noqa: F401
from tests.util import (FT_NAME, NP_SIGNED, NP_WORD, TORCH_WORD, WORD_BYTES, sparse_edge_elements,
                        sparse_far_element)

pytestmark = pytest.mark.gpu

FTS = [1, 2, 3, 4]
CANARY = 16  # words on each side of every destination
FILL = 0xA5  # byte pattern of canaries and untouched destinations

ws = workspace_fixture(1 << 30)
_ELEMENTS, _ARCHIVES = Cache(), Cache()


def elements(ft):
    return _ELEMENTS.get(ft, lambda: {name: w for _, name, w in sparse_edge_elements(ft)})


def oracle_archive(ft, key, w, pb=10, checksum=False):
    """The CPU oracle's archive on the device, made once per key."""
    return _ARCHIVES.get((ft, key, pb, checksum),
                         lambda: torch.from_numpy(O.sparse_compress(w, ft, pb, checksum)).to(DEV))


def run_members(C, ws, ft, members, pb=10):
    """members: (archive, words, first, count, expect ok).  One batched range
    decode on the current stream; member k's destination is `count` words
    (at most 64 for a member expected to fail, whose count may be absurd)
    starting k % 2 words past a 16 B boundary (16 B-aligned and one word off,
    alternating).  Checks ok, sz (count, or 0 for a failing member) and the
    whole buffer."""
    wb = WORD_BYTES[ft]
    per16 = 16 // wb
    starts, cur = [], 0
    for k, (_, _, _, count, good) in enumerate(members):
        st = -(-(cur + CANARY) // per16) * per16 + k % 2
        starts.append(st)
        cur = st + (count if good else min(count, 64)) + CANARY
    total = cur + per16
    buf = torch.full([total * wb], FILL, dtype=torch.uint8, device=DEV).view(TORCH_WORD[ft])
    assert buf.data_ptr() % 16 == 0
    expect = np.full(total * wb, FILL, dtype=np.uint8).view(NP_WORD[ft]).copy()
    for (_, w, first, count, good), st in zip(members, starts):
        if good:
            assert first + count <= w.size
            expect[st: st + count] = w[first: first + count]
    nb = len(members)
    ok = torch.full([nb], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([nb], -7, dtype=torch.int32, device=DEV)
    N = C.N
    for m in members:
        assert m[0].data_ptr() % 16 == 0
    rc = N.lib().dietgpu_float_decompress_sparse_range(
        ws.h, ft, pb, nb, N.ptr_array([m[0].data_ptr() for m in members]), N.u32_array([m[2] for m in members]),
        N.u32_array([m[3] for m in members]), N.ptr_array([buf.data_ptr() + st * wb for st in starts]),
        ok.data_ptr(), sz.data_ptr(), torch.cuda.current_stream().cuda_stream)
    N.check(rc)
    torch.cuda.current_stream().synchronize()
    ok_h, sz_h = ok.cpu().tolist(), sz.cpu().tolist()
    want_ok = [int(m[4]) for m in members]
    bad = [k for k in range(nb) if ok_h[k] != want_ok[k]]
    assert not bad, f"{FT_NAME[ft]}: status of member {bad[0]} (first {members[bad[0]][2]}, count " \
                    f"{members[bad[0]][3]}) is {ok_h[bad[0]]}; {len(bad)} wrong"
    assert sz_h == [m[3] if m[4] else 0 for m in members]
    got = buf.cpu().numpy().view(NP_WORD[ft])
    diff = np.flatnonzero(got != expect)
    if diff.size:
        k = int(np.searchsorted(np.asarray(starts) - CANARY, diff[0], side="right")) - 1
        raise AssertionError(f"{FT_NAME[ft]}: {diff.size} words differ, first at buffer word {diff[0]} (member {k}: "
                             f"n {members[k][1].size}, first {members[k][2]}, count {members[k][3]}, its words "
                             f"start at {starts[k]})")


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_range_edges(C, ws, ft):
    """sparse_edge_elements() at sizes 0-3, 63-65, 1023-1025, 4095-4097 and
    262,143-262,145 with all four tails (the content cycles through all-zero,
    half-zero and zero-free with the size); of each element every range whose
    first and end come from {0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096,
    4097, n-2, n-1, n}, the empty ranges and the whole element among them.
    The elements up to 4097 words are ONE pointer batch of 1,475 members in
    which up to 66 share an archive.  The scratch rows of a call are sized
    by its largest count, so the 262 K elements do not join that batch (it
    would take 1.4 to 5.7 GB of rows): each is a batch of its own 105 members
    interleaved with the 244 members of the twelve elements of 3, 65 and 1025
    words, so that archives of 3 to 262,145 words share a call in every float
    type."""
    els = elements(ft)
    small = []
    for name in K.edge_names(K.EDGE_SMALL):
        w = els[name]
        a = oracle_archive(ft, name, w)
        small += [(a, w, f, c, True) for f, c in K.edge_ranges(w.size)]
    assert len(small) == 1475
    run_members(C, ws, ft, small)
    few = [m for m in small if m[1].size in (3, 65, 1025)]
    assert len(few) == 244
    for name in K.edge_names(K.EDGE_LARGE):
        w = els[name]
        a = oracle_archive(ft, name, w)
        big = [(a, w, f, c, True) for f, c in K.edge_ranges(w.size)]
        mixed = []
        for k in range(len(few)):
            mixed.append(few[k])
            if k < len(big):
                mixed.append(big[k])
        assert len(mixed) == 244 + 105
        run_members(C, ws, ft, mixed)


def test_more_members_and_archives_than_a_grid_row(C, ws):
    """65,600 members, each reading its own copy of one archive: more members
    and more distinct archives than a grid's y dimension (65,535) holds, so
    every stage launches a second slice."""
    ft = 2
    w = elements(ft)["n65_dense_t01"]
    one = O.sparse_compress(w, ft, 10, False)
    stride = -(-one.size // 16) * 16
    copies = 65600
    row = np.zeros(stride, dtype=np.uint8)
    row[: one.size] = one
    pool = torch.from_numpy(row).to(DEV).repeat(copies).view(copies, stride)
    members = [(pool[k], w, k % 60, 1 + k % 5, True) for k in range(copies)]
    members[65590] = (pool[65590], w, 64, 2, False)  # a failing member in the second slice
    run_members(C, ws, ft, members)


@pytest.mark.parametrize("ft", [2, 3], ids=FT_NAME.get)
def test_list_block_edge(C, ws, ft):
    """rank(first) = 4095, 4096, 4097 with counts 1, 2 and 9000: the list slice
    starts before, on and after a dense rANS block edge and spans three
    blocks."""
    x = K.list_block_element(ft)
    a = oracle_archive(ft, "list_block", x)
    run_members(C, ws, ft, [(a, x, f, c, True) for f, c in K.list_block_ranges(x)])


def test_workgroup_total_edges(C, ws):
    """Ranks on each side of a counting workgroup's edge (words 262,144 and
    524,288 of a 2 x 262,144 + 1102-word element), and sparse_far_element():
    past 64 counting workgroups, the second round of the total sums in
    k_sparseRangePlan and k_sparseExpandRange."""
    x = K.wg_element()
    a = oracle_archive(2, "wg", x)
    run_members(C, ws, 2, [(a, x, f, c, True) for f, c in K.wg_ranges()])
    far = sparse_far_element()
    fa = oracle_archive(2, "far", far)
    run_members(C, ws, 2, [(fa, far, f, c, True) for f, c in K.far_ranges()])
    # both archives in one call: the chunk tables of two archives of very
    # different sizes side by side
    run_members(C, ws, 2, [(fa, far, *K.far_ranges()[1], True), (a, x, *K.wg_ranges()[6], True),
                           (fa, far, *K.far_ranges()[3], True)])


@pytest.mark.parametrize("ft", [2, 4], ids=FT_NAME.get)
def test_quirk_and_legal_archives(C, ws, ft):
    """Archives as the reference may write them: all ones in the list slot
    before x[n-1] (x[n-2] == 0), 0xFF bitmap padding, the bits past n of the
    last bitmap byte set, and 0xFF in the header's don't-care bytes 4..15
    (the reference writes them from uninitialised memory).  Ranges that end at
    n-1 and at n and that start at n-1 match x, with x[n-2] == 0 and != 0."""
    els = elements(ft)
    members, seen = [], set()
    for name in K.edge_names(K.QUIRK_SIZES):
        w = els[name]
        seen.add(bool(w[-2] != 0))
        arch = pyref.sparse_compress(ft, w, 10, gap_fill=K.ALL_ONES[ft], pad_fill=0xFF, pad_bits=True)
        plain = O.sparse_compress(w, ft, 10, False)
        if w[-2] == 0 or w.size % 8:
            assert not np.array_equal(arch, plain)
        arch = arch.copy()
        assert not arch[4:16].any()
        arch[4:16] = 0xFF
        a = torch.from_numpy(arch).to(DEV)
        members += [(a, w, f, c, True) for f, c in K.quirk_ranges(w.size)]
    assert seen == {False, True}
    run_members(C, ws, ft, members)


def test_parameters(C, ws):
    """Prob bits 9 and 11, an archive written with a checksum, an archive
    compressed on the GPU, and a side stream."""
    ft = 3
    w = elements(ft)["n4097_dense_t01"]
    h = elements(ft)["n4096_half_t01"]
    ranges = [(0, w.size), (4090, 7), (1, 1024), (w.size - 1, 1), (63, 2)]
    for pb in (9, 11):
        run_members(C, ws, ft, [(oracle_archive(ft, "w", w, pb), w, f, c, True) for f, c in ranges], pb=pb)
    run_members(C, ws, ft, [(oracle_archive(ft, "w", w, 10, True), w, f, c, True) for f, c in ranges])
    t = torch.from_numpy(h.view(NP_SIGNED[ft])).to(DEV)
    out, sizes = C.sparse_compress([t], ft=ft, ws=ws)
    torch.cuda.synchronize()
    gpu_arch = out[0, : int(sizes[0])]
    hr = [(0, h.size), (4000, 96), (1023, 2), (h.size - 2, 2)]
    run_members(C, ws, ft, [(gpu_arch, h, f, c, True) for f, c in hr])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_members(C, ws, ft, [(gpu_arch, h, f, c, True) for f, c in hr] +
                    [(oracle_archive(ft, "w", w), w, f, c, True) for f, c in ranges])
    torch.cuda.synchronize()


@pytest.mark.parametrize("ft", FTS, ids=FT_NAME.get)
def test_failures_in_a_mixed_batch(C, ws, ft):
    """Each failing member: status 0, size 0, destination untouched; the good
    members between them stay exact."""
    els = elements(ft)
    w = els["n4097_dense_t01"]
    n = w.size
    a = oracle_archive(ft, "n4097_dense_t01", w)
    pb9 = oracle_archive(ft, "n4097_dense_t01", w, 9)
    dense = torch.from_numpy(O.float_compress(w, ft)).to(DEV)
    # eight leading zero words, then no zeros: setting the first bitmap byte
    # makes every rank 8 too large, so the whole element's list slice
    # overruns the dense archive's element
    z = w.copy()
    z[:8] = 0
    za = oracle_archive(ft, "z8", z)
    zbad = za.clone()
    assert int(zbad[16]) == 0
    zbad[16] = 0xFF
    members = [
        (a, w, 0, n, True),
        (a, w, n - 3, 4, False),            # one word past the end
        (a, w, 100, 1000, True),
        (a, w, n + 1, 0, False),            # first > n
        (a, w, n + 5, 3, False),
        (a, w, n, 0, True),                 # the empty range at n
        (a, w, 0xFFFFFFFF, 2, False),       # first + count wraps
        (a, w, 5, 0xFFFFFFFE, False),       # a count no archive can hold: sizes no scratch row
        (za, z, 0, n, True),
        (retyped(a, ft, at=dense_at(n) + 8), w, 0, n, False),   # the wrong float type
        (pb9, w, 5, 50, False),             # the wrong prob bits
        (a, w, 4095, 2, True),
        (dense, w, 0, 100, False),          # a dense float archive
        (zbad, z, 0, n, False),             # the rank exceeds the list
        (a, w, n - 1, 1, True),
    ]
    run_members(C, ws, ft, members)


def test_gather_rows_sparse(C):
    """256 rows (repeats, the first and the last row) of a [4096, 1024] bf16
    table at 90 % zeros; an out-of-table row raises.  The workspace's peak
    stays below 256 * 4096 * 4 bytes, what chunk tables per MEMBER alone would
    take: the bitmap is counted once per archive."""
    table = K.gather_table()
    rows = K.gather_rows()
    arch = torch.from_numpy(O.sparse_compress(table.reshape(-1), 2, 10, False)).to(DEV)
    fresh = C.Workspace(64 << 20)
    got = C.gather_rows(arch, K.GATHER_WORDS, rows, torch.bfloat16, ws=fresh, sparse=True)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (256, K.GATHER_WORDS)
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), table[rows])
    assert 0 < fresh.max_usage() < 256 * 4096 * 4
    with pytest.raises(C.N.DietGpuError):
        C.gather_rows(arch, K.GATHER_WORDS, [3, K.GATHER_ROWS], torch.bfloat16, ws=fresh, sparse=True)
    with pytest.raises(ValueError):
        C.gather_rows(arch, K.GATHER_WORDS, [3], torch.uint8, ws=fresh, sparse=True)
    # codec.sparse_decompress_range, the list form of the same call
    outs, ok, sz = C.sparse_decompress_range([arch, arch], [1024 * 7 + 3, 0], [100, 1], dtype=torch.bfloat16,
                                             ws=fresh)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1, 1] and sz.cpu().tolist() == [100, 1]
    flat = table.reshape(-1)
    assert np.array_equal(outs[0].view(torch.int16).cpu().numpy().view(np.uint16), flat[7171: 7271])
    assert np.array_equal(outs[1].view(torch.int16).cpu().numpy().view(np.uint16), flat[:1])


def test_hook_rejects_a_checksum_config(C, ws):
    """floatDecompressSparseRange refuses FloatCodecConfig.useChecksum (the C
    ABI has no such flag); without it the same call decodes."""
    ft = 2
    w = elements(ft)["n1025_dense_t01"]
    a = oracle_archive(ft, "n1025_dense_t01", w)
    T = C.N.testlib()
    out = torch.full([64], 0x2525, dtype=torch.int16, device=DEV)
    ok = torch.full([1], 7, dtype=torch.uint8, device=DEV)
    sz = torch.full([1], -7, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    rc = T.dietgpu_test_sparse_range_config(ws.h, ft, 1, a.data_ptr(), 1000, 25, out.data_ptr(), ok.data_ptr(),
                                            sz.data_ptr(), s)
    assert rc != C.N.DIETGPU_OK
    assert "a range decode cannot verify a checksum" in T.dietgpu_test_last_error().decode()
    torch.cuda.synchronize()
    assert ok.item() == 7 and (out.cpu().numpy() == 0x2525).all()
    rc = T.dietgpu_test_sparse_range_config(ws.h, ft, 0, a.data_ptr(), 1000, 25, out.data_ptr(), ok.data_ptr(),
                                            sz.data_ptr(), s)
    C.N.test_check(rc)
    torch.cuda.synchronize()
    assert ok.item() == 1 and sz.item() == 25
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:25], w[1000:1025]) and (got[25:] == 0x2525).all()
