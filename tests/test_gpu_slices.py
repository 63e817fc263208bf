"""Batches of more than 65,535 members: every batched driver cuts its batch
into grid-Y slices (forGridYSlices, csrc/codec_internal.h) and each kernel adds
the slice's first member to blockIdx.y.  These tests run a second (and a
third) slice of every such launch and compare all members with the oracle's
archives, plain slices of the inputs or the CPU models (tests/slice_cases.py,
whose properties tests/test_slice_inputs.py checks on the CPU).

Member i holds content i % 7, so a member and the one 65,535 before it differ
in size and in words.  Every output, size and status buffer holds sentinels
before the call (0xAB bytes, sizes -7, status 7): a member no workgroup
reached shows as unwritten.  Decode outputs and accumulators lie in one buffer
with guard words between them (gpu_harness.word_starts); the buffer, what it
must hold and the comparison stay on the device, and the whole buffer is
compared, so a write that lands in another member's row fails the test.  The
members on both sides of each slice edge and the last one are asserted on by
name first.

The calls go to the C ABI with numpy pointer columns (the entry points that
dietgpu_fork_amd.codec wraps; its wrappers allocate their own status tensors,
and 65,537 tensor views per call are host time), except the operator test,
which is about those lists.  Footprints are device bytes per test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import accumulate_cases as A
from tests import slice_cases as SC
from tests import sparse_reduce_cases as SR
from tests.gpu_harness import (C, DEV, N, Cache, host_ptrs, pack_bytes, placed_mismatch, scatter_rows,  # noqa: F401
                               sentinel_words, word_starts, workspace_fixture)
from tests.util import TORCH_WORD, WORD_BYTES

pytestmark = pytest.mark.gpu

# The largest calls: the three-kernel compress of 131,071 bf16 members takes
# block slots of 5.8 KB per segment, member and block (two blocks: 1.5 GB),
# 4.6 KB of encode table and pdf per segment and member (0.6 GB) and a 1 KB
# histogram row each (the same for 65,537 fp64 members of two segments); the
# sparse reduce of 65,537 members decodes 4 x 65,537 nonzero lists into rows of
# the largest member's capacity (about 2.2 GB).  _call() asserts that no call
# goes past the arena.
WS_BYTES = 4 << 30
ws = workspace_fixture(WS_BYTES)
_CACHE = Cache()
SIGNED = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
CHUNK_ROWS = 16384  # rows of a [nb, cols] comparison at a time
K7 = SC.K_DISTINCT
SIZES = np.array(SC.ALL_SIZES, dtype=np.int64)  # by content index, the empty content last


_ROWS = []  # the archive matrices of the running test


@pytest.fixture(autouse=True)
def _release_archive_rows():
    """An archive matrix is tens of GB (see _archive_rows): its memory goes
    back when the test ends, also while a failure's traceback still refers
    to the tensor, so that one failing test does not starve the next."""
    yield
    for t in _ROWS:
        t.untyped_storage().resize_(0)
    _ROWS.clear()


def _archive_rows(nb, cols):
    """[nb, cols] sentinel bytes for nb archives.  cols is the codec's bound
    for the largest member, as the pointer and stride forms ask for; its
    constant term (the header overhead of 4,096 blocks) makes that 572 KB for
    a 4097-word bf16 member and 1.16 MB for an fp64 one."""
    out = sentinel_words([nb, cols], torch.uint8)
    _ROWS.append(out)
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(N, ws, name, *args):
    """One C-ABI call on the current stream, finished, within the arena."""
    N.lib().dietgpu_stack_reset_max_usage(ws.h)
    N.check(getattr(N.lib(), name)(ws.h, *args, _stream()))
    torch.cuda.synchronize()
    assert ws.max_usage() <= WS_BYTES, f"{name}: the call took {ws.max_usage()} B of a {WS_BYTES} B arena"


def _dev(a):
    """A numpy array on the device, unsigned words as signed ones."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(a.dtype.str.replace("u", "i"))
    return torch.from_numpy(a).to(DEV)


def _which(nb, empty=False):
    """(numpy, device) content index of every member; empty: with the empty
    members of slice_cases.empty_members()."""
    def make():
        w = SC.member_contents(nb, empty)
        return w, _dev(w)
    return _CACHE.get(("which", nb, empty), make)


def _blobs(key, arrays):
    """The arrays' bytes in one device buffer, each 16 B-aligned -> (views,
    addresses as numpy uint64), made once and left unchanged."""
    def make():
        # (an empty array gets 16 bytes of its own, so that it has an address)
        blobs = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) if a.size else np.zeros(16, dtype=np.uint8)
                 for a in arrays]
        views = pack_bytes(blobs, [0] * len(arrays))
        return views, np.array([v.data_ptr() for v in views], dtype=np.uint64)
    return _CACHE.get(key, make)


def _inputs(kind, ft, src=0):
    """The seven contents of a kind and the empty one on the device -> (words,
    views, addresses)."""
    make = {"dense": SC.words, "sparse": SC.sparse_words}[kind]
    words = _CACHE.get(("words", kind, ft, src), lambda: [make(ft, c, src) for c in range(SC.CONTENTS)])
    return (words,) + _blobs(("in", kind, ft, src), words)


def _archives(kind, ft, checksum=False, src=0):
    """The oracle's archives of the eight contents, each encoded once ->
    (archives, device views, addresses)."""
    def make():
        words = _inputs(kind, ft, src)[0]
        if kind == "sparse":
            return [O.sparse_compress(w, ft, 10, checksum) for w in words]
        if ft == 0:
            return [O.ans_encode(w, 10, checksum) for w in words]
        return [O.float_compress(w, ft, 10, checksum) for w in words]
    refs = _CACHE.get(("refs", kind, ft, checksum, src), make)
    return (refs,) + _blobs(("arch", kind, ft, checksum, src), refs)


def _status(nb):
    return (torch.full([nb], 7, dtype=torch.uint8, device=DEV), torch.full([nb], -7, dtype=torch.int32, device=DEV))


def _check_status(what, ok, sz, want_ok, want_sz):
    """Status and sizes of all members, the named ones first."""
    nb = len(want_ok)
    ok, sz = ok.cpu().numpy().astype(np.int64), sz.cpu().numpy().astype(np.int64)
    for i in SC.named_members(nb):
        assert (ok[i], sz[i]) == (want_ok[i], want_sz[i]), (
            f"{what}: member {i} reports status {ok[i]} and size {sz[i]}, expected "
            f"{want_ok[i]} and {want_sz[i]}")
    bad = np.flatnonzero((ok != want_ok) | (sz != want_sz))
    assert bad.size == 0, f"{what}: status or size of {bad.size} members is wrong, first {bad[:8].tolist()}"


class Placed:
    """Destinations of caps[i] words of `dtype` for every member in one
    buffer of sentinels, GUARD words apart (word_starts); `want` is what the
    buffer must hold after the call, filled by put()."""

    def __init__(self, dtype, caps):
        self.caps = np.asarray(caps, dtype=np.int64)
        starts, self.total = word_starts(dtype, self.caps.tolist(), [0] * self.caps.size)
        self.starts = np.array(starts, dtype=np.int64)
        self.starts_dev = _dev(self.starts)
        self.buf = sentinel_words(self.total, dtype)
        self.want = sentinel_words(self.total, dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = host_ptrs(self.buf.data_ptr(), self.starts, dtype.itemsize)
        self.caps32 = self.caps.astype(np.uint32)

    def put(self, target, members, row, firsts=0, counts=None):
        """row[firsts + j], j < counts (default: the whole row), into the
        slices of `members` (numpy indices) of target (buf or want)."""
        row = _dev(row) if isinstance(row, np.ndarray) else row
        counts = row.numel() if counts is None else counts
        firsts, counts = (_dev(v) if isinstance(v, np.ndarray) else v for v in (firsts, counts))
        scatter_rows(target, self.starts_dev[_dev(members)], firsts, counts, row)

    def put_rows(self, target, rows, which, skip=()):
        """rows[which[i]] (numpy words) into every member's slice but `skip`."""
        for c, row in enumerate(rows):
            members = np.setdiff1d(np.flatnonzero(which == c), np.asarray(skip, dtype=np.int64))
            self.put(target, members, row)

    def check(self, what):
        for i in SC.named_members(self.caps.size):
            sl = slice(int(self.starts[i]), int(self.starts[i] + self.caps[i]))
            got, want = self.buf[sl].cpu(), self.want[sl].cpu()
            bad = (got != want).nonzero().view(-1)
            assert bad.numel() == 0, (
                f"{what}: member {i} ({self.caps[i]} words): {bad.numel()} words differ, first at "
                f"word {int(bad[0])}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}")
        problem = placed_mismatch(self.buf, self.want, self.starts)
        assert problem is None, f"{what}: {problem}"


def _check_archives(what, out, sizes, refs, nb, empty=False):
    """out [nb, cols] uint8 and sizes int32 [nb] on the device: row i holds
    the archive refs[content of member i], byte for byte, over its length."""
    cols = out.shape[1]
    lens = np.array([r.size for r in refs], dtype=np.int64)
    assert lens.max() <= cols
    which, which_dev = _which(nb, empty)
    got = sizes.cpu().numpy().astype(np.int64)
    want = lens[which]
    for i in SC.named_members(nb):
        assert got[i] == want[i], (f"{what}: member {i} (content {which[i]}) has size {got[i]}, the oracle's "
                                   f"archive has {want[i]} bytes")
        row = out[i, : want[i]].cpu().numpy()
        bad = np.flatnonzero(row != refs[which[i]])
        assert bad.size == 0, (f"{what}: member {i} (content {which[i]}) differs from the oracle's archive in "
                               f"{bad.size} of {want[i]} bytes, first at byte {bad[0]}")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: the sizes of {bad.size} members are wrong, first {bad[:8].tolist()}"
    width = int(lens.max())  # (nothing is compared past a row's archive)
    exp7 = _dev(SC.padded(refs, width))
    mask7 = torch.arange(width, device=DEV)[None, :] < _dev(lens)[:, None]
    for r0 in range(0, nb, CHUNK_ROWS):
        w = which_dev[r0:r0 + CHUNK_ROWS]
        rows = ((out[r0:r0 + CHUNK_ROWS, :width] != exp7[w]) & mask7[w]).any(1).nonzero().view(-1)
        assert rows.numel() == 0, (f"{what}: {rows.numel()} members of {r0} .. differ from the oracle's archives, "
                                   f"first {(rows[:8] + r0).tolist()}")


def _compress_pointer(N, ws, entry, ft, addrs, nb, checksum, cols):
    """One pointer-form compress of nb members, the empty ones among them,
    member i the content at addrs[its content], into rows of `cols` sentinel
    bytes -> (out, sizes)."""
    which, _ = _which(nb, True)
    out = _archive_rows(nb, cols)
    sizes = torch.full([nb], -7, dtype=torch.int32, device=DEV)
    ins = addrs[which]
    ns = SIZES[which].astype(np.uint32)
    outs = host_ptrs(out.data_ptr(), np.arange(nb), cols)
    head = (10, int(checksum)) if ft == 0 else (ft, 10, int(checksum))
    mid = (None,) if ft == 0 else ()  # the byte codec's histograms
    _call(N, ws, entry, *head, nb, ins.ctypes.data, ns.ctypes.data, *mid, outs.ctypes.data, sizes.data_ptr())
    return out, sizes


# --------------------------------------------------------- 1, 2: dense compress ----

@pytest.mark.parametrize("name,ft,form,checksum,user_hist,nb", SC.COMPRESS_THREE_KERNEL,
                         ids=SC.ids(SC.COMPRESS_THREE_KERNEL))
def test_compress_three_kernel(C, N, ws, name, ft, form, checksum, user_hist, nb):
    """k_hist, launchChecksum, k_normalize, k_encode and (fp64) k_coalesce per
    slice; archives byte-identical to the oracle's.  Pointer form: ragged
    sizes, empty members among them; stride form: rows of 4097 words.  Footprint: nb rows of the largest
    member's bound (_archive_rows; bf16 and bytes 37.5 GB, 75 GB at 131,071
    members; fp32 38 GB; fp64 76 GB), the comparison's chunks (under 1 GB),
    and up to 2.3 GB of the arena."""
    with C.compress_path("three-kernel"):
        # the plan of nb members of the largest size: the driver plans by the
        # largest member, so it is the ragged pointer-form call's plan too, as
        # far as the path and the normalisation route go
        plan = C.test_compress_plan(ft, nb, SC.ROW, checksum, user_hist, True)
        print(name, plan)
        assert not plan["single_pass"] and plan["normalise"] == "kernel", plan
        if form == "pointer":
            refs = _archives("dense", ft, checksum)[0]
            cols = C.max_compressed_size(SC.ROW) if ft == 0 else C.max_float_compressed_size(ft, SC.ROW)
            entry = "dietgpu_ans_encode_batch_pointer" if ft == 0 else "dietgpu_float_compress"
            out, sizes = _compress_pointer(N, ws, entry, ft, _inputs("dense", ft)[2], nb, checksum, cols)
        else:
            rows = _CACHE.get(("rows", ft), lambda: [SC.row_words(ft, c) for c in range(K7)])
            refs = _CACHE.get(("rowrefs", ft, checksum), lambda: [
                O.ans_encode(w, 10, checksum) if ft == 0 else O.float_compress(w, ft, 10, checksum) for w in rows])
            _, which_dev = _which(nb)
            x = _dev(np.stack(rows))[which_dev]
            cols = C.max_compressed_size(SC.ROW) if ft == 0 else C.max_float_compressed_size(ft, SC.ROW)
            out = _archive_rows(nb, cols)
            sizes = torch.full([nb], -7, dtype=torch.int32, device=DEV)
            if ft == 0:
                hist = _dev(np.stack([O.histogram(w) for w in rows]).astype(np.int32))[which_dev] if user_hist else None
                C.ans_encode_stride(x, prob_bits=10, checksum=checksum, ws=ws, histogram=hist, out=out, sizes=sizes)
            else:
                C.float_compress_stride(x, ft=ft, prob_bits=10, checksum=checksum, ws=ws, out=out, sizes=sizes)
            torch.cuda.synchronize()
    _check_archives(name, out, sizes, refs, nb, empty=form == "pointer")


@pytest.mark.parametrize("name,ft,nb", SC.COMPRESS_SINGLE_PASS, ids=SC.ids(SC.COMPRESS_SINGLE_PASS))
def test_compress_single_pass(C, N, ws, name, ft, nb):
    """k_pcompress takes the batch in some 65 rounds off its dequeue counter,
    behind (bf16) the sliced float checksum pass; checksum on.  Footprint: as
    the pointer form above, 37.5 GB."""
    C.device_error_count()
    C.barrier_fallback_count()
    with C.compress_path("single-pass"):
        plan = C.test_compress_plan(ft, nb, SC.ROW, True, False, True)
        print(name, plan)
        assert plan["single_pass"] and not plan["too_many_items"], plan
        refs = _archives("dense", ft, True)[0]
        cols = C.max_compressed_size(SC.ROW) if ft == 0 else C.max_float_compressed_size(ft, SC.ROW)
        entry = "dietgpu_ans_encode_batch_pointer" if ft == 0 else "dietgpu_float_compress"
        out, sizes = _compress_pointer(N, ws, entry, ft, _inputs("dense", ft)[2], nb, True, cols)
    assert C.device_error_count() == 0
    assert C.barrier_fallback_count() == 0
    _check_archives(name, out, sizes, refs, nb, empty=True)


# ------------------------------------------------------------- 3: dense decode ----

@pytest.mark.parametrize("name,ft,form,checksum,short,nb", SC.DECODE, ids=SC.ids(SC.DECODE))
def test_decode(C, N, ws, name, ft, form, checksum, short, nb):
    """k_decode's full form (and, checksum on, verifyChecksums' sliced
    checksum pass) over the oracle's archives.  short: member 65,535 has room
    for 32 of its 33 words; it alone fails, its row stays untouched.
    Footprint: two placed buffers of nb x about 1,530 words (fp64: 2 x
    0.8 GB), stride form two of nb x 4097 words, and transient index tensors
    of the expected buffer (up to 1.2 GB at 131,071 members)."""
    words = _inputs("dense", ft)[0]
    refs, views, addrs = _archives("dense", ft, checksum)
    which, which_dev = _which(nb, form == "pointer")  # (pointer form: with the empty members)
    ok, sz = _status(nb)
    want_ok, want_sz = np.ones(nb, dtype=np.int64), SIZES[which]
    wdt = TORCH_WORD[ft]
    if form == "pointer":
        caps = SIZES[which].copy()
        skip = ()
        if short:
            assert SC.SHORT_MEMBER < nb and caps[SC.SHORT_MEMBER] == 33
            caps[SC.SHORT_MEMBER] -= 1
            want_ok[SC.SHORT_MEMBER] = 0
            skip = (SC.SHORT_MEMBER,)
        p = Placed(wdt, caps)
        p.put_rows(p.want, words, which, skip)
        ins = addrs[which]
        head = (10, int(checksum)) if ft == 0 else (ft, 10, int(checksum))
        entry = "dietgpu_ans_decode_batch_pointer" if ft == 0 else "dietgpu_float_decompress"
        _call(N, ws, entry, *head, nb, ins.ctypes.data, p.ptrs.ctypes.data, p.caps32.ctypes.data, ok.data_ptr(),
              sz.data_ptr())
        _check_status(name, ok, sz, want_ok, want_sz)
        p.check(name)
        return
    stride = -(-max(r.size for r in refs) // 16) * 16
    arch = _dev(SC.padded(refs, stride))[which_dev]
    out = sentinel_words([nb, SC.ROW], wdt)
    want = _dev(SC.padded(words, SC.ROW)).clone()
    tail = torch.arange(SC.ROW, device=DEV)[None, :] >= _dev(SIZES)[:, None]
    want[tail] = sentinel_words(1, wdt)[0]
    if ft == 0:
        _call(N, ws, "dietgpu_ans_decode_batch_stride", 10, int(checksum), nb, arch.data_ptr(), stride, out.data_ptr(),
              SC.ROW, SC.ROW, ok.data_ptr(), sz.data_ptr())
    else:
        _call(N, ws, "dietgpu_float_decompress_batch_stride", ft, 10, int(checksum), nb, arch.data_ptr(), stride,
              out.data_ptr(), SC.ROW * WORD_BYTES[ft], SC.ROW, ok.data_ptr(), sz.data_ptr())
    _check_status(name, ok, sz, want_ok, want_sz)
    for i in SC.named_members(nb):
        assert torch.equal(out[i], want[which[i]]), f"{name}: row {i} (content {which[i]}) is not the element"
    rows = (out != want[which_dev]).any(1).nonzero().view(-1)
    assert rows.numel() == 0, f"{name}: {rows.numel()} rows differ, first {rows[:8].tolist()}"


# ------------------------------------------------------------- 4: range decode ----

def _range_test(N, ws, name, entry, head, ft, nb, words, ins):
    firsts, counts = SC.member_ranges(nb)
    p = Placed(TORCH_WORD[ft], counts)
    for c in range(K7):
        m = np.arange(c, nb, K7)
        p.put(p.want, m, words[c], firsts[m], counts[m])
    ok, sz = _status(nb)
    f32, c32 = firsts.astype(np.uint32), counts.astype(np.uint32)
    _call(N, ws, entry, *head, nb, ins.ctypes.data, f32.ctypes.data, c32.ctypes.data, p.ptrs.ctypes.data,
          ok.data_ptr(), sz.data_ptr())
    _check_status(name, ok, sz, np.ones(nb, dtype=np.int64), counts)
    p.check(name)


@pytest.mark.parametrize("name,ft,nb", SC.RANGE, ids=SC.ids(SC.RANGE))
def test_range_decode(C, N, ws, name, ft, nb):
    """k_decode's range form: member i reads range i // 7 of its content's
    edge ranges (sparse_range_cases.edge_ranges) out of one of the seven
    archives.  Footprint: two placed buffers of about nb x 1,000 words."""
    words = _inputs("dense", ft)[0]
    addrs = _archives("dense", ft)[2]
    which, _ = _which(nb)
    entry, head = ("dietgpu_ans_decode_batch_range", (10,)) if ft == 0 else ("dietgpu_float_decompress_range",
                                                                              (ft, 10))
    _range_test(N, ws, name, entry, head, ft, nb, words, addrs[which])


# --------------------------------------------------------- 5: decode-accumulate ----

def _accumulate_test(N, ws, name, entry, kind, ft, mode, nb, rows):
    acc_t = A.acc_dtype(ft, mode)
    acc_ft = 3 if mode == 2 else ft
    which, _ = _which(nb, True)  # with the empty members
    addrs = _archives(kind, ft)[2]
    p = Placed(SIGNED[acc_t.itemsize], SIZES[which])
    for c in range(K7):  # (an empty member has no accumulator words)
        acc = SC.bit_words(SC.acc_values(ft, mode, SC.acc_which(c), sparse=kind == "sparse"))
        p.put(p.buf, np.flatnonzero(which == c), acc, 0, SC.SIZES[c])
    p.put_rows(p.want, [SC.bit_words(r) for r in rows], which)
    ok, sz = _status(nb)
    ins = addrs[which]
    _call(N, ws, entry, ft, 10, nb, ins.ctypes.data, p.ptrs.ctypes.data, p.caps32.ctypes.data, acc_ft,
          ok.data_ptr(), sz.data_ptr())
    _check_status(name, ok, sz, np.ones(nb, dtype=np.int64), SIZES[which])
    p.check(name)


@pytest.mark.parametrize("name,ft,mode,nb", SC.ACCUMULATE, ids=SC.ids(SC.ACCUMULATE))
def test_decode_accumulate(C, N, ws, name, ft, mode, nb):
    """k_decode's two accumulate forms, bit-exact against
    accumulate_cases.model; member i's accumulator starts as values
    (i + 3) % 7.  Footprint: two placed buffers of nb x about 1,530
    accumulator words (fp32: 2 x 0.4 GB)."""
    _accumulate_test(N, ws, name, "dietgpu_float_decompress_accumulate", "dense", ft, mode, nb,
                     SC.accumulate_rows(ft, mode))


# ------------------------------------------------------------ 6: fused reduce ----

def _reduce_test(C, N, ws, name, entry, kind, ft, K, nb, rows, family, launches):
    """family, launches: the profile family of the reduce's own launches and
    how many of them the call must make, so that the test says which passes
    and slices it ran."""
    which, _ = _which(nb)
    ins = np.concatenate([_archives(kind, ft, src=k)[2][which] for k in range(K)])
    init = Placed(torch.int32, SIZES[which])  # fp32 inits: the call must leave them as they are
    out = Placed(TORCH_WORD[ft], SIZES[which])
    for c in range(K7):
        m = np.arange(c, nb, K7)
        acc = SC.bit_words(SC.acc_values(ft, SR.acc_mode(ft), SC.acc_which(c), sparse=kind == "sparse"))
        for target in (init.buf, init.want):
            init.put(target, m, acc, 0, SC.SIZES[c])
    out.put_rows(out.want, [SC.bit_words(r) for r in rows], which)
    ok, sz = _status(nb)
    C.profile_filter(family)
    C.profile(True)
    C.profile_reset()
    try:
        _call(N, ws, entry, ft, 10, nb, K, ins.ctypes.data, init.ptrs.ctypes.data, 3, out.ptrs.ctypes.data,
              out.caps32.ctypes.data, ft, ok.data_ptr(), sz.data_ptr())
        got = C.profile_query(family)[1]
    finally:
        C.profile(False)
        C.profile_filter(None)
    assert got == launches, f"{name}: {got} launches of the {family} family, expected {launches}"
    _check_status(name, ok, sz, np.ones(nb, dtype=np.int64), SIZES[which])
    out.check(name)
    init.check(name + " (inits)")


@pytest.mark.parametrize("name,per_launch,nb", SC.REDUCE, ids=SC.ids(SC.REDUCE))
def test_fused_reduce(C, N, ws, name, per_launch, nb):
    """k_reduce at three bf16 sources and fp32 inits, in one pass and (two
    sources per launch) in two, whose fp32 partial rows of the members past
    65,535 are written and read back.  The launch count (one per pass and
    slice) and the arena's high-water mark (the partial: every member's words
    rounded up to 4, as fp32, 0.4 GB) say which of the two ran.  Footprint: a
    placed fp32 buffer and a placed bf16 one, each with its expected copy
    (1.2 GB), and the partial."""
    passes = 1 if per_launch == 0 else -(-SC.REDUCE_K // per_launch)
    slices = -(-nb // SC.GRID_Y)
    which, _ = _which(nb)
    partial = 4 * int((-(-SIZES[which] // 4) * 4).sum())
    C.set_reduce_max_sources(per_launch)
    try:
        _reduce_test(C, N, ws, name, "dietgpu_float_reduce", "dense", 2, SC.REDUCE_K, nb,
                     SC.reduce_rows(2, SC.REDUCE_K), "reduce", passes * slices)
    finally:
        C.set_reduce_max_sources(0)
    used = ws.max_usage()  # of that call alone (_call)
    assert (used >= partial) == (passes > 1), f"{name}: {used} B of the arena, a partial is {partial} B"


# ------------------------------------------------------------ 7: sparse codec ----

@pytest.mark.parametrize("name,ft,nb", SC.SPARSE_COMPRESS, ids=SC.ids(SC.SPARSE_COMPRESS))
def test_sparse_compress(C, N, ws, name, ft, nb):
    """k_sparseCount and its gather, then the dense compressor on the nonzero
    lists; oracle-identical.  Footprint: nb rows of the largest member's bound
    (_archive_rows plus the bitmap: bf16 37.5 GB, fp32 38 GB)."""
    refs = _archives("sparse", ft)[0]
    cols = C.max_sparse_float_compressed_size(ft, SC.ROW)
    out, sizes = _compress_pointer(N, ws, "dietgpu_float_compress_sparse", ft, _inputs("sparse", ft)[2], nb, False,
                                   cols)
    _check_archives(name, out, sizes, refs, nb, empty=True)


@pytest.mark.parametrize("name,ft,nb", SC.SPARSE_DECOMPRESS, ids=SC.ids(SC.SPARSE_DECOMPRESS))
def test_sparse_decompress(C, N, ws, name, ft, nb):
    """k_sparseChunks and k_sparseExpand's store form (behind the dense decode
    of the lists).  Footprint: two placed buffers of nb x about 1,530 words."""
    words = _inputs("sparse", ft)[0]
    addrs = _archives("sparse", ft)[2]
    which, _ = _which(nb, True)  # with the empty members
    p = Placed(TORCH_WORD[ft], SIZES[which])
    p.put_rows(p.want, words, which)
    ok, sz = _status(nb)
    ins = addrs[which]
    _call(N, ws, "dietgpu_float_decompress_sparse", ft, 10, 0, nb, ins.ctypes.data, p.ptrs.ctypes.data,
          p.caps32.ctypes.data, ok.data_ptr(), sz.data_ptr())
    _check_status(name, ok, sz, np.ones(nb, dtype=np.int64), SIZES[which])
    p.check(name)


@pytest.mark.parametrize("name,ft,mode,nb", SC.SPARSE_ACCUMULATE, ids=SC.ids(SC.SPARSE_ACCUMULATE))
def test_sparse_accumulate(C, N, ws, name, ft, mode, nb):
    """k_sparseExpand's accumulate form, bit-exact against
    sparse_accumulate_cases.expected (the words under clear bits keep their
    bits).  Footprint: as test_decode_accumulate."""
    _accumulate_test(N, ws, name, "dietgpu_float_decompress_sparse_accumulate", "sparse", ft, mode, nb,
                     SC.sparse_accumulate_rows(ft, mode))


@pytest.mark.parametrize("name,ft,nb", SC.SPARSE_RANGE, ids=SC.ids(SC.SPARSE_RANGE))
def test_sparse_range(C, N, ws, name, ft, nb):
    """k_sparseRangeChunks, sliced over the distinct archives, and
    k_sparseExpandRange: every member reads its own copy of its content's
    archive (nb addresses, back to back in one buffer).  Footprint: the copies
    (40 MB) and two placed buffers of about nb x 1,000 words."""
    words = _inputs("sparse", ft)[0]
    refs = _archives("sparse", ft)[0]
    which, _ = _which(nb)
    lens = np.array([r.size for r in refs], dtype=np.int64)
    room = -(-lens[which] // 16) * 16
    at = np.concatenate([[0], np.cumsum(room)[:-1]])
    copies = torch.zeros([int(room.sum()) + 16], dtype=torch.uint8, device=DEV)
    assert copies.data_ptr() % 16 == 0
    for c in range(K7):
        scatter_rows(copies, _dev(at[np.arange(c, nb, K7)]), 0, int(lens[c]), _dev(refs[c]))
    ins = host_ptrs(copies.data_ptr(), at, 1)
    assert np.unique(ins).size == nb
    _range_test(N, ws, name, "dietgpu_float_decompress_sparse_range", (ft, 10), ft, nb, words, ins)


@pytest.mark.parametrize("name,nb", SC.SPARSE_REDUCE, ids=SC.ids(SC.SPARSE_REDUCE))
def test_sparse_reduce(C, N, ws, name, nb):
    """k_sparseReduce at four bf16 sources and fp32 inits.  Its chunk count
    (k_sparseChunks) runs over sources x members rows: 65,536 and 65,540 of
    them at 16,384 and 16,385 members, 262,148 at 65,537, where the reduce
    itself is sliced too.  The launches of the sparse_reduce family, one per
    slice of the chunk count and one per slice of k_sparseReduce in each pass,
    say that one pass took all four sources (two passes of two sources would
    count 32,768 rows each, unsliced): 2 + 1 at 16,384 and 16,385 members,
    5 + 2 at 65,537.  Footprint: as test_fused_reduce, and up to 2.2 GB of
    list rows in the arena."""
    rows = SC.INNER_K * nb  # of the one pass
    launches = -(-rows // SC.GRID_Y) + -(-nb // SC.GRID_Y)
    assert launches == {16384: 3, 16385: 3, 65537: 7}[nb]
    _reduce_test(C, N, ws, name, "dietgpu_float_reduce_sparse", "sparse", 2, SC.INNER_K, nb,
                 SC.sparse_reduce_rows(2, SC.INNER_K), "sparse_reduce", launches)


# ------------------------------------------------- 8: info readouts, operator ----

def test_compressed_info(C, N, ws):
    """ans / float compressed-info over 65,537 archives: the uploaded pointer
    column and one output row per member.  Footprint: under 1 MB."""
    nb = SC.INFO_NB
    which, _ = _which(nb)
    words = _inputs("dense", 0)[0]
    refs, _, addrs = _archives("dense", 0, True)
    ins = addrs[which]
    _, sz = _status(nb)
    ck = torch.full([nb], -7, dtype=torch.int32, device=DEV)
    _call(N, ws, "dietgpu_ans_get_compressed_info", ins.ctypes.data, nb, sz.data_ptr(), ck.data_ptr())
    want_ck = np.array([int(O.checksum(w)) for w in words], dtype=np.int64)[which]
    one = np.ones(nb, dtype=np.int64)
    _check_status("ans info", torch.ones_like(sz), sz, one, SIZES[which])  # (no status: sizes only)
    got = ck.cpu().numpy().astype(np.int64) & 0xffffffff
    bad = np.flatnonzero(got != want_ck)
    assert bad.size == 0, f"ans info: checksums of {bad.size} members are wrong, first {bad[:8].tolist()}"

    for ft in (2, 4):
        refs, _, addrs = _archives("dense", ft, True)
        ins = addrs[which]
        _, sz = _status(nb)
        ty = torch.full([nb], -7, dtype=torch.int32, device=DEV)
        ck = torch.full([nb], -7, dtype=torch.int32, device=DEV)
        _call(N, ws, "dietgpu_float_get_compressed_info", ins.ctypes.data, nb, sz.data_ptr(), ty.data_ptr(),
              ck.data_ptr())
        _check_status(f"float info {ft}", (ty == ft).int(), sz, one, SIZES[which])  # status: the type is ft
        want_ck = np.array([int(r[12:16].view(np.uint32)[0]) for r in refs], dtype=np.int64)[which]
        got = ck.cpu().numpy().astype(np.int64) & 0xffffffff
        bad = np.flatnonzero(got != want_ck)
        assert bad.size == 0, f"float info {ft}: checksums of {bad.size} members are wrong, first {bad[:8].tolist()}"


def test_operator_round_trip(C, N, ws):
    """torch.ops.dietgpu.compress_data and decompress_data on 65,537 bf16
    tensors: the op layer's member table and the uploaded columns at that
    size.  Footprint: the archive matrix the operator allocates (37.5 GB) and
    two placed buffers of nb x about 1,530 words."""
    nb = SC.OP_NB
    ft = 2
    which, _ = _which(nb)
    words, views, _ = _inputs("dense", ft)
    refs = _archives("dense", ft)[0]
    xs = [v.view(torch.bfloat16) for v in views]
    comp, sizes, _ = torch.ops.dietgpu.compress_data(True, [xs[c] for c in which.tolist()], False, ws.buf)
    _ROWS.append(comp)
    torch.cuda.synchronize()
    _check_archives("compress_data", comp, sizes, refs, nb)

    p = Placed(TORCH_WORD[ft], SIZES[which])
    p.put_rows(p.want, words, which)
    lens = [r.size for r in refs]
    flat = p.buf.view(torch.bfloat16)
    rows = [comp[i, : lens[c]] for i, c in enumerate(which.tolist())]
    outs = [flat[s: s + n] for s, n in zip(p.starts.tolist(), p.caps.tolist())]
    ok, sz = _status(nb)
    torch.ops.dietgpu.decompress_data(True, rows, outs, False, ws.buf, ok, sz)
    torch.cuda.synchronize()
    _check_status("decompress_data", ok, sz, np.ones(nb, dtype=np.int64), SIZES[which])
    p.check("decompress_data")
