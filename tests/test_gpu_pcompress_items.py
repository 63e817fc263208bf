"""Item descriptors of the single-pass compressor (csrc/pcompress.h): an item
is decoded once into an LDS record (element, sizes, addresses, block sizes)
and every later use reads the record; the workgroup's team coordinates are
computed once; each hand-off window reads the kernel arguments once.  The
shapes below are the smallest that reach each descriptor path:

* four rounds of single-item teams (3 x the resident grid + 5 elements), so
  rounds 2 and 3 take their element from the dequeue log, with sizes on every
  block edge (0, 1, 7, 4095, 4096, 4097, 32768 words);
* teams of 5 items with idle members (elements of 5 items, 1 block, 9 blocks
  and 0 words), enough elements that the third round comes from the log and
  the last teams get none, in fp16, fp32 and bytes with the checksum;
* the same teams through every batch descriptor: pointer API with the tables
  inline in the kernel arguments (<= 400 elements) and in device memory
  (> 400), split sizes, and a stride with one fixed size;
* a team-5 call and a team-1 call back to back on one stream (a record or an
  argument surviving a call would show).

Every archive is compared byte for byte (and by size) with the CPU oracle's,
decoded back bit-exactly, and neither the device error count nor the team
barrier's fallback count may move."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, Cache, single_pass_fixture, workspace_fixture  # noqa: F401
from tests.util import NP_W, exp_bytes, float_words

pytestmark = pytest.mark.gpu

PB = 10
BUDGET_TICKS = 500_000  # 5 ms: a co-tenant cannot trip the no-fallback assertion

# teams of 5 items (32768 words each): 5 items whose last holds 2 blocks,
# 1 block, 9 blocks (a second member with one block, the rest none), nothing.
# Multiples of 16 words, so split sizes keep every element 16 B-aligned; the
# other modes add TEAM_ODD to leave the block and vector edges.
TEAM_SIZES = (4 * 32768 + 4096 + 96, 2992, 8 * 4096 + 16, 0)
TEAM_ODD = (5, 3, 1, 0)
EDGE_SIZES = (0, 1, 7, 4095, 4096, 4097, 32768)
POOL = 1 << 18


_single_pass = single_pass_fixture()


@pytest.fixture(autouse=True)
def _barrier_budget(C, _single_pass):
    """On the single-pass path, with a team-barrier budget of BUDGET_TICKS."""
    C.set_barrier_budget(BUDGET_TICKS)
    try:
        yield
    finally:
        C.set_barrier_budget(20000)


ws = workspace_fixture(768 << 20)


@pytest.fixture(scope="module")
def slots():
    """Resident workgroups of k_pcompress: 4 per CU (its LDS and VGPRs)."""
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


_pools, _refs = Cache(), Cache()


def _pool(ft):
    return _pools.get(ft, lambda: (exp_bytes(POOL, lam=20.0, seed=41) if ft == 0
                                   else float_words(ft, POOL, seed=40 + ft)))


def _elem(ft, k, n):
    """Element k of n words: one of 8 windows of the pool (so the oracle runs
    on a handful of distinct elements, once per module)."""
    off = (k % 8) * 4099
    return off, _pool(ft)[off: off + n]


def _ref(ft, ck, off, n):
    def make():
        w = _pool(ft)[off: off + n]
        return O.ans_encode(w, PB, ck) if ft == 0 else O.float_compress(w, ft, PB, ck)
    return _refs.get((ft, ck, off, n), make)


class Batch:
    """nb elements laid out 16 B-aligned in one device buffer, with their
    archive rows and decode buffer."""

    def __init__(self, C, ft, sizes):
        self.ft, self.sizes, self.nb = ft, list(sizes), len(sizes)
        wb = np.dtype(NP_W[ft]).itemsize
        al = 16 // wb
        self.offs, o = [], 0
        for n in self.sizes:
            self.offs.append(o)
            o += -(-n // al) * al
        flat = np.zeros(max(o, al), dtype=NP_W[ft])
        self.src = []
        for k, (n, at) in enumerate(zip(self.sizes, self.offs)):
            off, w = _elem(ft, k, n)
            flat[at: at + n] = w
            self.src.append(off)
        self.host = flat
        self.x = torch.from_numpy(flat.view(np.dtype(f"i{wb}") if wb > 1 else np.uint8)).to(DEV)
        nmax = max(self.sizes)
        cols = C.max_compressed_size(nmax) if ft == 0 else C.max_float_compressed_size(ft, nmax)
        self.cols = -(-cols // 16) * 16
        self.out = torch.zeros([self.nb, self.cols], dtype=torch.uint8, device=DEV)
        self.csz = torch.zeros([self.nb], dtype=torch.int32, device=DEV)
        self.wb = wb

    def in_ptrs(self):
        return [self.x.data_ptr() + at * self.wb for at in self.offs]

    def out_ptrs(self):
        return [self.out.data_ptr() + i * self.cols for i in range(self.nb)]


def _compress(C, ws, b, mode, ck):
    from dietgpu_fork_amd import _native as N

    L, s = N.lib(), C._s()
    if mode == "pointer":
        ins, outs, szs = N.ptr_array(b.in_ptrs()), N.ptr_array(b.out_ptrs()), N.u32_array(b.sizes)
        if b.ft == 0:
            rc = L.dietgpu_ans_encode_batch_pointer(ws.h, PB, int(ck), b.nb, ins, szs, None, outs,
                                                    b.csz.data_ptr(), s)
        else:
            rc = L.dietgpu_float_compress(ws.h, b.ft, PB, int(ck), b.nb, ins, szs, outs, b.csz.data_ptr(), s)
    elif mode == "split":
        szs = N.u32_array(b.sizes)
        if b.ft == 0:
            rc = L.dietgpu_ans_encode_batch_split_size(ws.h, PB, int(ck), b.nb, b.x.data_ptr(), szs, None,
                                                       b.out.data_ptr(), b.cols, b.csz.data_ptr(), s)
        else:
            rc = L.dietgpu_float_compress_split_size(ws.h, b.ft, PB, int(ck), b.nb, b.x.data_ptr(), szs,
                                                     b.out.data_ptr(), b.cols, b.csz.data_ptr(), s)
    else:
        assert mode == "stride" and b.ft != 0 and len(set(b.sizes)) == 1
        n = b.sizes[0]
        stride = (b.offs[1] - b.offs[0]) if b.nb > 1 else n
        rc = L.dietgpu_float_compress_batch_stride(ws.h, b.ft, PB, int(ck), b.nb, b.x.data_ptr(), n,
                                                   stride * b.wb, b.out.data_ptr(), b.cols, b.csz.data_ptr(), s)
    N.check(rc)


def _check(C, ws, b, ck):
    """Archives and sizes against the oracle, then the decode."""
    from dietgpu_fork_amd import _native as N

    torch.cuda.synchronize()
    assert C.barrier_fallback_count(reset=True) == 0
    assert C.device_error_count(reset=True) == 0
    sizes = b.csz.cpu().tolist()
    host = b.out.cpu().numpy()
    for i, (n, off) in enumerate(zip(b.sizes, b.src)):
        ref = _ref(b.ft, ck, off, n)
        assert sizes[i] == ref.size, (i, n, sizes[i], ref.size)
        assert np.array_equal(host[i, : ref.size], ref), f"element {i} ({n} words)"
    y = torch.zeros_like(b.x)
    ok = torch.zeros([b.nb], dtype=torch.uint8, device=DEV)
    sz = torch.zeros([b.nb], dtype=torch.int32, device=DEV)
    ins = N.ptr_array(b.out_ptrs())
    outs = N.ptr_array([y.data_ptr() + at * b.wb for at in b.offs])
    caps = N.u32_array(b.sizes)
    L, s = N.lib(), C._s()
    if b.ft == 0:
        rc = L.dietgpu_ans_decode_batch_pointer(ws.h, PB, int(ck), b.nb, ins, outs, caps, ok.data_ptr(),
                                                sz.data_ptr(), s)
    else:
        rc = L.dietgpu_float_decompress(ws.h, b.ft, PB, int(ck), b.nb, ins, outs, caps, ok.data_ptr(),
                                        sz.data_ptr(), s)
    N.check(rc)
    torch.cuda.synchronize()
    assert bool((ok == 1).all())
    assert sz.cpu().tolist() == b.sizes
    assert torch.equal(y, b.x)


def _reset(C):
    C.device_error_count(reset=True)
    C.barrier_fallback_count(reset=True)


def _team_sizes(nb, odd):
    return [TEAM_SIZES[k % 4] + (TEAM_ODD[k % 4] if odd else 0) for k in range(nb)]


def _team_count(slots):
    """Elements for three rounds of 5-item teams, XCD-aligned (teams per round
    a multiple of 8 within the resident grid): round 2 comes from the log and
    its last three teams find no element."""
    t8 = slots // 5 // 8 * 8
    assert t8 >= 8
    return 3 * t8 - 3


def test_four_rounds_team_one(C, ws, slots):
    nb = 3 * slots + 5
    b = Batch(C, 2, [EDGE_SIZES[k % len(EDGE_SIZES)] for k in range(nb)])
    _reset(C)
    _compress(C, ws, b, "pointer", False)
    _check(C, ws, b, False)


@pytest.mark.parametrize("ft,ck", [(1, False), (3, False), (0, True)], ids=["fp16", "fp32", "bytes-ck"])
def test_teams_with_idle_members(C, ws, slots, ft, ck):
    b = Batch(C, ft, _team_sizes(_team_count(slots), odd=True))
    _reset(C)
    _compress(C, ws, b, "pointer", ck)
    _check(C, ws, b, ck)


@pytest.mark.parametrize("mode", ["inline", "device-tables", "split", "stride"])
def test_teams_descriptor_modes(C, ws, slots, mode):
    nb = _team_count(slots)
    if mode == "inline":
        b = Batch(C, 2, _team_sizes(min(nb, 396), odd=True))  # <= 400 elements: tables in the kernel arguments
    elif mode == "device-tables":
        assert nb > 400
        b = Batch(C, 2, _team_sizes(nb, odd=True))
    elif mode == "split":
        b = Batch(C, 2, _team_sizes(nb, odd=False))
    else:
        b = Batch(C, 2, [TEAM_SIZES[0] + TEAM_ODD[0]] * nb)
    _reset(C)
    _compress(C, ws, b, {"inline": "pointer", "device-tables": "pointer"}.get(mode, mode), False)
    _check(C, ws, b, False)


def test_team_five_then_team_one_back_to_back(C, ws, slots):
    b5 = Batch(C, 2, _team_sizes(_team_count(slots), odd=True))
    b1 = Batch(C, 2, [EDGE_SIZES[k % len(EDGE_SIZES)] for k in range(3 * slots + 5)])
    _reset(C)
    _compress(C, ws, b5, "pointer", False)
    _compress(C, ws, b1, "pointer", False)
    torch.cuda.synchronize()
    assert C.barrier_fallback_count(reset=False) == 0
    assert C.device_error_count(reset=False) == 0
    _check(C, ws, b5, False)
    _check(C, ws, b1, False)
