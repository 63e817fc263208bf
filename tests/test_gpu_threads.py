"""The host-thread contract with real codec calls:
concurrent calls on different streams, concurrent calls on ONE stream from
several host threads (serialised in stream order), and the per-thread stream
handle, whose synchronisation arena is keyed per host thread.  What exists
only for these cases runs here: the per-stream arena lock held until launch
(csrc/sync_arena.cpp), the per-thread key, the staging ring's mutex
(csrc/stack_memory.cpp), the mutex of the per-device caches and the
thread-local error string.

The main thread prepares every worker's inputs, the oracle's archives and what
every output must hold, all on the device, before the workers start.  A worker
fills its outputs with SENTINEL, issues a whole round without synchronising,
synchronises its stream once and compares on the device: archives with the
oracle's bytes and sizes, decodes with the inputs, placed buffers whole."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, N, SENTINEL, Cache, pack_bytes, sentinel_words, word_starts  # noqa: F401
from tests.thread_harness import run_workers
from tests.util import float_words, sparsify

pytestmark = pytest.mark.gpu

ROUNDS = 25
SIZES = [300000, 70001, 4097]  # bf16 words; 16 B-aligned they take the single-pass compressor
SPARSE_N = 40000               # fp32 words, 90 % zeros: batch 1, a rows lease
RANGE_N, RANGE_ROWS, RANGE_W = 64000, 4000, 16  # 4,000 members: a 96,000 B table, through the staging ring
ROW_PITCH = RANGE_W + 8        # words between the range decode's rows (8 sentinel words after each)
PER_THREAD_STREAM = 2          # hipStreamPerThread as a handle (hip_runtime_api.h)

_host = Cache()


def host_data(seed):
    """A worker's words and the oracle's archives of them (numpy, computed once)."""
    def make():
        words = [float_words(2, n, seed=1000 * seed + i) for i, n in enumerate(SIZES)]
        sp = sparsify(float_words(3, SPARSE_N, seed=1000 * seed + 7), frac_zero=0.9, seed=1000 * seed + 8)
        rw = float_words(2, RANGE_N, seed=1000 * seed + 9)
        return dict(words=words, refs=[O.float_compress(w, 2) for w in words], sp=sp, sp_ref=O.sparse_compress(sp, 3),
                    rw=rw, rw_ref=O.float_compress(rw, 2))

    return _host.get(seed, make)


def dev_bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


class Placed:
    """Destinations of `caps` words each in one sentinel buffer (word_starts),
    and the buffer as it must be once `words` have been decoded into them."""

    def __init__(self, dtype, npdtype, caps, offs, words):
        self.starts, total = word_starts(dtype, caps, offs)
        want = np.full(total * dtype.itemsize, SENTINEL, dtype=np.uint8).view(npdtype)
        for st, w in zip(self.starts, words):
            want[st:st + w.size] = w.view(npdtype)
        self.want = torch.from_numpy(want).to(DEV)
        self.buf = sentinel_words(total, dtype)
        self.ptrs = [self.buf.data_ptr() + st * dtype.itemsize for st in self.starts]

    def fill(self):
        self.buf.view(torch.uint8).fill_(SENTINEL)


class Job:
    """Everything one worker touches, made by the main thread."""

    def __init__(self, N, C, seed):
        self.N, self.L = N, N.lib()
        h = host_data(seed)
        self.ws = C.Workspace(128 << 20)
        nb = len(SIZES)
        # the same words 16 B-aligned and one word off (the fused three-kernel path)
        stride = max(SIZES) + 64
        self.x = {}
        for key, off in (("aligned", 0), ("unaligned", 1)):
            host = np.zeros(nb * stride + 8, dtype=np.uint16)
            for i, w in enumerate(h["words"]):
                host[i * stride + off:i * stride + off + w.size] = w
            x = torch.from_numpy(host.view(np.int16).copy()).to(DEV)
            assert x.data_ptr() % 16 == 0
            self.x[key] = (x, N.ptr_array([x.data_ptr() + 2 * (i * stride + off) for i in range(nb)]))
        self.in_size = N.u32_array(SIZES)
        self.cols = self.L.dietgpu_get_max_float_compressed_size(2, max(SIZES))
        self.out = {k: torch.empty([nb, self.cols], dtype=torch.uint8, device=DEV) for k in self.x}
        self.out_ptrs = {k: N.ptr_array([o.data_ptr() + i * self.cols for i in range(nb)]) for k, o in self.out.items()}
        self.out_sizes = {k: torch.empty([nb], dtype=torch.int32, device=DEV) for k in self.x}
        self.refs = [dev_bytes(r) for r in h["refs"]]
        self.ref_sizes = torch.tensor([r.size for r in h["refs"]], dtype=torch.int32, device=DEV)
        # batch-1 sparse fp32
        self.sp_x = torch.from_numpy(h["sp"].view(np.int32).copy()).to(DEV)
        self.sp_cols = self.L.dietgpu_get_max_sparse_float_compressed_size(3, SPARSE_N)
        self.sp_out = torch.empty([1, self.sp_cols], dtype=torch.uint8, device=DEV)
        self.sp_out_size = torch.empty([1], dtype=torch.int32, device=DEV)
        self.sp_ref = dev_bytes(h["sp_ref"])
        self.sp_ref_size = torch.tensor([h["sp_ref"].size], dtype=torch.int32, device=DEV)
        self.sp_args = (N.ptr_array([self.sp_x.data_ptr()]), N.u32_array([SPARSE_N]),
                        N.ptr_array([self.sp_out.data_ptr()]))
        # decodes of the oracle's archives
        self.archives = pack_bytes(h["refs"] + [h["sp_ref"], h["rw_ref"]], [0] * (nb + 2))
        self.dec = Placed(torch.int16, np.int16, SIZES, [0, 1, 0], h["words"])
        self.dec_args = (N.ptr_array([a.data_ptr() for a in self.archives[:nb]]), N.ptr_array(self.dec.ptrs),
                         N.u32_array(SIZES))
        self.sp_dec = Placed(torch.int32, np.int32, [SPARSE_N], [0], [h["sp"]])
        self.sp_dec_args = (N.ptr_array([self.archives[nb].data_ptr()]), N.ptr_array(self.sp_dec.ptrs),
                            N.u32_array([SPARSE_N]))
        # rows m * 16 .. m * 16 + 15 of one archive, ROW_PITCH words apart
        rows = h["rw"].reshape(RANGE_ROWS, RANGE_W)
        self.rng_dec = Placed(torch.int16, np.int16, [RANGE_ROWS * ROW_PITCH], [0], [])
        st = self.rng_dec.starts[0]
        want = self.rng_dec.want[st:st + RANGE_ROWS * ROW_PITCH].view(RANGE_ROWS, ROW_PITCH)
        want[:, :RANGE_W] = torch.from_numpy(rows.view(np.int16).copy()).to(DEV)
        base = self.rng_dec.ptrs[0]
        self.rng_cols = (np.full(RANGE_ROWS, self.archives[nb + 1].data_ptr(), dtype=np.uint64),
                         np.arange(RANGE_ROWS, dtype=np.uint32) * np.uint32(RANGE_W),
                         np.full(RANGE_ROWS, RANGE_W, dtype=np.uint32),
                         np.uint64(base) + np.arange(RANGE_ROWS, dtype=np.uint64) * np.uint64(2 * ROW_PITCH))
        assert self.rng_cols[0].nbytes + self.rng_cols[1].nbytes + self.rng_cols[2].nbytes + self.rng_cols[3].nbytes \
            == 96000
        # status of the three decodes: 7 / -7 are values no call reports
        self.ok = {k: torch.empty([n], dtype=torch.uint8, device=DEV)
                   for k, n in (("dec", nb), ("sp", 1), ("rng", RANGE_ROWS))}
        self.sz = {k: torch.empty([v.numel()], dtype=torch.int32, device=DEV) for k, v in self.ok.items()}
        self.want_sz = {"dec": torch.tensor(SIZES, dtype=torch.int32, device=DEV),
                        "sp": torch.tensor([SPARSE_N], dtype=torch.int32, device=DEV),
                        "rng": torch.full([RANGE_ROWS], RANGE_W, dtype=torch.int32, device=DEV)}

    def fill(self):
        """Every output as no call leaves it (on the current torch stream)."""
        for o in list(self.out.values()) + list(self.out_sizes.values()) + [self.sp_out, self.sp_out_size]:
            o.view(torch.uint8).fill_(SENTINEL)
        for p in (self.dec, self.sp_dec, self.rng_dec):
            p.fill()
        for k in self.ok:
            self.ok[k].fill_(7)
            self.sz[k].fill_(-7)

    def issue(self, stream, everything=True):
        """One round on the stream handle `stream`, nothing synchronised."""
        N, L, h = self.N, self.L, self.ws.h
        for k in ("aligned", "unaligned"):
            N.check(L.dietgpu_float_compress(h, 2, 10, 0, len(SIZES), self.x[k][1], self.in_size, self.out_ptrs[k],
                                             self.out_sizes[k].data_ptr(), stream))
        if everything:
            N.check(L.dietgpu_float_compress_sparse(h, 3, 10, 0, 1, *self.sp_args, self.sp_out_size.data_ptr(), stream))
        N.check(L.dietgpu_float_decompress(h, 2, 10, 0, len(SIZES), *self.dec_args, self.ok["dec"].data_ptr(),
                                           self.sz["dec"].data_ptr(), stream))
        if everything:
            N.check(L.dietgpu_float_decompress_sparse(h, 3, 10, 0, 1, *self.sp_dec_args, self.ok["sp"].data_ptr(),
                                                      self.sz["sp"].data_ptr(), stream))
            c = self.rng_cols
            N.check(L.dietgpu_float_decompress_range(h, 2, 10, RANGE_ROWS, c[0].ctypes.data, c[1].ctypes.data,
                                                     c[2].ctypes.data, c[3].ctypes.data, self.ok["rng"].data_ptr(),
                                                     self.sz["rng"].data_ptr(), stream))

    def verify(self, where, everything=True):
        """After the round's one synchronisation: compares on the device."""
        for k in ("aligned", "unaligned"):
            assert torch.equal(self.out_sizes[k], self.ref_sizes), (where, k, self.out_sizes[k].tolist())
            for i, ref in enumerate(self.refs):
                assert torch.equal(self.out[k][i, :ref.numel()], ref), (where, k, f"archive {i} differs from the oracle's")
        kinds = [("dec", self.dec)] + ([("sp", self.sp_dec), ("rng", self.rng_dec)] if everything else [])
        if everything:
            assert torch.equal(self.sp_out_size, self.sp_ref_size), (where, "sparse", self.sp_out_size.tolist())
            assert torch.equal(self.sp_out[0, :self.sp_ref.numel()], self.sp_ref), (where, "sparse archive")
        for k, placed in kinds:
            assert bool((self.ok[k] == 1).all()), (where, k, "status")
            assert torch.equal(self.sz[k], self.want_sz[k]), (where, k, "sizes")
            assert torch.equal(placed.buf, placed.want), (where, k, "decoded words or a stray write")


@pytest.fixture(scope="module")
def jobs(N, C):
    made = [Job(N, C, seed) for seed in range(4)]
    torch.cuda.synchronize()
    return made


def run_rounds(C, jobs, streams):
    """Worker i runs ROUNDS rounds of jobs[i] on streams[i]."""
    def worker(i):
        job, s = jobs[i], streams[i]
        with torch.cuda.stream(s):
            for r in range(ROUNDS):
                job.fill()
                job.issue(s.cuda_stream)
                s.synchronize()
                job.verify((i, r))

    C.device_error_count(reset=True)
    with C.compress_path("single-pass"):  # process-wide: set before the threads start, restored after they end
        run_workers(worker, len(jobs), timeout=120.0, name="codec")
    torch.cuda.synchronize()
    assert C.device_error_count(reset=True) == 0


def test_four_threads_on_their_own_streams(C, jobs):
    run_rounds(C, jobs, [torch.cuda.Stream() for _ in jobs])


def test_four_threads_on_one_stream(C, jobs):
    """Calls on one stream from several host threads are serialised in stream
    order: each worker has its own workspace and its own outputs, the stream
    and with it the synchronisation arena are shared."""
    shared = torch.cuda.Stream()
    run_rounds(C, jobs, [shared] * len(jobs))


def test_two_threads_on_the_per_thread_stream(C, jobs):
    """The C ABI with the per-thread stream handle as its stream argument: one
    handle, a different stream and a different arena on each host thread.
    Compress and decompress only; torch cannot name that stream, so the device
    is synchronised around the calls."""
    def worker(i):
        job = jobs[i]
        for r in range(ROUNDS):
            job.fill()
            torch.cuda.synchronize()
            job.issue(PER_THREAD_STREAM, everything=False)
            torch.cuda.synchronize()
            job.verify((i, r), everything=False)

    C.device_error_count(reset=True)
    with C.compress_path("single-pass"):
        run_workers(worker, 2, timeout=120.0, name="per-thread")
    torch.cuda.synchronize()
    assert C.device_error_count(reset=True) == 0
