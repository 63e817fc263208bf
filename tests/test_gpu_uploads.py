"""The parameter-table upload (StackDeviceMemory::copyToDevice, through the test
hooks dietgpu_test_upload / dietgpu_test_upload_reset) while the host is ahead
of the GPU, and from several host threads.

Tables of up to 64 KiB ride in kernel arguments, up to 2 MiB they go through a
process-wide 8 MiB pinned staging ring (csrc/staging_plan.h holds its rule,
tests/test_staging_plan.py checks that rule on the CPU), larger ones straight
to the copy engine.  In a codec call a table holds pointers and sizes; here
only bytes move: every upload's source is its own random pattern, every
destination a slice of one buffer whose every other byte is SENTINEL, and the
buffer is compared whole, so the one thing that can go wrong is bytes in
memory the test owns.  The stall is dietgpu_test_occupy: one workgroup that
holds its stream for 300 ms; each test asserts that it was still running where
its premise needs it, and fails (not passes) on a host too slow for that."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests.gpu_harness import DEV, SENTINEL, N, C, placed_mismatch, sentinel_words, word_starts  # noqa: F401
from tests.thread_harness import run_workers

pytestmark = pytest.mark.gpu

MIB = 1 << 20
RING_MIN, RING_MAX = 65540, 2 * MIB  # the first and the last size that goes through the ring
STALL_US = 300000


@pytest.fixture(scope="module")
def T(N):
    return N.testlib()


class Uploads:
    """Sources and destinations of a list of uploads: sizes[i] random bytes
    each (seeded), to 16 B-aligned slices of one sentinel buffer, 16 bytes
    apart at least."""

    def __init__(self, sizes, seed):
        rng = np.random.default_rng(seed)
        self.sizes = list(sizes)
        self.starts, total = word_starts(torch.uint8, self.sizes, [0] * len(self.sizes))
        self.src = [rng.integers(0, 256, n, dtype=np.uint8) for n in self.sizes]
        want = np.full(total, SENTINEL, dtype=np.uint8)
        for st, s in zip(self.starts, self.src):
            want[st:st + s.size] = s
        self.want = torch.from_numpy(want).to(DEV)
        self.buf = sentinel_words(total, torch.uint8)
        assert self.buf.data_ptr() % 16 == 0
        self.base = self.buf.data_ptr()

    def send(self, N, T, i, stream, clobber=False):
        """Upload i on `stream`; clobber: overwrite the host source as soon as
        the call has returned, as a driver's table dies with its call."""
        s = self.src[i]
        N.test_check(T.dietgpu_test_upload(ctypes.c_void_p(self.base + self.starts[i]), ctypes.c_void_p(s.ctypes.data),
                                           s.size, ctypes.c_void_p(stream.cuda_stream)))
        if clobber:
            s.fill(0x5A)

    def check(self):
        problem = placed_mismatch(self.buf, self.want, np.asarray(self.starts))
        assert problem is None, problem


def stall(N, T, stream):
    """-> an event behind a 300 ms kernel on `stream` (one workgroup)."""
    N.test_check(T.dietgpu_test_occupy(ctypes.c_void_p(stream.cuda_stream), STALL_US, 1, 1024))
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def test_wrap_that_skips_a_pending_tail(N, T):
    """Seven 1 MiB uploads and a sync leave the ring's head at 7 MiB.  Behind
    a stall: H of 917,504 B lands in the tail, N1..N7 of 1 MiB wrap to 0 and
    end at 7 MiB, and N8 of 1,310,720 B wraps onto N1 and N2, which are
    pending behind H, the oldest use, in the tail the wrap skipped.  A ring
    that looks only at its oldest use copies N8's bytes over N1 and a quarter
    of N2 before their copies have run."""
    s = torch.cuda.Stream()
    u = Uploads([MIB] * 7 + [917504] + [MIB] * 7 + [1310720], seed=1)
    torch.cuda.synchronize()
    N.test_check(T.dietgpu_test_upload_reset())
    for i in range(7):
        u.send(N, T, i, s)
    s.synchronize()
    ev = stall(N, T, s)
    for i in range(7, 15):
        u.send(N, T, i, s)
    assert not ev.query(), "the stall ended before N8 was issued: the host was too slow for the premise"
    u.send(N, T, 15, s)
    s.synchronize()
    u.check()


def test_every_path_under_a_stall(N, T):
    """The last kernel-argument sizes (4 and 65,536 B), the first and the last
    ring size, the first direct size and 3 MiB, all behind one stall, every
    source overwritten as soon as its call returns.  The kernel-argument and
    ring uploads must return while the stall runs; a direct upload may wait
    for it, but the bytes that arrive are the ones passed in."""
    s = torch.cuda.Stream()
    sizes = [4, 65536, RING_MIN, RING_MAX, RING_MAX + 4, 3 * MIB]
    u = Uploads(sizes, seed=2)
    torch.cuda.synchronize()
    N.test_check(T.dietgpu_test_upload_reset())
    ev = stall(N, T, s)
    for i in range(4):
        u.send(N, T, i, s, clobber=True)
    assert not ev.query(), "the stall ended before the first direct upload: the host was too slow for the premise"
    for i in range(4, 6):
        u.send(N, T, i, s, clobber=True)
    s.synchronize()
    u.check()


def mixed_sizes(rng, count):
    """Sizes of the ring's range: most a few thousand members' worth, some
    large, a few exactly the first and the last ring size."""
    r = rng.random(count)
    small = rng.integers(RING_MIN, 100000, count)
    mid = rng.integers(100000, 400000, count)
    big = rng.integers(400000, RING_MAX + 1, count)
    sizes = np.where(r < 0.8, small, np.where(r < 0.95, mid, big))
    sizes[rng.random(count) < 0.02] = RING_MAX
    sizes[0], sizes[-1] = RING_MIN, RING_MAX
    return [int(v) for v in sizes]


def test_a_stalled_stream_does_not_hold_up_another(N, T):
    """Stream A is stalled with one upload pending in the ring's tail; stream
    B makes 40 uploads of 65,540 B to 2 MiB, several turns of the ring.

    The ring's rule (staging_plan.h, rule 3): an upload never waits for a use
    of another stream while the ring has room elsewhere; it steps over A's
    region.  B does have to see its OWN earlier copies done every time it
    comes round, and whether those run beside A's stall is the HIP runtime's
    business, not the ring's: on MI355X a pinned copy of stream B was
    measured both finishing in 0.26 ms beside A's stall and, in another
    process, held for more than 200 ms behind A's pending copy in the
    runtime's copy queue (a kernel, or a kernel-argument upload, on B was
    never held).  So: every pattern arrives, always.  B's first copy behind
    the stall is the witness; when it runs beside the stall, B's whole loop
    must end while the stall lasts.  When the runtime holds it, no rule of
    the ring can end B's loop early and only the bytes are checked;
    tests/test_staging_plan.py::test_a_stalled_stream_does_not_hold_up_another
    holds the rule itself, without a runtime in between."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ua = Uploads([917504], seed=3)
    rng = np.random.default_rng(5)
    mixed = [RING_MAX if i % 5 == 0 else int(rng.integers(RING_MIN, RING_MAX)) for i in range(40)]
    assert sum(mixed) > 4 * 8 * MIB
    ub = Uploads([MIB] * 7 + mixed, seed=4)
    torch.cuda.synchronize()
    N.test_check(T.dietgpu_test_upload_reset())
    for i in range(7):
        ub.send(N, T, i, b)
    b.synchronize()
    ev = stall(N, T, a)
    ua.send(N, T, 0, a)  # [7 MiB, 7.875 MiB)
    ub.send(N, T, 7, b)
    witness = torch.cuda.Event()
    witness.record(b)
    t0 = time.perf_counter()
    while not witness.query() and time.perf_counter() - t0 < 0.05:  # (0.3 ms when it runs)
        pass
    beside = witness.query() and not ev.query()
    for i in range(8, 47):
        ub.send(N, T, i, b)
    ended_in_stall = not ev.query()
    print(f"stream B's copies ran beside stream A's stall: {beside}; B's loop ended within it: {ended_in_stall}")
    if beside:
        assert ended_in_stall, "stream B's uploads waited for stream A's stall"
    b.synchronize()
    ub.check()
    a.synchronize()
    ua.check()


def test_four_host_threads_four_streams(N, T):
    """Four host threads with a stream each make 200 uploads of 65,540 B to
    2 MiB: the ring's lock, its event pool and its placement under contention
    (about 34 MiB per thread, more than four turns of the ring each)."""
    streams = [torch.cuda.Stream() for _ in range(4)]
    sets = [Uploads(mixed_sizes(np.random.default_rng(50 + t), 200), seed=60 + t) for t in range(4)]
    torch.cuda.synchronize()
    N.test_check(T.dietgpu_test_upload_reset())

    def worker(t):
        u, s = sets[t], streams[t]
        for i in range(len(u.sizes)):
            u.send(N, T, i, s, clobber=True)
        s.synchronize()

    run_workers(worker, 4, timeout=120.0, name="uploader")
    torch.cuda.synchronize()
    for u in sets:
        u.check()
