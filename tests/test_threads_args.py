"""The error string of the C ABI is per host thread (thread_local gLastError,
csrc/capi.cpp): two threads each make a call that is refused before the stack
or any pointer is looked at, meet, and then read dietgpu_last_error(): each
sees its own message.  No device is touched.  Also the thread helper the GPU
tests share (tests/thread_harness.py): results, the first exception, a worker
that does not end.  tests/test_gpu_threads.py holds the calls that need a GPU."""
import threading

import pytest

import dietgpu_fork_amd  # noqa: F401
from dietgpu_fork_amd import _native as N
from tests.thread_harness import WorkerHung, run_workers


def test_last_error_is_per_thread():
    L = N.lib()
    meet = threading.Barrier(2)
    # (float_type, prob_bits) and what refuses it
    calls = [((2, 12), "unhandled pdf precision 12"), ((7, 10), "float_type must be 1..4")]

    def refused(ft, pb):
        """dietgpu_float_reduce with a null stack and null pointers: its flattened checks come first."""
        return L.dietgpu_float_reduce(None, ft, pb, 1, 3, None, None, 0, None, None, ft, None, None, None)

    def worker(i):
        rc = refused(*calls[i][0])
        meet.wait(30)  # both calls have failed before either thread reads
        return rc, L.dietgpu_last_error().decode()

    for _ in range(20):
        got = run_workers(worker, 2, timeout=60.0)
        for (rc, msg), (_, want) in zip(got, calls):
            assert rc == N.DIETGPU_ERR_INVALID
            assert want in msg
        assert calls[0][1] not in got[1][1] and calls[1][1] not in got[0][1]
    # the main thread made no failing call of its own in between: its string is untouched by theirs
    assert refused(2, 8) == N.DIETGPU_ERR_INVALID
    run_workers(worker, 2, timeout=60.0)
    assert "unhandled pdf precision 8" in L.dietgpu_last_error().decode()


def test_run_workers_returns_results_by_index():
    assert run_workers(lambda i: i * i, 5) == [0, 1, 4, 9, 16]


def test_run_workers_raises_the_first_workers_error_in_the_caller():
    def worker(i):
        if i == 2:
            raise KeyError("from worker 2")
        return i

    with pytest.raises(KeyError, match="from worker 2"):
        run_workers(worker, 4)


def test_run_workers_names_a_worker_that_does_not_end():
    release = threading.Event()

    def worker(i):
        if i == 1:
            release.wait(30)
        return i

    try:
        with pytest.raises(WorkerHung, match="stuck-1"):
            run_workers(worker, 2, timeout=0.2, name="stuck")
    finally:
        release.set()
