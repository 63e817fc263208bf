"""Host threads for the GPU tests: run_workers() starts one threading.Thread per
worker, hands back what they returned and re-raises, in the calling thread,
the first exception any of them raised.  A worker that is still running when
the time limit ends fails the test by name (the thread is a daemon, so the
process can still end).  Workers start together, behind a barrier, so that
their calls really overlap.

Not a conftest: test modules import what they use by name."""
import threading
import time


class WorkerHung(AssertionError):
    pass


def run_workers(target, count, timeout=120.0, name="worker"):
    """target(index) on `count` threads -> [results by index]."""
    results = [None] * count
    errors = [None] * count
    gate = threading.Barrier(count)

    def body(i):
        try:
            gate.wait(timeout)
            results[i] = target(i)
        except BaseException as e:  # noqa: BLE001  (re-raised below, in the caller)
            errors[i] = e
            gate.abort()

    threads = [threading.Thread(target=body, args=(i,), name=f"{name}-{i}", daemon=True) for i in range(count)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    # a worker's own failure explains more than the barrier breaking under the others
    first = next((e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)),
                 next((e for e in errors if e is not None), None))
    if alive:
        raise WorkerHung(f"still running after {timeout} s: {alive}" + (f"; first error: {first!r}" if first else ""))
    if first is not None:
        raise first
    return results
