"""What the GPU test modules share: the package fixtures, words on the device,
one archive from the GPU compressor, header corruption, compute-once caches,
and the placement of a call's archives and destinations.

Placement carries the suite's strongest guarantee.  The archives of a call lie
in one uint8 buffer at chosen alignments; its destinations are slices of one
buffer of known values, `guard` words apart and from both ends, and the buffer
is compared whole afterwards: a stray write anywhere, or any write to a
failing member, fails the test.  tests/test_gpu_harness_selftest.py checks
that on the CPU (hence the `device` arguments).

Not a conftest: test modules import what they use by name."""
import numpy as np
import pytest
import torch

from tests import pyref
from tests.util import NP_SIGNED, NP_W, TORCH_OUT, TORCH_WORD, WORD_BYTES, exp_bytes, float_words

DEV = "cuda"
GUARD = 16  # words between placed destinations, and before the first and after the last


# ------------------------------------------------------------------ fixtures ----

@pytest.fixture(scope="module")
def C():
    import dietgpu_fork_amd  # noqa: F401
    from dietgpu_fork_amd import codec

    return codec


@pytest.fixture(scope="module")
def N(C):
    from dietgpu_fork_amd import _native

    return _native


def workspace_fixture(nbytes):
    """A module-scoped `ws` of nbytes.  The size is the module's own: it
    decides whether a call overflows the arena."""
    @pytest.fixture(scope="module")
    def ws(C):
        return C.Workspace(nbytes)

    return ws


def single_pass_fixture():
    @pytest.fixture(autouse=True)
    def _single_pass(C):
        """Small batches take the three-kernel path by default (the size rule,
        codec.hip persistentPreferred): the module's batches are meant for the
        single-pass compressor whenever it can take them."""
        with C.compress_path("single-pass"):
            yield

    return _single_pass


# -------------------------------------------------------------------- caches ----

class Cache:
    """Compute-once values (inputs, oracle archives), left unchanged by their
    users.  One instance per module: the archives are large, and a module's
    are dropped with it."""

    def __init__(self):
        self._made = {}

    def get(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]


# --------------------------------------------------------- words and archives ----

def to_dev(words, ft, offset=0, as_float=False):
    """A device copy of numpy `words` as signed integers (TORCH_WORD[ft]; bytes
    for ft 0) that starts `offset` words past a 16 B boundary; as_float: viewed
    as TORCH_OUT[ft]."""
    room = torch.empty(words.size + offset, dtype=TORCH_WORD[ft], device=DEV)
    assert room.data_ptr() % 16 == 0
    t = room[offset:]
    t.copy_(torch.from_numpy(words.view(NP_SIGNED[ft]).copy()))
    return t.view(TORCH_OUT[ft]) if as_float else t


def to_host_words(t, ft):
    """The words of tensor `t` (integer or float view) as unsigned numpy."""
    return t.reshape(-1).view(TORCH_WORD[ft]).cpu().numpy().view(NP_W[ft])


def make_words(ft, n, kind="normal", seed=0):
    if kind == "normal":
        return exp_bytes(n, lam=20.0, seed=seed + 1) if ft == 0 else float_words(ft, n, seed=seed)
    # uniformly random bit patterns: incompressible, blocks of > 512 compressed words
    rng = np.random.default_rng(seed + 77)
    return rng.integers(0, 256, n * WORD_BYTES[ft], dtype=np.uint8).view(NP_W[ft])


def compress_one(C, ws, t_or_words, ft, pb=10, checksum=False, clone=False):
    """One archive (a 16 B-aligned uint8 device tensor) of a device tensor or
    of numpy words from the GPU compressor; clone: exactly sized, nothing of
    the compressor's row behind it."""
    t = to_dev(t_or_words, ft) if isinstance(t_or_words, np.ndarray) else t_or_words
    if ft == 0:
        out, sizes = C.ans_encode_pointer([t], prob_bits=pb, checksum=checksum, ws=ws)
    else:
        out, sizes = C.float_compress_pointer([t], ft=ft, prob_bits=pb, checksum=checksum, ws=ws)
    a = out[0, : int(sizes[0])]
    if clone:
        a = a.clone()
    assert a.data_ptr() % 16 == 0
    return a


def dense_at(n):
    """Where the dense archive starts inside a sparse archive of n words."""
    return 16 + pyref.round_up((n + 7) // 8, 16)


def retyped(a, ft, at=8):
    """A copy of float archive `a` (numpy or torch) whose header names another
    float type: the type is the low nibble of header word 2, byte `at` (for
    the dense part of a sparse archive of n words: dense_at(n) + 8).  The
    layout stays that of `a`, so every header read stays inside it."""
    p = a.clone() if torch.is_tensor(a) else a.copy()
    p[at] = (int(a[at]) & 0xF0) | {1: 2, 2: 1, 3: 4, 4: 3}[ft]
    return p


# ----------------------------------------------------------------- placement ----

def pack_bytes(blobs, offs, device=DEV):
    """Byte blobs in one uint8 buffer, each 16 B-aligned plus its offset."""
    at, cur = [], 0
    for b, o in zip(blobs, offs):
        at.append(cur + o)
        cur = -(-(cur + o + b.size) // 16) * 16
    host = np.zeros(cur + 16, dtype=np.uint8)
    for b, a in zip(blobs, at):
        host[a:a + b.size] = b
    dev = torch.from_numpy(host).to(device)
    assert dev.data_ptr() % 16 == 0
    return [dev[a:a + b.size] for b, a in zip(blobs, at)]


def word_starts(dtype, caps, offs, guard=GUARD):
    """-> (starts, total): member i's caps[i] words start offs[i] words past a
    16 B boundary of a buffer of `total` words, `guard` words apart at least
    and from both ends."""
    per16 = 16 // dtype.itemsize
    starts, cur = [], 0
    for cap, off in zip(caps, offs):
        st = -(-(cur + guard) // per16) * per16 + off
        starts.append(st)
        cur = st + cap + guard
    return starts, cur + per16


def place_words(dtype, caps, offs, init, guard=GUARD, device=DEV):
    """-> (views, buffer, its CPU copy, starts): one buffer of init(total)
    (a CPU tensor of `dtype`) laid out by word_starts()."""
    starts, total = word_starts(dtype, caps, offs, guard)
    init_cpu = init(total)
    assert init_cpu.dtype == dtype and init_cpu.numel() == total
    buf = init_cpu.to(device, copy=True)  # (a CPU `device` would share init_cpu's memory without it)
    assert buf.data_ptr() % 16 == 0
    return [buf[st:st + cap] for st, cap in zip(starts, caps)], buf, init_cpu, starts


# ------------------------------------------------------------- large batches ----
# Batches of tens of thousands of members (tests/test_gpu_slices.py): the
# destinations are placed by word_starts() as above, but the buffer, what it
# must hold afterwards and the comparison all stay on the device, and the
# call's pointer columns are numpy arrays, not lists of tensor views.

SENTINEL = 0xAB  # every byte of a buffer nothing has written yet


def sentinel_words(shape, dtype, device=DEV):
    """A tensor of `shape` and `dtype` whose every byte is SENTINEL."""
    shape = [shape] if isinstance(shape, int) else list(shape)
    flat = torch.full([int(np.prod(shape)) * dtype.itemsize], SENTINEL, dtype=torch.uint8, device=device)
    return flat.view(dtype).view(shape)


def host_ptrs(base, starts, itemsize):
    """The addresses base + starts[i] * itemsize as a numpy uint64 column."""
    return np.uint64(base) + np.asarray(starts, dtype=np.uint64) * np.uint64(itemsize)


def scatter_rows(buf, starts, firsts, counts, row):
    """buf[starts[m] + j] = row[firsts[m] + j] for j < counts[m] and every m:
    1-d tensors on buf's device; starts an int64 tensor, firsts and counts
    int64 tensors of its length or plain ints."""
    m = starts.numel()
    if m == 0:
        return
    most = int(counts.max()) if torch.is_tensor(counts) else int(counts)
    if most == 0:
        return
    j = torch.arange(most, device=buf.device)
    dst = starts[:, None] + j
    src = (firsts[:, None] if torch.is_tensor(firsts) else firsts) + j.expand(m, most)
    if torch.is_tensor(counts):
        keep = j < counts[:, None]
        dst, src = dst[keep], src[keep]
    buf[dst.reshape(-1)] = row[src.reshape(-1)]


def placed_mismatch(got, want, starts):
    """None, or what differs between two placed buffers (integer words on one
    device) and in which member's slice or guard: starts is word_starts()'s,
    ascending, as a numpy array."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"buffers of {got.shape} {got.dtype} and {want.shape} {want.dtype}"
    bad = (got != want).nonzero().view(-1)
    if bad.numel() == 0:
        return None
    first = int(bad[0])
    member = int(np.searchsorted(starts, first, side="right")) - 1
    at = f"{first - int(starts[member])} words into member {member}" if member >= 0 else "before member 0"
    return (f"{bad.numel()} words differ, the first is buffer word {first}, {at}: got "
            f"{int(got[first]):#x}, want {int(want[first]):#x}")


# ---------------------------------------------------- accumulate-style calls ----

class Member:
    """One member of a call that adds an archive's element to an accumulator:
    archive bytes, the words it encodes (None: there is no element, it must
    fail), the accumulator's capacity, the alignments (acc_off words, arch_off
    bytes), whether it must succeed, the size it must report (default: n, or 0
    when it fails) and (acc) values to put into its accumulator instead of
    the buffer's."""

    def __init__(self, arch, x, cap=None, acc_off=0, arch_off=0, ok=True, size=None, acc=None):
        n = x.size if x is not None else 0
        self.arch, self.x, self.ok, self.acc = arch, x, ok, acc
        self.cap = n if cap is None else cap
        self.acc_off, self.arch_off = acc_off, arch_off
        self.size = (n if ok else 0) if size is None else size


def place_members(members, dtype, init, device=DEV):
    """-> (archives, accs, buf, init, starts): pack_bytes() of the archives and
    place_words() of the accumulators over init(total), a member's `acc`
    written over its slice."""
    caps, offs = [m.cap for m in members], [m.acc_off for m in members]
    starts, _ = word_starts(dtype, caps, offs)

    def filled(total):
        t = init(total)
        for m, st in zip(members, starts):
            if m.acc is not None:
                t[st:st + m.acc.numel()] = m.acc
        return t

    archives = pack_bytes([m.arch for m in members], [m.arch_off for m in members], device)
    accs, buf, init_cpu, starts = place_words(dtype, caps, offs, filled, device=device)
    return archives, accs, buf, init_cpu, starts


def accumulate_call(api, names, C, ws, ft, mode, archives, accs, acc_ptrs, pb=10, with_status=True, temp_mem=True):
    """One call through `api`: "codec" (the wrapper names["codec"] of C), "op"
    (names["op"] of torch.ops.dietgpu) or "capi" (names["capi"] of the C ABI,
    the accumulators at acc_ptrs).  The status tensors handed in hold 7 / -7,
    values no call reports.  -> (ok, sz) CPU lists, or None without status."""
    nb = len(archives)
    ok = torch.full([nb], 7, dtype=torch.uint8, device=DEV) if with_status else None
    sz = torch.full([nb], -7, dtype=torch.int32, device=DEV) if with_status else None
    if api == "codec":
        assert with_status
        ok, sz = getattr(C, names["codec"])(archives, accs, ft=ft, prob_bits=pb, ws=ws)
    elif api == "op":
        assert pb == 10
        used = getattr(torch.ops.dietgpu, names["op"])(archives, accs, ws.buf if temp_mem else None, ok, sz)
        assert isinstance(used, int) and used >= 0
    else:
        from dietgpu_fork_amd import _native as N

        rc = getattr(N.lib(), names["capi"])(
            ws.h, ft, pb, nb, N.ptr_array([a.data_ptr() for a in archives]), N.ptr_array(acc_ptrs),
            N.u32_array([a.numel() for a in accs]), 3 if mode == 2 else ft, ok.data_ptr() if with_status else None,
            sz.data_ptr() if with_status else None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.lib().dietgpu_last_error()
    torch.cuda.synchronize()
    return (ok.cpu().tolist(), sz.cpu().tolist()) if with_status else None


def expected_placed(members, init, starts, apply, touched):
    """-> (want, touch): the buffer after the call and the words it may write.
    apply(acc slice, words) is the model's accumulator afterwards and
    touched(words) the positions it may write, for every succeeding member;
    nothing else changes."""
    want = init.clone()
    touch = torch.zeros(init.numel(), dtype=torch.bool)
    for m, st in zip(members, starts):
        if m.ok:
            n = m.x.size
            want[st:st + n] = apply(want[st:st + n], m.x)
            touch[st:st + n] = touched(m.x)
    return want, touch


def check_placed(members, status, got, init, starts, apply, touched, compare):
    """What every placed call must satisfy: status and sizes as the members say
    (status: (ok, sz) lists, or None when the call had no status tensors), and
    the whole buffer `got` (CPU) as expected_placed() has it.
    compare(got, want, init, touch) returns None or what is wrong."""
    if status is not None:
        assert status[0] == [int(m.ok) for m in members]
        assert status[1] == [m.size for m in members]
    want, touch = expected_placed(members, init, starts, apply, touched)
    problem = compare(got, want, init, touch)
    assert problem is None, problem
