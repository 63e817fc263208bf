"""The GPU test harness (tests/gpu_harness.py) checked on the CPU: the layout
that placement promises, that a correct call passes check_placed() in both
comparison styles, and that every kind of wrong write or wrong status makes it
fail.  The "call" is a fake written here that applies the CPU model in place;
no device and no codec is involved."""
import numpy as np
import pytest
import torch

from tests import accumulate_cases as A
from tests import sparse_accumulate_cases as S
from tests.gpu_harness import (GUARD, SENTINEL, Cache, Member, check_placed, dense_at, host_ptrs, pack_bytes,
                               place_members, place_words, placed_mismatch, retyped, scatter_rows, sentinel_words,
                               word_starts)
from tests.util import NP_WORD, float_words

SIZES = (0, 1, 7, 8, 9)
# (ft, mode): 2-, 4- and 8-byte accumulators, 8, 4 and 2 of them per 16 B
MODES = [(2, 1), (2, 2), (4, 1)]
MODE_IDS = ["bf16", "bf16-f32acc", "fp64"]


def words(ft, n, seed):
    """n nonzero words, every third one (the first among them) +0.0."""
    w = float_words(ft, n, seed=seed) | NP_WORD[ft](1)
    w[::3] = 0
    return w


def blob(i):
    return (np.arange(5 + 7 * i) % 251 + 1).astype(np.uint8)


class Style:
    """The two ways the accumulate modules fill and compare a buffer."""

    def __init__(self, name, ft, mode):
        self.name, self.ft, self.mode, self.dtype = name, ft, mode, A.acc_dtype(ft, mode)
        if name == "dense":  # every word is added; same_bits over the whole buffer
            self.init = lambda total: A.random_acc(ft, mode, total, seed=1)
            self.apply = lambda acc, w: A.model(acc, A.words_to_float(w, ft), mode)
            self.touched = lambda w: torch.ones(w.size, dtype=torch.bool)
            self.compare = lambda got, want, init, touch: None if A.same_bits(got, want) else "differs"
        else:  # nonzero words only; everything else keeps its very bits
            self.init = lambda total: S.case_acc(ft, mode, total, seed=1)
            self.apply = lambda acc, w: S.expected(acc, w, ft, mode)
            self.touched = S.touched
            self.compare = S.check

    def model(self):
        return self.apply, self.touched, self.compare


class Placed:
    """Members of every size at both offsets, one a word short (it must fail),
    one with room to spare and one over an accumulator of -0.0, placed on the
    CPU; call() is the fake: the model applied in place."""

    def __init__(self, style):
        self.style = style
        ft = style.ft
        ms = [Member(blob(len(SIZES) * off + i), words(ft, n, seed=10 * off + i), acc_off=off,
                     arch_off=4 * (i % 2) if style.name == "dense" else 0)
              for off in (0, 1) for i, n in enumerate(SIZES)]
        self.failing, self.spare, self.negzero = len(ms), len(ms) + 1, len(ms) + 2
        ms.append(Member(blob(10), words(ft, 9, seed=30), cap=8, acc_off=1, ok=False, size=9))
        ms.append(Member(blob(11), words(ft, 7, seed=31), cap=7 + 3))
        ms.append(Member(blob(12), words(ft, 8, seed=32), acc=torch.full([8], -0.0, dtype=style.dtype)))
        self.members = ms
        self.archives, self.accs, self.buf, self.init, self.starts = place_members(ms, style.dtype, style.init,
                                                                                   device="cpu")
        assert self.buf.data_ptr() != self.init.data_ptr()

    def call(self):
        """-> (ok, sz) as a correct call reports them."""
        for m, acc in zip(self.members, self.accs):
            if m.ok:
                acc[:m.x.size] = self.style.apply(acc[:m.x.size], m.x)
        return [int(m.ok) for m in self.members], [m.size for m in self.members]

    def check(self, status):
        check_placed(self.members, status, self.buf, self.init, self.starts, *self.style.model())

    def change_word(self, at):
        A.bits(self.buf)[at] ^= 1


def styles():
    return [Style(name, ft, mode) for name in ("dense", "sparse") for ft, mode in MODES]


STYLES = pytest.mark.parametrize("style", styles(), ids=lambda s: f"{s.name}-{MODE_IDS[MODES.index((s.ft, s.mode))]}")


# -------------------------------------------------------------------- layout ----

@pytest.mark.parametrize("guard", [GUARD, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64], ids=["2B", "4B", "8B"])
def test_words_start_at_their_offset_with_guards_around(dtype, guard):
    caps = [n for n in SIZES for _ in (0, 1)] + [8, 10]
    offs = [k % 2 for k in range(len(caps))]
    views, buf, init, starts = place_words(dtype, caps, offs, lambda total: torch.zeros(total, dtype=dtype),
                                           guard=guard, device="cpu")
    assert (starts, buf.numel()) == word_starts(dtype, caps, offs, guard)
    assert buf.data_ptr() % 16 == 0 and buf.data_ptr() != init.data_ptr() and buf.dtype == dtype
    end = 0
    for v, st, cap, off in zip(views, starts, caps, offs):
        assert v.numel() == cap
        assert cap == 0 or v.data_ptr() == buf.data_ptr() + st * dtype.itemsize
        assert (st - off) * dtype.itemsize % 16 == 0
        assert st - end >= guard  # from the buffer's start, then from the member before
        end = st + cap
    assert buf.numel() - end >= guard


def test_a_view_is_the_buffer():
    views, buf, init, _ = place_words(torch.float32, [3, 5], [1, 0], lambda total: torch.arange(total).float(),
                                      device="cpu")
    views[1][2] = -1.0
    assert int((buf != init).sum()) == 1


def test_packed_bytes_are_aligned_apart_and_whole():
    blobs = [blob(i) for i in range(8)] + [np.zeros(0, dtype=np.uint8), blob(9)]
    offs = [4 * (i % 2) for i in range(len(blobs))]
    views = pack_bytes(blobs, offs, device="cpu")
    base = views[0].data_ptr() - offs[0]
    assert base % 16 == 0
    end = 0
    for v, b, off in zip(views, blobs, offs):
        assert np.array_equal(v.numpy(), b)
        if b.size:
            at = v.data_ptr() - base
            assert at % 16 == off and at >= end
            end = at + b.size


# -------------------------------------------------------------- check_placed ----

@STYLES
def test_a_correct_call_passes(style):
    p = Placed(style)
    status = p.call()
    assert status[0].count(0) == 1
    p.check(status)
    p.check(None)  # a call without status tensors
    assert not torch.equal(A.bits(p.buf), A.bits(p.init))


def flipped_bit(p, status):
    k = SIZES.index(9)
    p.change_word(p.starts[k] + 4)  # under a nonzero word


def flipped_bit_under_a_zero_word(p, status):
    k = SIZES.index(9)
    assert p.members[k].x[3] == 0
    p.change_word(p.starts[k] + 3)


def guard_before(p, status):
    p.change_word(p.starts[3] - 1)


def first_guard_word(p, status):
    p.change_word(0)


def guard_after(p, status):
    p.change_word(p.starts[3] + p.members[3].cap)


def last_guard_word(p, status):
    p.change_word(p.buf.numel() - 1)


def after_an_empty_member(p, status):
    assert p.members[0].cap == 0
    p.change_word(p.starts[0])


def failing_member_written(p, status):
    p.change_word(p.starts[p.failing] + 4)


def spare_capacity_written(p, status):
    m = p.members[p.spare]
    assert m.cap > m.x.size
    p.change_word(p.starts[p.spare] + m.x.size)


def failing_member_reports_success(p, status):
    status[0][p.failing] = 1


def wrong_size(p, status):
    status[1][2] += 1


def failing_member_reports_size_zero(p, status):
    assert status[1][p.failing] == 9
    status[1][p.failing] = 0


TAMPER = [flipped_bit, flipped_bit_under_a_zero_word, guard_before, first_guard_word, guard_after, last_guard_word,
          after_an_empty_member, failing_member_written, spare_capacity_written, failing_member_reports_success,
          wrong_size, failing_member_reports_size_zero]


@pytest.mark.parametrize("tamper", TAMPER, ids=lambda f: f.__name__)
@STYLES
def test_check_placed_fails_on(style, tamper):
    p = Placed(style)
    status = p.call()
    tamper(p, status)
    with pytest.raises(AssertionError):
        p.check(status)


@pytest.mark.parametrize("ft,mode", MODES, ids=MODE_IDS)
def test_sparse_style_tells_the_zeros_apart(ft, mode):
    """-0.0 under a zero word turned into +0.0: what an add of +0.0 would do."""
    p = Placed(Style("sparse", ft, mode))
    status = p.call()
    at = p.starts[p.negzero]
    assert p.members[p.negzero].x[0] == 0
    neg = A.bits(torch.tensor([-0.0], dtype=p.style.dtype))[0]
    assert A.bits(p.buf)[at] == neg == A.bits(p.init)[at]
    p.check(status)
    p.buf[at] = 0.0
    assert p.buf[at] == p.init[at] and A.bits(p.buf)[at] == 0
    with pytest.raises(AssertionError, match="untouched words changed|words differ"):
        p.check(status)


def test_member_defaults():
    w = words(2, 9, seed=0)
    m = Member(blob(0), w)
    assert (m.cap, m.size, m.ok, m.acc_off, m.arch_off, m.acc) == (9, 9, True, 0, 0, None)
    assert Member(blob(0), w, cap=8, ok=False).size == 0       # a failing member reports 0 unless told
    assert Member(blob(0), w, cap=8, ok=False, size=9).size == 9
    none = Member(blob(0), None, cap=5, ok=False)
    assert (none.cap, none.size) == (5, 0)


# ------------------------------------------------------------ Cache, retyped ----

def test_cache_makes_once_per_key():
    made = []

    def make(k):
        made.append(k)
        return [k]

    c, other = Cache(), Cache()
    first = c.get(("a", 1), lambda: make("a"))
    assert c.get(("a", 1), lambda: make("again")) is first
    assert c.get(("b", 1), lambda: make("b")) == ["b"]
    assert other.get(("a", 1), lambda: make("other")) == ["other"]  # instances share nothing
    assert made == ["a", "b", "other"]


def test_dense_at():
    assert [dense_at(n) for n in (0, 1, 128, 129, 4097)] == [16, 32, 32, 48, 16 + 528]


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("at", [8, dense_at(200) + 8])
@pytest.mark.parametrize("ft", [1, 2, 3, 4])
def test_retyped_changes_the_type_nibble_alone(ft, at, as_torch):
    a = (np.arange(at + 40) * 37 % 256).astype(np.uint8)
    a[at] = 0xA0 | ft
    keep = a.copy()
    src = torch.from_numpy(a) if as_torch else a
    p = retyped(src, ft, at=at)
    assert type(p) is type(src) and np.array_equal(a, keep)  # a copy
    got = p.numpy() if as_torch else p
    assert np.flatnonzero(got != keep).tolist() == [at]
    assert got[at] >> 4 == 0xA and got[at] & 0xF in (1, 2, 3, 4) and got[at] & 0xF != ft


# ------------------------------------------------------------- large batches ----

def test_large_batch_helpers_place_and_locate():
    """sentinel_words / host_ptrs / scatter_rows / placed_mismatch (the
    device-side placement of tests/test_gpu_slices.py) on the CPU: the rows
    land in their slices and nowhere else, and a wrong word is named with its
    member."""
    caps = [3, 0, 5, 1, 4]
    starts, total = word_starts(torch.int16, caps, [0] * len(caps))
    starts_np = np.array(starts, dtype=np.int64)
    buf = sentinel_words(total, torch.int16, device="cpu")
    assert buf.shape == (total,) and buf.dtype == torch.int16
    assert bool((buf.view(torch.uint8) == SENTINEL).all())
    assert sentinel_words([2, 3], torch.uint8, device="cpu").shape == (2, 3)
    assert host_ptrs(1000, starts_np, 2).tolist() == [1000 + 2 * s for s in starts]

    row = torch.arange(100, 110, dtype=torch.int16)
    want = buf.clone()
    for st, cap in zip(starts, caps):
        want[st:st + cap] = row[:cap]
    # whole rows (plain counts), member by member
    got = buf.clone()
    for st, cap in zip(starts, caps):
        scatter_rows(got, torch.tensor([st]), 0, cap, row)
    assert torch.equal(got, want) and placed_mismatch(got, want, starts_np) is None
    # ragged counts and firsts in one call
    got = buf.clone()
    firsts = torch.tensor([0, 4, 2, 9, 1])
    scatter_rows(got, torch.tensor(starts), firsts, torch.tensor(caps), row)
    for st, cap, f in zip(starts, caps, firsts.tolist()):
        assert torch.equal(got[st:st + cap], row[f:f + cap])
    touched = torch.zeros(total, dtype=torch.bool)
    for st, cap in zip(starts, caps):
        touched[st:st + cap] = True
    assert torch.equal(got[~touched], buf[~touched])
    scatter_rows(got, torch.tensor(starts)[:0], 0, 3, row)  # no member: nothing happens
    scatter_rows(got, torch.tensor(starts), 0, torch.zeros(5, dtype=torch.int64), row)

    wrong = want.clone()
    wrong[starts[2] + 1] += 1
    assert "1 words into member 2" in placed_mismatch(wrong, want, starts_np)
    wrong = want.clone()
    wrong[starts[4] + caps[4] + 2] = 0  # a guard word
    assert "member 4" in placed_mismatch(wrong, want, starts_np)
    wrong = want.clone()
    wrong[0] = 0
    assert "before member 0" in placed_mismatch(wrong, want, starts_np)
