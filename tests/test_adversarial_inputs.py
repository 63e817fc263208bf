"""CPU checks of the adversarial generators in tests/util.py: they pin what
tests/test_gpu_adversarial.py feeds the kernels, so that those tests cannot
silently go soft.  The rate-extreme elements must really hold blocks at the
maximum rate beside nearly silent ones, the float words must split into
exactly the given symbol streams, and the histogram families must really
reach the normalisation branches they are named for.  Oracle and pyref (two
independent restatements of the reference) must agree on all of them."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import pyref
from tests.util import (BLOCK, LARGE_FAMILIES, NP_WORD, SMALL_BLOCKS, SMALL_RARE, STD_BLOCKS, STD_RARE,
                        STD_RARE_C1, STD_TAIL, bytes_from_histogram, exp_bytes, hard_histograms,
                        rate_extreme_bytes, small_extreme_bytes, std_extreme_bytes, std_mirror_bytes,
                        words_from_symbols)

PBS = [9, 10, 11]


def block_words(arch):
    """Compressed words of every block, from the archive's block-words table."""
    nb = int(arch[4:8].view(np.uint32)[0])
    off = 32 + 512 + 128 * nb
    return arch[off: off + 8 * nb].view(np.uint32)[0::2] & 0xFFFF


def test_generators_are_seeded_and_shaped():
    d = std_extreme_bytes()
    assert d.size == STD_BLOCKS * BLOCK + STD_TAIL == 263144 and d.dtype == np.uint8
    np.testing.assert_array_equal(d, std_extreme_bytes())
    rare = np.zeros(STD_BLOCKS + 1, dtype=bool)
    rare[STD_RARE] = True
    for b in range(STD_BLOCKS + 1):
        blk = d[b * BLOCK: (b + 1) * BLOCK]
        assert (blk != 0).all() if rare[b] else (blk == 0).all(), b
    # one counter runs on through the rare blocks: 1, 2, .., 255, 1, ..
    np.testing.assert_array_equal(d[d != 0], 1 + np.arange(int((d != 0).sum())) % 255)
    assert small_extreme_bytes().size == SMALL_BLOCKS * BLOCK
    m = std_mirror_bytes()
    np.testing.assert_array_equal(m, std_mirror_bytes())
    for b in STD_RARE:
        assert (m[b * BLOCK: (b + 1) * BLOCK] == 7).all()
    assert len(np.unique(m[2 * BLOCK: 3 * BLOCK])) > 200
    with pytest.raises(AssertionError):  # a rare symbol's pdf would exceed 1
        rate_extreme_bytes(4, [0, 1, 2], 0)


@pytest.mark.parametrize("pb", PBS)
def test_standard_element_rates(pb):
    """Full rare blocks encode to 4096 * pb / 16 words (every symbol costs pb
    bits), the rare tail block to floor(k * pb / 16) words per lane of k
    symbols, every filler block to fewer than 256; 255 symbols have pdf 1."""
    arch = O.ans_encode(std_extreme_bytes(), pb)
    cw = block_words(arch)
    assert cw.size == STD_BLOCKS + 1
    full = BLOCK * pb // 16
    assert full == {9: 2304, 10: 2560, 11: 2816}[pb]
    for b in range(STD_BLOCKS + 1):
        if b == STD_BLOCKS:
            long_lanes = STD_TAIL % 32
            k = STD_TAIL // 32
            assert cw[b] == long_lanes * ((k + 1) * pb // 16) + (32 - long_lanes) * (k * pb // 16)
        elif b in STD_RARE:
            assert cw[b] == full, (b, cw[b])
        else:
            assert cw[b] < 256, (b, cw[b])
    pdf = arch[32:544].view(np.uint16)
    assert int((pdf == 1).sum()) == 255 and pdf[0] > 1
    # the 5-block element: one rare block between quiet ones.  At pb 11 its
    # quantised pdfs sum to less than 2^11 and symbols 1 .. 154 are bumped to
    # pdf 2 (10 bits each): still above uniform bytes' 2048 words.
    arch = O.ans_encode(small_extreme_bytes(), pb)
    cw = block_words(arch)
    pdf = arch[32:544].view(np.uint16).astype(np.int64)
    bits = 4096 * pb - int(np.floor(np.log2(pdf[small_extreme_bytes()[2 * BLOCK: 3 * BLOCK]])).sum())
    assert (pdf[1:] == 1).all() == (pb < 11)
    for b in range(SMALL_BLOCKS):
        if b in SMALL_RARE:
            assert 2048 < bits // 16 - 32 <= cw[b] <= bits // 16 and (pb == 11 or cw[b] == full), (b, cw[b])
        else:
            assert cw[b] < 256, (b, cw[b])
    # the mirror: about 2048 words in a random block, far fewer in a constant one
    cw = block_words(O.ans_encode(std_mirror_bytes(), pb))
    for b in range(STD_BLOCKS):
        assert (cw[b] < 1024) if b in STD_RARE else (1900 < cw[b] < 2200), (b, cw[b])


@pytest.mark.parametrize("pb", PBS)
def test_oracle_matches_pyref_on_byte_elements(pb):
    for name, d in (("standard", std_extreme_bytes()), ("small", small_extreme_bytes()),
                    ("mirror", std_mirror_bytes()), ("33 bytes", exp_bytes(33, lam=10.0, seed=3))):
        np.testing.assert_array_equal(O.ans_encode(d, pb), pyref.ans_encode(d, pb), err_msg=name)


def _small_words(ft):
    c0 = small_extreme_bytes()
    c1 = rate_extreme_bytes(SMALL_BLOCKS, [3], 0) if ft == 4 else None
    return c0, c1, words_from_symbols(ft, c0, c1, seed=ft)


@pytest.mark.parametrize("ft", [1, 2, 3, 4])
def test_words_from_symbols_split(ft):
    """float_split returns exactly the given streams, for the 5-block element
    and for uniformly random streams (every byte value)."""
    c0, c1, w = _small_words(ft)
    assert w.dtype == NP_WORD[ft]
    g0, g1, _ = pyref.float_split(ft, w)
    assert g0 == c0.tobytes()
    if ft == 4:
        assert g1 == c1.tobytes()
    rng = np.random.default_rng(ft)
    r0 = rng.integers(0, 256, 3000, dtype=np.uint8)
    r1 = rng.integers(0, 256, 3000, dtype=np.uint8) if ft == 4 else None
    for nonzero in (False, True):
        w = words_from_symbols(ft, r0, r1, seed=9, nonzero=nonzero)
        g0, g1, _ = pyref.float_split(ft, w)
        assert g0 == r0.tobytes() and (ft != 4 or g1 == r1.tobytes())
        assert not nonzero or (w != 0).all()
    # the other bits are random, not constant
    assert len(np.unique(words_from_symbols(ft, np.zeros(3000, np.uint8),
                                            np.zeros(3000, np.uint8) if ft == 4 else None, seed=1))) > 100


@pytest.mark.parametrize("ft", [1, 2, 3, 4])
@pytest.mark.parametrize("pb", [9, 11])
def test_oracle_matches_pyref_on_float_elements(ft, pb):
    _, _, w = _small_words(ft)
    np.testing.assert_array_equal(O.float_compress(w, ft, pb), pyref.float_compress(ft, w, pb))


def test_standard_float_layouts_differ_per_stream():
    """fp64: the two symbol streams of the standard element are rare in
    different blocks (the two chains of a wave then refill at different
    times)."""
    c0, c1 = std_extreme_bytes(), std_extreme_bytes(STD_RARE_C1)
    w = words_from_symbols(4, c0, c1, seed=4)
    v = (w << np.uint64(1)) | (w >> np.uint64(63))
    np.testing.assert_array_equal((v >> np.uint64(56)).astype(np.uint8), c0)
    np.testing.assert_array_equal(((v >> np.uint64(48)) & np.uint64(0xFF)).astype(np.uint8), c1)
    r0 = {b for b in range(STD_BLOCKS + 1) if c0[b * BLOCK] != 0}
    r1 = {b for b in range(STD_BLOCKS + 1) if c1[b * BLOCK] != 0}
    assert r0 == set(STD_RARE) and r1 == set(STD_RARE_C1) and r0 - r1 and r1 - r0 and r0 & r1


# ---------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------

def trace_normalize(h, total, pb, exact=False):
    """normalizeProbabilitiesFromHistogram once more, recording its course:
    -> (pdf, quantised pdf, diff, [(g, k) per decrement round], whether a round
    cut inside a group of equal pdfs).  exact: the quotient as the exact
    rational floor instead of the reference's float32 arithmetic."""
    W = 1 << pb
    q = []
    for s in range(256):
        c = int(h[s])
        v = int(Fraction(W * c, total)) if exact else pyref.quantize(c, total, W)
        q.append(1 if c > 0 and v == 0 else v)
    q0 = list(q)
    order = sorted(range(256), key=lambda s: (q[s], s), reverse=True)
    diff = W - sum(q)
    if diff > 0:
        for s in range(256):
            q[s] += diff // 256 + (1 if s < diff % 256 else 0)
    rounds, tie_cut = [], False
    d = -diff
    while d > 0:
        g = sum(1 for v in q if v > 1)
        k = min(d, g)
        if k < g and q[order[g - k - 1]] == q[order[g - k]]:
            tie_cut = True
        for r in range(g - k, g):
            q[order[r]] -= 1
        rounds.append((g, k))
        d -= k
    return q, q0, diff, rounds, tie_cut


@pytest.fixture(scope="module")
def families():
    return hard_histograms(0)


def test_families_are_seeded(families):
    again = hard_histograms(0)
    assert list(again) == list(families)
    for name, h in families.items():
        assert h.shape == (256,) and h.dtype == np.uint32 and h.sum() > 0, name
        np.testing.assert_array_equal(h, again[name])
    small = [int(h.sum()) for n, h in families.items() if n not in LARGE_FAMILIES]
    assert max(small) <= 200000 and sum(small) < 2_000_000
    h = families["squares"]
    d = bytes_from_histogram(h, seed=3)
    np.testing.assert_array_equal(np.bincount(d, minlength=256), h)
    np.testing.assert_array_equal(d, bytes_from_histogram(h, seed=3))
    assert (np.diff(d.astype(np.int32)) < 0).any()  # permuted, not sorted


@pytest.mark.parametrize("pb", PBS)
def test_oracle_matches_pyref_on_families(families, pb):
    for name, h in families.items():
        total = int(h.sum())
        want = pyref.normalize([int(c) for c in h], total, pb)
        pdf, cdf = O.normalize(h, total, pb)
        assert pdf.tolist() == want, name
        assert int(pdf.sum()) == 1 << pb, name
        assert cdf.tolist() == [sum(want[:s]) for s in range(256)], name
        assert trace_normalize(h, total, pb)[0] == want, name


def test_families_reach_every_branch(families):
    shrinking, tie_cuts, bumps_absent = [], [], []
    for name, h in families.items():
        total = int(h.sum())
        for pb in PBS:
            _, _, diff, rounds, tie_cut = trace_normalize(h, total, pb)
            if len(rounds) > 1 and len({g for g, _ in rounds}) > 1:
                shrinking.append((name, pb))
            if tie_cut:
                tie_cuts.append((name, pb))
            if diff > 0 and any(h[s] == 0 for s in range(min(diff, 256))):
                bumps_absent.append((name, pb))
    # each branch in the family built for it, at every prob-bits
    assert {("singletons_mid_dominant", pb) for pb in PBS} <= set(shrinking)
    assert {("tie_group_cut", pb) for pb in PBS} <= set(tie_cuts)
    assert {("bump_absent_ids", pb) for pb in PBS} <= set(bumps_absent)
    # rounds in which every remaining entry is decremented, then a partial one
    _, _, _, rounds, _ = trace_normalize(families["tie_group_cut"], int(families["tie_group_cut"].sum()), 10)
    assert rounds[0][0] == rounds[0][1] and rounds[-1][1] < rounds[-1][0]


def test_float32_quotient_differs_from_exact_floor(families):
    """The quantised pdfs of the large-total vectors (and of small_round_up)
    are not the exact rational floors: float32(count) rounds above 2^24, and
    the float32 quotient rounds up across an integer."""
    h = families["large_round_up"]
    assert int(h.sum()) == 33561600
    assert pyref.quantize(32774999, 33561600, 1024) == 1000
    assert (1024 * 32774999) // 33561600 == 999
    for name in LARGE_FAMILIES + ("small_round_up",):
        h = families[name]
        total = int(h.sum())
        differs = [pb for pb in PBS
                   if trace_normalize(h, total, pb)[1] != trace_normalize(h, total, pb, exact=True)[1]]
        assert 10 in differs, (name, differs)
    # ... and for these two the final tables differ as well, so an archive
    # from any other quotient cannot equal the oracle's
    for name in ("large_above_2p24", "small_round_up"):
        h = families[name]
        total = int(h.sum())
        assert trace_normalize(h, total, 10)[0] != trace_normalize(h, total, 10, exact=True)[0], name
    for name in LARGE_FAMILIES:
        assert int(families[name].max()) > 1 << 24
