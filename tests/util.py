"""Shared type tables and input generators for the parity tests (seeded; the
generators are numpy only)."""
import numpy as np
import torch

NP_WORD = {1: np.uint16, 2: np.uint16, 3: np.uint32, 4: np.uint64}
FT_NAME = {1: "fp16", 2: "bf16", 3: "fp32", 4: "fp64"}

# The same per float type (ft) tables with ft 0, the byte codec, where a byte
# entry makes sense.  Words travel to torch as signed integers of their width
# (torch has no unsigned 16 / 32 / 64-bit arithmetic): NP_SIGNED / TORCH_WORD
# name that view, NP_W the unsigned one the archives and the oracle use.
NP_W = {0: np.uint8, **NP_WORD}
NP_SIGNED = {0: np.uint8, 1: np.int16, 2: np.int16, 3: np.int32, 4: np.int64}
TORCH_WORD = {0: torch.uint8, 1: torch.int16, 2: torch.int16, 3: torch.int32, 4: torch.int64}
TORCH_FLOAT = {1: torch.float16, 2: torch.bfloat16, 3: torch.float32, 4: torch.float64}
TORCH_OUT = {0: torch.uint8, **TORCH_FLOAT}  # what a decode's output holds
WORD_BYTES = {0: 1, 1: 2, 2: 2, 3: 4, 4: 8}
FT_IDS = {0: "bytes", **FT_NAME}
FT_OF = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3, torch.float64: 4}


def exp_bytes(n, lam=100.0, seed=1):
    """b = min(255, floor(256 * min(Exp(lam), 1))) -- ANSTest.cu:18-31 shape."""
    rng = np.random.default_rng(seed)
    x = rng.exponential(1.0 / lam, n)
    return np.minimum(255, np.floor(256.0 * np.minimum(x, 1.0))).astype(np.uint8)


def float_words(ft, n, seed=0, scale=1.0):
    """N(0,1) floats as raw words: bf16 by fp32 truncation (FloatTest.cu:21-29),
    fp16 by round-to-nearest, fp32 / fp64 native."""
    rng = np.random.default_rng(seed)
    if ft == 4:
        return (rng.standard_normal(n) * scale).astype(np.float64).view(np.uint64)
    f = (rng.standard_normal(n) * scale).astype(np.float32)
    if ft == 1:
        return f.astype(np.float16).view(np.uint16)
    if ft == 2:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    return f.view(np.uint32)


def sparsify(words, frac_zero=0.9, seed=5):
    rng = np.random.default_rng(seed)
    w = words.copy()
    w[rng.random(w.size) < frac_zero] = 0
    return w


# --------------------------------------------------------------------------
# Adversarial content: blocks at the maximum rate beside nearly silent ones,
# and histograms that drive every branch of the table normalisation.
# --------------------------------------------------------------------------

BLOCK = 4096

# The standard rate-extreme element: both halves of a wave's block pair rare
# (0, 1 and 20, 21), only the low half (6), only the high half (9), a rare
# block in another 8-block workgroup (40) and a rare partial tail block with
# no partner (64).
STD_BLOCKS, STD_TAIL = 64, 1000
STD_RARE = [0, 1, 6, 9, 20, 21, 40, 64]
# A second layout for the second symbol stream of fp64, so that the two
# streams of one wave run dry at different steps.
STD_RARE_C1 = [1, 7, 8, 40]
SMALL_BLOCKS, SMALL_RARE = 5, [2]


def _block_slices(n_blocks, blocks, tail):
    n = n_blocks * BLOCK + tail
    for b in blocks:
        assert 0 <= b < n_blocks or (b == n_blocks and tail > 0), b
        yield slice(b * BLOCK, min((b + 1) * BLOCK, n))


def rate_extreme_bytes(n_blocks, rare_blocks, tail, filler=0, max_pb=11):
    """n_blocks * 4096 + tail bytes of `filler`, except that every listed block
    (index n_blocks: the tail block) holds 1 + (k mod 255), k one counter that
    runs on through the rare blocks.  Every rare symbol occurs fewer than
    2 N / 2^max_pb times (asserted), so it quantises to pdf 1 at every
    prob-bits up to max_pb, and keeps it unless the pdfs sum to less than
    2^pb (the 5-block element at pb 11).  With every rare pdf 1 a full rare
    block encodes to 4096 * pb / 16 words, the maximum, all 32 lanes emitting
    on the same steps, and a filler block to almost none."""
    n = n_blocks * BLOCK + tail
    out = np.full(n, filler, dtype=np.uint8)
    k = 0
    for sl in _block_slices(n_blocks, rare_blocks, tail):
        m = sl.stop - sl.start
        out[sl] = 1 + (k + np.arange(m)) % 255
        k += m
    counts = np.bincount(out, minlength=256)
    counts[filler] = 0
    assert counts.max() * (1 << max_pb) < 2 * n, (int(counts.max()), n)
    return out


def rate_mirror_bytes(n_blocks, const_blocks, tail, const=7, seed=11):
    """The mirror image of rate_extreme_bytes: uniformly random bytes (about
    2048 words per block, the lanes out of step) except the listed blocks,
    which hold one constant."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, n_blocks * BLOCK + tail, dtype=np.uint8)
    for sl in _block_slices(n_blocks, const_blocks, tail):
        out[sl] = const
    return out


def std_extreme_bytes(rare=None):
    return rate_extreme_bytes(STD_BLOCKS, STD_RARE if rare is None else rare, STD_TAIL)


def small_extreme_bytes():
    return rate_extreme_bytes(SMALL_BLOCKS, SMALL_RARE, 0)


def std_mirror_bytes():
    return rate_mirror_bytes(STD_BLOCKS, STD_RARE, STD_TAIL)


def words_from_symbols(ft, c0, c1=None, seed=0, nonzero=False):
    """Float words whose ANS symbol streams (pyref.float_split) are exactly
    the bytes c0 (and, fp64, c1); every other bit is random.  fp16: the high
    byte; bf16: bits 14..7; fp32: bits 30..23; fp64: c0 = bits 62..55, c1 =
    bits 54..47.  nonzero: bit 0 (never a symbol bit) is set in every word."""
    rng = np.random.default_rng(seed)
    c0 = np.asarray(c0, dtype=np.uint8)
    n = c0.size
    assert (c1 is not None) == (ft == 4)
    if ft in (1, 2):
        r = rng.integers(0, 1 << 16, n, dtype=np.uint16)
        c = c0.astype(np.uint16)
        w = (c << 8) | (r & 0x00FF) if ft == 1 else (r & 0x807F) | (c << 7)
    elif ft == 3:
        r = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        w = (r & np.uint32(0x807FFFFF)) | (c0.astype(np.uint32) << 23)
    else:
        c1 = np.asarray(c1, dtype=np.uint8)
        assert c1.size == n
        r = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
        keep = np.uint64((1 << 63) | ((1 << 47) - 1))
        w = (r & keep) | (c0.astype(np.uint64) << np.uint64(55)) | (c1.astype(np.uint64) << np.uint64(47))
    if nonzero:
        w = w | w.dtype.type(1)
    return w


LARGE_FAMILIES = ("large_round_up", "large_above_2p24")


def hard_histograms(seed=0):
    """Named 256-entry count vectors (uint32) that drive the branches of the
    table normalisation the stationary inputs never reach.  The two
    LARGE_FAMILIES have totals of 32 MiB; every other total is below 200 KB."""
    rng = np.random.default_rng(seed)
    fam = {}

    def vec(d):
        h = np.zeros(256, dtype=np.uint32)
        for s, c in d.items():
            h[s] = c
        return h

    # many count-1 symbols + a few mid counts + one dominant count: the excess
    # (one per singleton) exceeds the number of entries above 1, so there are
    # many decrement rounds, and the mid entries reach 1 and leave the group
    # (g shrinks from round to round)
    h = np.zeros(256, dtype=np.uint32)
    h[rng.permutation(256)[:200]] = 1
    free = np.flatnonzero(h == 0)
    for s, c in zip(free[:6], (60, 90, 150, 150, 240, 400)):
        h[s] = c
    h[free[6]] = 60000
    fam["singletons_mid_dominant"] = h

    # 40 equal mid counts + singletons + a dominant count: the last round
    # decrements only part of the group of equal pdfs (the symbol id decides)
    h = np.zeros(256, dtype=np.uint32)
    perm = rng.permutation(256)
    h[perm[:40]] = 700
    h[perm[40:140]] = 1
    h[perm[140]] = 72000
    fam["tie_group_cut"] = h
    # two tie groups of different pdfs
    h = np.zeros(256, dtype=np.uint32)
    perm = rng.permutation(256)
    h[perm[:40]] = 500
    h[perm[40:60]] = 1100
    h[perm[60:190]] = 1
    h[perm[190]] = 50000
    fam["two_tie_groups"] = h

    # 2 .. 256 symbols with counts 1 .. 3
    for nsym in (2, 3, 17, 100, 255, 256):
        h = np.zeros(256, dtype=np.uint32)
        h[rng.permutation(256)[:nsym]] = rng.integers(1, 4, nsym)
        fam[f"tiny_counts_{nsym}"] = h

    # diff > 0 (equal counts whose quotient truncates), and the bumped ids
    # 0 .. diff - 1 do not occur in the input
    fam["bump_absent_ids"] = vec({s: 1000 for s in range(200, 211)})
    fam["bump_absent_ids_3"] = vec({100: 3333, 180: 3333, 255: 3333})

    fam["two_symbols"] = vec({10: 1, 200: 99999})
    fam["lone_255"] = vec({255: 5000})
    fam["squares"] = (np.arange(256, dtype=np.uint32) * 7 % 23) ** 2

    # the float32 quotient rounds up across an integer at a small total: at
    # pb 10, 1024 * fl(35016 / 40063) = 895 where the exact floor is 894.  The
    # pdfs then sum to 1024 and nothing is bumped; with the exact floor
    # symbol 0, which does not occur, would get pdf 1.
    fam["small_round_up"] = vec({5: 35016, 9: 5047})

    # totals above 2^24: float32(count) rounds, and at pb 10 the float32
    # quotient of the first rounds up across an integer (1000, exactly 999)
    fam["large_round_up"] = vec({0: 32774999, 1: 786601})
    fam["large_above_2p24"] = vec({0: (1 << 24) + 1, 1: (1 << 24) + 3, 2: 5, 255: 1})
    assert set(LARGE_FAMILIES) <= set(fam)
    return fam


def bytes_from_histogram(h, seed=0):
    """A seeded permutation of h[s] copies of every symbol s."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), np.asarray(h, dtype=np.int64)))


# --------------------------------------------------------------------------
# Sparse codec: sizes on every edge of its index arithmetic (64-word ballot
# steps, 1024-word chunks, 4096-word tiles, 262,144-word scan workgroups), the
# four zero / nonzero combinations of the last two words (the reference's n-2
# quirk), special bit patterns, and one element past 65 scan workgroups.
# --------------------------------------------------------------------------

SPARSE_SMALL_B = (256, 1024, 2048, 4096, 8192)
SPARSE_LARGE_B = 262144  # one k_sparseChunks workgroup: 256 chunks of 1024 words
SPARSE_BLOCK_EDGE = (4095, 4096, 4097, 4098, 8191, 8192, 8193)
# (x[n-2] != 0, x[n-1] != 0)
SPARSE_TAILS = ((False, False), (False, True), (True, False), (True, True))
SPARSE_FILLS = ("zero", "half", "dense")


def sparse_edge_sizes():
    """(small sizes, large sizes)."""
    small = list(range(201)) + [B + d for B in SPARSE_SMALL_B for d in range(-2, 3)]
    large = [SPARSE_LARGE_B + d for d in range(-2, 3)]
    return small, large


def _sparse_fill(ft, n, fill, seed):
    if fill == "zero":
        return np.zeros(n, dtype=NP_WORD[ft])
    w = float_words(ft, n, seed=seed)
    if fill == "half":
        return sparsify(w, 0.5, seed=seed + 1)
    w[w == 0] = 1  # (fp16 rounds small draws to zero)
    return w


def sparse_edge_elements(ft):
    """[(group, name, words)]: group "small" or "large".  Every size of
    sparse_edge_sizes() with each of the four SPARSE_TAILS (for n == 1 the two
    values of x[0]); a forced nonzero word is w | 1.  The other words cycle
    with n through SPARSE_FILLS.  Then elements without zeros and all-zero
    elements at SPARSE_BLOCK_EDGE: the list's length falls on the dense
    codec's 4096-symbol block edge, and an all-zero element's list is the n-2
    slot alone."""
    out = []
    small, large = sparse_edge_sizes()
    for group, sizes in (("small", small), ("large", large)):
        for n in sizes:
            fill = SPARSE_FILLS[n % 3]
            base = _sparse_fill(ft, n, fill, seed=7 * n + ft)
            tails = SPARSE_TAILS if n >= 2 else SPARSE_TAILS[:2][:n + 1]
            for t2, t1 in tails:
                w = base.copy()
                if n >= 2:
                    w[n - 2] = (w[n - 2] | 1) if t2 else 0
                if n >= 1:
                    w[n - 1] = (w[n - 1] | 1) if t1 else 0
                out.append((group, f"n{n}_{fill}_t{int(t2)}{int(t1)}", w))
    for n in SPARSE_BLOCK_EDGE:
        for fill in ("dense", "zero"):
            out.append(("small", f"n{n}_all_{fill}", _sparse_fill(ft, n, fill, seed=11 * n + ft)))
    return out


def sparse_special_patterns(ft):
    """name -> word: the bit patterns sparse_special_words() mixes in.  Only
    +0.0 is a zero of the sparse codec (generate_bitmap tests the word)."""
    bits = 8 * np.dtype(NP_WORD[ft]).itemsize
    exp_bits, man_bits = {1: (5, 10), 2: (8, 7), 3: (8, 23), 4: (11, 52)}[ft]
    sign = 1 << (bits - 1)
    inf = ((1 << exp_bits) - 1) << man_bits
    p = {
        "pos_zero": 0,
        "neg_zero": sign,
        "min_denormal": 1,
        "neg_min_denormal": sign | 1,
        "pos_inf": inf,
        "neg_inf": sign | inf,
        "quiet_nan": inf | (1 << (man_bits - 1)),
        "signalling_nan": inf | 1,
        "neg_nan_all_ones": (1 << bits) - 1,
    }
    if ft == 4:
        p["low_half_zero"] = 0x3FF0000000000000  # 1.0
        p["low_half_zero_denormal"] = 0x0000000100000000
        p["high_half_zero"] = 0x00000000FFFFFFFF
        p["high_half_zero_top_bit"] = 0x0000000080000000
    return {k: NP_WORD[ft](v) for k, v in p.items()}


SPARSE_SPECIAL_N = 4321  # two tiles, five chunks, an odd tail


def sparse_special_words(ft):
    """name -> words, three variants of one element of SPARSE_SPECIAL_N words:
    N(0,1) words, 40 % of them +0.0, then 30 % of the positions overwritten
    with the patterns of sparse_special_patterns() in equal shares (each at
    least once).  "base" ends in two random nonzero words, "negzero_n2" has -0.0 at
    n-2 (no gap slot: -0.0 is nonzero) and "negzero_n1" has +0.0 at n-2 and
    -0.0 at n-1 (the gap slot, then a -0.0 in the list)."""
    n = SPARSE_SPECIAL_N
    rng = np.random.default_rng(900 + ft)
    pats = sparse_special_patterns(ft)
    w = sparsify(float_words(ft, n, seed=910 + ft), 0.4, seed=920 + ft)
    vals = np.array(list(pats.values()), dtype=NP_WORD[ft])
    pick = rng.random(n) < 0.3
    w[pick] = vals[rng.integers(0, len(vals), int(pick.sum()))]
    pos = rng.permutation(n - 2)[: len(vals)]  # every pattern at least once
    w[pos] = vals
    neg0 = pats["neg_zero"]
    base = w.copy()
    base[n - 2:] |= NP_WORD[ft](1)
    n2 = w.copy()
    n2[n - 2], n2[n - 1] = neg0, w[n - 1] | NP_WORD[ft](1)
    n1 = w.copy()
    n1[n - 2], n1[n - 1] = 0, neg0
    return {"base": base, "negzero_n2": n2, "negzero_n1": n1}


SPARSE_FAR_N = 66 * SPARSE_LARGE_B + 1102


def sparse_far_element():
    """bf16, SPARSE_FAR_N words, about 1 % nonzero at seeded positions,
    x[n-2] == 0 != x[n-1].  Its chunks from word 65 * 262,144 on belong to scan
    workgroups above 64, whose list offsets k_sparseExpand sums in a second
    round of its blockTot loop."""
    n = SPARSE_FAR_N
    rng = np.random.default_rng(66)
    k = n // 100
    w = np.zeros(n, dtype=np.uint16)
    w[rng.integers(0, n, k)] = float_words(2, k, seed=67) | np.uint16(1)
    w[n - 2] = 0
    w[n - 1] = 0x3F81
    return w
