"""Independent pure-Python restatement of the reference codec, for SMALL
inputs only.  Written separately from oracle/dietgpu_oracle.c (different
structure, Python ints, struct packing) so the two can pin each other.

Citations relative to /root/reference/dietgpu.
"""
import struct

import numpy as np

BLOCK = 4096


def round_up(a, b):
    return (a + b - 1) // b * b


def quantize(count, total, W):
    # ans/GpuANSStatistics.cuh:212-218 in IEEE float32
    r = np.float32(count) / np.float32(total)
    f = np.float32(W) * r
    return int(f)


def normalize(hist, total, pb):
    """normalizeProbabilitiesFromHistogram (ans/GpuANSStatistics.cuh:178-366)"""
    if total == 0:
        return [0] * 256
    W = 1 << pb
    q = []
    for s in range(256):
        v = quantize(hist[s], total, W)
        if hist[s] > 0 and v == 0:
            v = 1
        q.append(v)
    order = sorted(range(256), key=lambda s: (q[s] << 16) | s, reverse=True)
    diff = W - sum(q)
    while diff > 0:
        step = min(diff, 256)
        for s in range(step):
            q[s] += 1
        diff -= step
    d = -diff
    while d > 0:
        g = sum(1 for v in q if v > 1)
        k = min(d, g)
        for r in range(g - k, g):
            q[order[r]] -= 1
        d -= k
    return q


def ans_encode(data, pb=10, checksum=False):
    data = bytes(bytearray(np.asarray(data, dtype=np.uint8)))
    n = len(data)
    hist = [0] * 256
    for b in data:
        hist[b] += 1
    pdf = normalize(hist, n, pb)
    cdf = [0] * 256
    for s in range(1, 256):
        cdf[s] = cdf[s - 1] + pdf[s - 1]
    nb = (n + BLOCK - 1) // BLOCK
    blocks = []
    for b in range(nb):
        chunk = data[b * BLOCK:(b + 1) * BLOCK]
        states = [1 << 15] * 32
        words = []
        for t in range((len(chunk) + 31) // 32):
            for lane in range(32):
                i = 32 * t + lane
                if i >= len(chunk):
                    continue
                s = chunk[i]
                x = states[lane]
                if x >= pdf[s] << (31 - pb):
                    words.append(x & 0xFFFF)
                    x >>= 16
                states[lane] = (x // pdf[s]) * (1 << pb) + x % pdf[s] + cdf[s]
        blocks.append((len(chunk), states, words))
    pre = []
    run = 0
    for (_, _, w) in blocks:
        pre.append(run)
        run += round_up(len(w), 8)
    total = run
    ck = 0
    if checksum:
        for b in data:
            ck ^= b
    out = bytearray()
    out += struct.pack("<8I", 0xD00D0001, nb, n, total, pb | (16 if checksum else 0), ck, 0, 0)
    out += struct.pack("<256H", *pdf)
    for (_, st, _) in blocks:
        out += struct.pack("<32I", *st)
    for b, (uw, _, w) in enumerate(blocks):
        out += struct.pack("<2I", (uw << 16) | len(w), pre[b])
    if nb % 2:
        out += bytes(8)
    for (_, _, w) in blocks:
        out += struct.pack(f"<{len(w)}H", *w) + bytes(2 * (round_up(len(w), 8) - len(w)))
    return np.frombuffer(bytes(out), dtype=np.uint8)


def ans_decode(arch, pb=10):
    a = bytes(np.asarray(arch, dtype=np.uint8))
    magic, nb, n, total, opts, ck, _, _ = struct.unpack_from("<8I", a, 0)
    assert magic == 0xD00D0001 and opts & 0xF == pb
    pdf = struct.unpack_from("<256H", a, 32)
    cdf = [0] * 256
    for s in range(1, 256):
        cdf[s] = cdf[s - 1] + pdf[s - 1]
    lut = []
    for s in range(256):
        lut += [(s, pdf[s], cdf[s])] * pdf[s]
    off_states = 544
    off_bw = off_states + 128 * nb
    off_data = off_bw + 8 * round_up(nb, 2)
    out = bytearray(n)
    for b in range(nb):
        states = list(struct.unpack_from("<32I", a, off_states + 128 * b))
        x0, start = struct.unpack_from("<2I", a, off_bw + 8 * b)
        uw, cw = x0 >> 16, x0 & 0xFFFF
        words = struct.unpack_from(f"<{cw}H", a, off_data + 2 * start)
        ptr = cw
        for t in reversed(range((uw + 31) // 32)):
            for lane in reversed(range(32)):
                i = 32 * t + lane
                if i >= uw:
                    continue
                x = states[lane]
                s, p, c = lut[x & ((1 << pb) - 1)]
                out[b * BLOCK + i] = s
                x = p * (x >> pb) + (x & ((1 << pb) - 1)) - c
                if x < (1 << 15):
                    ptr -= 1
                    x = (x << 16) + words[ptr]
                states[lane] = x
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _rotl(v, s, bits):
    m = (1 << bits) - 1
    return ((v << s) | (v >> (bits - s))) & m


def float_split(ft, words):
    """(comp0 bytes, comp1 bytes, raw section bytes) per float/GpuFloatUtils.cuh."""
    n = len(words)
    c0 = bytearray(n)
    c1 = bytearray(n)
    if ft in (1, 2):
        raw = bytearray(round_up(n, 16))
        for i, w in enumerate(int(v) for v in words):
            if ft == 1:
                c0[i], raw[i] = w >> 8, w & 0xFF
            else:
                v = _rotl((w << 16) | w, 1, 32)
                c0[i], raw[i] = v >> 24, v & 0xFF
    elif ft == 3:
        lo = bytearray(2 * round_up(n, 8))
        hi = bytearray(round_up(n, 16))
        for i, w in enumerate(int(v) for v in words):
            v = _rotl(w, 1, 32)
            c0[i] = v >> 24
            struct.pack_into("<H", lo, 2 * i, v & 0xFFFF)
            hi[i] = (v >> 16) & 0xFF
        raw = lo + hi
    else:
        lo = bytearray(4 * round_up(n, 4))
        hi = bytearray(2 * round_up(n, 8))
        for i, w in enumerate(int(v) for v in words):
            v = _rotl(w, 1, 64)
            c0[i] = v >> 56
            c1[i] = (v >> 48) & 0xFF
            struct.pack_into("<I", lo, 4 * i, v & 0xFFFFFFFF)
            struct.pack_into("<H", hi, 2 * i, (v >> 32) & 0xFFFF)
        raw = lo + hi
    return bytes(c0), bytes(c1), bytes(raw)


def float_compress(ft, words, pb=10, checksum=False, word_bytes=None):
    c0, c1, raw = float_split(ft, words)
    n = len(words)
    a1 = ans_encode(np.frombuffer(c0, np.uint8), pb).tobytes()
    ck = 0
    if checksum:
        for b in word_bytes[:n]:
            ck ^= b
    out = struct.pack("<4I", 0xF00F0001, n, ft | (16 if checksum else 0), ck)
    out += struct.pack("<4I", round_up(len(a1), 16), 0, 0, 0)
    out += raw + a1
    if ft == 4:
        out += bytes(round_up(len(a1), 16) - len(a1))
        out += ans_encode(np.frombuffer(c1, np.uint8), pb).tobytes()
    return np.frombuffer(out, dtype=np.uint8)


# --------------------------------------------------------------------------
# Sparse float codec.  Restated from the reference's kernels, not from
# oracle/dietgpu_oracle.c: float/GpuSparseFloatCompress.cuh :32-58
# (generate_bitmap), :64-113 (bitmap_bytes_to_bits), :119-185
# (fill_comp_input), :237-247 (addBitmapToOutSizes), :360-367 (the exclusive
# scan); float/GpuSparseFloatDecompress.cuh :26-62 (bitmap_bits_to_bytes),
# :73-145 (fill_in_nonzeros).  Like the reference it keeps a 0/1 flag array
# and an explicit u32 exclusive scan of it.
# --------------------------------------------------------------------------

_NP_WORD = {1: np.uint16, 2: np.uint16, 3: np.uint32, 4: np.uint64}


def _exclusive_scan_u32(flags):
    # thrust::exclusive_scan(.., 0) into uint32_t (:360-367)
    idx = np.zeros(flags.size, dtype=np.uint32)
    if flags.size > 1:
        np.cumsum(flags[:-1], dtype=np.uint32, out=idx[1:])
    return idx


def sparse_list(ft, words, gap_fill=0):
    """fill_comp_input (:119-185): the nonzero list handed to the dense codec.
    gap_fill: the value of the slot the reference never writes (list[idx[n-2]]
    when x[n-2] == 0; uninitialised memory there)."""
    W = _NP_WORD[ft]
    x = np.ascontiguousarray(words, dtype=W)
    n = x.size
    flag = (x != 0).astype(np.uint8)  # generate_bitmap :56, bitwise: -0.0 is nonzero
    if n <= 1:
        # the reference reads idx[-1] here; as the oracle defines it, the list
        # is the word itself when it is nonzero, and empty otherwise
        return x[flag == 1].copy()
    idx = _exclusive_scan_u32(flag)
    count = int(idx[n - 2]) + int(flag[n - 1]) + 1  # :183
    lst = np.full(count, gap_fill, dtype=W)
    body = np.flatnonzero(flag[: n - 1] == 1)  # :162-168, i < n-1
    lst[idx[body]] = x[body]
    if flag[n - 1] == 1:
        lst[int(idx[n - 2]) + 1] = x[n - 1]  # :177-179
    return lst


def sparse_compress(ft, words, pb=10, checksum=False, gap_fill=0, pad_fill=0, pad_bits=False):
    """Sparse archive: 16 B header {n, 0, 0, 0}, the bitmap MSB-first
    (bitmap_bytes_to_bits :108-110) padded to 16 B, the dense archive of the
    nonzero list.  gap_fill, pad_fill, pad_bits: the content of what the
    reference leaves uninitialised -- the n-2 quirk's list slot, the bitmap's
    padding bytes and (pad_bits) the bits of its last byte past n, filled from
    pad_fill too.  The defaults are what this project's compressor writes."""
    W = _NP_WORD[ft]
    x = np.ascontiguousarray(words, dtype=W)
    n = x.size
    flag = (x != 0).astype(np.uint8)
    nbytes = (n + 7) // 8
    padded = np.zeros(8 * nbytes, dtype=np.uint8)  # "zero-padded at the end" :66-68
    padded[:n] = flag
    bitmap = np.zeros(round_up(nbytes, 16), dtype=np.uint8)
    g = padded.reshape(nbytes, 8).astype(np.uint32)
    for j in range(8):
        bitmap[:nbytes] |= (g[:, j] << (7 - j)).astype(np.uint8)  # v.x[j] << (7 - j)
    bitmap[nbytes:] = pad_fill
    if pad_bits and n % 8:
        bitmap[nbytes - 1] |= pad_fill & ((1 << (8 - n % 8)) - 1)
    lst = sparse_list(ft, x, gap_fill)
    dense = float_compress(ft, lst, pb, checksum=checksum, word_bytes=lst.view(np.uint8))
    out = struct.pack("<4I", n, 0, 0, 0) + bitmap.tobytes() + dense.tobytes()
    return np.frombuffer(out, dtype=np.uint8)


def float_join(ft, c0, c1, raw, n):
    """The inverse of float_split."""
    W = _NP_WORD[ft]
    out = np.zeros(n, dtype=W)
    for i in range(n):
        if ft == 1:
            w = (c0[i] << 8) | raw[i]
        elif ft == 2:
            # c0 = bits 14..7 of w; raw = bits 6..0, then the sign
            w = (c0[i] << 7) | (raw[i] >> 1) | ((raw[i] & 1) << 15)
        elif ft == 3:
            lo, = struct.unpack_from("<H", raw, 2 * i)
            hi = raw[2 * round_up(n, 8) + i]
            v = (c0[i] << 24) | (hi << 16) | lo
            w = ((v >> 1) | (v << 31)) & 0xFFFFFFFF
        else:
            lo, = struct.unpack_from("<I", raw, 4 * i)
            hi, = struct.unpack_from("<H", raw, 4 * round_up(n, 4) + 2 * i)
            v = (c0[i] << 56) | (c1[i] << 48) | (hi << 32) | lo
            w = ((v >> 1) | (v << 63)) & 0xFFFFFFFFFFFFFFFF
        out[i] = w
    return out


def float_decompress(ft, arch, pb=10):
    a = bytes(np.asarray(arch, dtype=np.uint8))
    magic, n, opts, _, ans_off = struct.unpack_from("<5I", a, 0)
    assert magic == 0xF00F0001 and opts & 0xF == ft
    rawsz = {1: round_up(n, 16), 2: round_up(n, 16), 3: 2 * round_up(n, 8) + round_up(n, 16),
             4: 4 * round_up(n, 4) + 2 * round_up(n, 8)}[ft]
    raw = a[32: 32 + rawsz]
    body = np.frombuffer(a, dtype=np.uint8)[32 + rawsz:]
    c0 = ans_decode(body, pb)
    c1 = ans_decode(body[ans_off:], pb) if ft == 4 else None
    return float_join(ft, bytes(c0), bytes(c1) if ft == 4 else None, raw, n)


def sparse_decompress(ft, arch, pb=10):
    """bitmap_bits_to_bytes (:26-62) and fill_in_nonzeros (:73-145)."""
    a = np.asarray(arch, dtype=np.uint8)
    n = int(a[:4].view(np.uint32)[0])
    nbytes = (n + 7) // 8
    bits = a[16: 16 + nbytes]
    flag = np.zeros(8 * nbytes, dtype=np.uint8)
    for j in range(8):
        flag[j::8] = (bits & (1 << (7 - j))) >> (7 - j)  # :59
    lst = float_decompress(ft, a[16 + round_up(nbytes, 16):], pb)
    out = np.zeros(n, dtype=_NP_WORD[ft])
    if n == 0:
        return out
    if n == 1:  # idx[-1] in the reference; see sparse_list
        if flag[0]:
            out[0] = lst[0]
        return out
    idx = _exclusive_scan_u32(flag[:n])
    body = np.flatnonzero(flag[: n - 1] == 1)
    out[body] = lst[idx[body]]
    if flag[n - 1] == 1:
        out[n - 1] = lst[int(idx[n - 2]) + 1]  # :139-140
    return out
