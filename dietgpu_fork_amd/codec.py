"""Tensor-level wrappers of the C ABI (stride / pointer / split / sparse entry
points), used by tests and bench.py.  Every function runs the HIP kernels on
the torch current stream and returns device tensors; nothing here computes on
the CPU.
"""
import contextlib

import torch

from . import _native as N

FLOAT_TYPE = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3, torch.float64: 4}
WORD_DTYPE = {1: torch.int16, 2: torch.int16, 3: torch.int32, 4: torch.int64}


def _s():
    return torch.cuda.current_stream().cuda_stream


class Workspace:
    """A StackDeviceMemory over a torch uint8 buffer (reused across calls)."""

    def __init__(self, nbytes, device="cuda"):
        self.buf = torch.empty([max(int(nbytes), 256)], dtype=torch.uint8, device=device)
        self.stack = N.Stack(self.buf.get_device(), self.buf.data_ptr(), self.buf.numel())

    def max_usage(self):
        return self.stack.max_usage()

    @property
    def h(self):
        return self.stack.h


def _ws(ws, device):
    return ws if ws is not None else Workspace(256, device)


def test_histogram(x2d, size=None, ws=None):
    """Test hook (libdietgpu_testhooks.so): per-row byte histograms of a [nb, stride] uint8 CUDA tensor
    (the first `size` bytes of each row) by the compressor's histogram kernel."""
    nb, stride = x2d.shape
    size = stride if size is None else size
    hist = torch.empty([nb, 256], dtype=torch.int32, device=x2d.device)
    ws = _ws(ws, x2d.device)
    N.test_check(N.testlib().dietgpu_test_histogram(ws.h, nb, x2d.data_ptr(), size, stride, hist.data_ptr(), _s()))
    return hist


def test_enc_magic(device="cuda"):
    """Test hook (libdietgpu_testhooks.so): the compressors' in-register
    division magic of every pdf 0 .. 2048, as an int64 CPU tensor."""
    m = torch.empty([(1 << 11) + 1], dtype=torch.int32, device=device)
    N.test_check(N.testlib().dietgpu_test_enc_magic(m.data_ptr(), _s()))
    return m.cpu().to(torch.int64) & 0xffffffff


# csrc/compress_plan.h: Refused, HistKernel, Normalise
PLAN_REFUSED = ("", "two-segments", "user-hist", "unaligned", "forced", "too-large", "size-rule")
PLAN_HIST = ("plain", "checksum", "rows")
PLAN_NORMALISE = ("caller", "prologue", "in-hist", "in-reduce", "kernel")
_PLAN_FIELDS = ("single_pass", "refused", "team", "too_many_items", "rounds", "teams_per_round", "xcd", "grid",
                "max_r", "items", "chunk_words", "chunks", "groups", "run_hist", "raw_ck", "hist", "normalise",
                "encode_wgs", "encode_runs", "coalesce_from_flags")


def test_compress_plan(ft, nb, max_size, checksum=False, user_hist=False, aligned16=True):
    """Test hook (libdietgpu_testhooks.so): the plan (dietgpu_test_plan, as a
    dict with the enumerations named) the dense compress driver computes on
    this device in the current compress-path mode for nb elements of at most
    max_size bytes (ft 0) or words (ft 1..4)."""
    import ctypes

    out = (ctypes.c_uint32 * len(_PLAN_FIELDS))()
    N.test_check(N.testlib().dietgpu_test_compress_plan(int(ft), int(nb), int(max_size), int(checksum),
                                                        int(user_hist), int(aligned16), out))
    plan = dict(zip(_PLAN_FIELDS, out))
    plan["refused"] = PLAN_REFUSED[plan["refused"]]
    plan["hist"] = PLAN_HIST[plan["hist"]]
    plan["normalise"] = PLAN_NORMALISE[plan["normalise"]]
    return plan


def max_compressed_size(nbytes):
    return N.size_or_raise(N.lib().dietgpu_get_max_compressed_size(int(nbytes)))


def max_float_compressed_size(ft, words):
    return N.size_or_raise(N.lib().dietgpu_get_max_float_compressed_size(int(ft), int(words)))


def max_sparse_float_compressed_size(ft, words):
    return N.size_or_raise(N.lib().dietgpu_get_max_sparse_float_compressed_size(int(ft),
                                                                                 int(words)))


def device_error_count(reset=True):
    """Elements the compressor abandoned (outSize 0) since the last reset;
    synchronises the device."""
    return int(N.lib().dietgpu_device_error_count(int(reset)))


def barrier_fallback_count(reset=True):
    """Single-pass compressor team-barrier fallbacks (a workgroup that counted
    its element from the input after waiting out the barrier budget; the
    archive is unchanged) since the last reset; synchronises the device."""
    return int(N.lib().dietgpu_barrier_fallback_count(int(reset)))


def set_dispatch_skew(ticks):
    """Test hook: emulate out-of-order workgroup dispatch (0 = off)."""
    N.lib().dietgpu_set_dispatch_skew(int(ticks))


def set_spin_cap(polls):
    """Test hook: polls per cross-workgroup wait of the compressor (default
    1 << 24; 0 makes every wait that has to wait fail)."""
    N.lib().dietgpu_set_spin_cap(int(polls))


def set_barrier_budget(ticks):
    """Test hook: 100 MHz ticks a single-pass compressor workgroup waits for
    its team before counting the element itself (default 20000; 0 forces the
    fallback on every team wait)."""
    N.lib().dietgpu_set_barrier_budget(int(ticks))


_PATHS = {"auto": 0, "single-pass": 1, "three-kernel": 2}


def set_compress_path(mode):
    """Test hook: "auto" (default: the size rule), "single-pass" (k_pcompress
    whenever the batch is eligible) or "three-kernel" (always k_hist ->
    k_encode).  Archives are identical whatever the mode."""
    N.lib().dietgpu_set_compress_path(_PATHS[mode])


@contextlib.contextmanager
def compress_path(mode):
    """set_compress_path(mode) for the body, "auto" after it."""
    set_compress_path(mode)
    try:
        yield
    finally:
        set_compress_path("auto")


def _pointer_compress(fn, head, ts, row_width, ws, mid=()):
    """The pointer-form compress call fn(ws, *head, nb, ins, sizes, *mid, outs,
    out sizes, stream): ts[i] -> row i of a [nb, row_width(largest numel)]
    matrix -> (out, sizes)."""
    nb = len(ts)
    dev = ts[0].device
    cols = row_width(max(t.numel() for t in ts))
    out = torch.empty([nb, cols], dtype=torch.uint8, device=dev)
    sizes = torch.empty([nb], dtype=torch.int32, device=dev)
    ws = _ws(ws, dev)
    N.check(fn(ws.h, *head, nb, N.ptr_array([t.data_ptr() for t in ts]), N.u32_array([t.numel() for t in ts]), *mid,
               N.ptr_array([out.data_ptr() + i * cols for i in range(nb)]), sizes.data_ptr(), _s()))
    return out, sizes


def _pointer_decode(fn, head, archives, outs, ws, tail=()):
    """The pointer-form decode call fn(ws, *head, nb, archives, outs,
    capacities, *tail, ok, sz, stream): archives[i] -> outs[i] -> (ok, sz)."""
    nb = len(archives)
    dev = archives[0].device
    ok = torch.empty([nb], dtype=torch.uint8, device=dev)
    sz = torch.empty([nb], dtype=torch.int32, device=dev)
    ws = _ws(ws, dev)
    N.check(fn(ws.h, *head, nb, N.ptr_array([a.data_ptr() for a in archives]),
               N.ptr_array([o.data_ptr() for o in outs]), N.u32_array([o.numel() for o in outs]), *tail,
               ok.data_ptr(), sz.data_ptr(), _s()))
    return ok, sz


# ------------------------------------------------------------------ ANS ----

def ans_encode_stride(data2d, prob_bits=10, checksum=False, ws=None, histogram=None,
                      out=None, sizes=None):
    """data2d: [nb, n] uint8 CUDA tensor -> (archives [nb, maxComp] uint8, sizes int32)"""
    nb, n = data2d.shape
    cols = max_compressed_size(n)
    out = out if out is not None else torch.empty([nb, cols], dtype=torch.uint8,
                                                  device=data2d.device)
    sizes = sizes if sizes is not None else torch.empty([nb], dtype=torch.int32,
                                                        device=data2d.device)
    ws = _ws(ws, data2d.device)
    rc = N.lib().dietgpu_ans_encode_batch_stride(
        ws.h, prob_bits, int(checksum), nb, data2d.data_ptr(), n, data2d.stride(0),
        histogram.data_ptr() if histogram is not None else None, out.data_ptr(), out.stride(0),
        sizes.data_ptr(), _s())
    N.check(rc)
    return out, sizes


def ans_decode_stride(archives2d, n, prob_bits=10, checksum=False, ws=None, out=None,
                      capacity=None):
    nb = archives2d.shape[0]
    cap = n if capacity is None else capacity
    out = out if out is not None else torch.empty([nb, max(cap, 1)], dtype=torch.uint8,
                                                  device=archives2d.device)
    ok = torch.empty([nb], dtype=torch.uint8, device=archives2d.device)
    sz = torch.empty([nb], dtype=torch.int32, device=archives2d.device)
    ws = _ws(ws, archives2d.device)
    rc = N.lib().dietgpu_ans_decode_batch_stride(
        ws.h, prob_bits, int(checksum), nb, archives2d.data_ptr(), archives2d.stride(0),
        out.data_ptr(), out.stride(0), cap, ok.data_ptr(), sz.data_ptr(), _s())
    N.check(rc)
    return out, ok, sz


def ans_encode_pointer(ts, prob_bits=10, checksum=False, ws=None):
    """ts: list of uint8 CUDA tensors -> (list of archive rows, sizes)"""
    return _pointer_compress(N.lib().dietgpu_ans_encode_batch_pointer, (prob_bits, int(checksum)), ts,
                             max_compressed_size, ws, mid=(None,))  # no histograms


def ans_decode_pointer(archives, outs, prob_bits=10, checksum=False, ws=None):
    return _pointer_decode(N.lib().dietgpu_ans_decode_batch_pointer, (prob_bits, int(checksum)), archives, outs, ws)


# ---------------------------------------------------------------- float ----

def float_compress_stride(x2d, ft=None, prob_bits=10, checksum=False, ws=None, out=None,
                          sizes=None):
    """x2d: [nb, n] float CUDA tensor (or int16/32/64 words with ft given)."""
    ft = ft or FLOAT_TYPE[x2d.dtype]
    nb, n = x2d.shape
    cols = max_float_compressed_size(ft, n)
    out = out if out is not None else torch.empty([nb, cols], dtype=torch.uint8,
                                                  device=x2d.device)
    sizes = sizes if sizes is not None else torch.empty([nb], dtype=torch.int32,
                                                        device=x2d.device)
    ws = _ws(ws, x2d.device)
    rc = N.lib().dietgpu_float_compress_batch_stride(
        ws.h, ft, prob_bits, int(checksum), nb, x2d.data_ptr(), n,
        x2d.stride(0) * x2d.element_size(), out.data_ptr(), out.stride(0), sizes.data_ptr(),
        _s())
    N.check(rc)
    return out, sizes


def float_decompress_stride(archives2d, n, dtype, prob_bits=10, checksum=False, ws=None,
                            out=None, capacity=None):
    ft = FLOAT_TYPE[dtype] if dtype in FLOAT_TYPE else None
    nb = archives2d.shape[0]
    cap = n if capacity is None else capacity
    out = out if out is not None else torch.empty([nb, max(cap, 1)], dtype=dtype,
                                                  device=archives2d.device)
    ft = ft or {2: 2, 4: 3, 8: 4}[out.element_size()]
    ok = torch.empty([nb], dtype=torch.uint8, device=archives2d.device)
    sz = torch.empty([nb], dtype=torch.int32, device=archives2d.device)
    ws = _ws(ws, archives2d.device)
    rc = N.lib().dietgpu_float_decompress_batch_stride(
        ws.h, ft, prob_bits, int(checksum), nb, archives2d.data_ptr(), archives2d.stride(0),
        out.data_ptr(), out.stride(0) * out.element_size(), cap, ok.data_ptr(), sz.data_ptr(),
        _s())
    N.check(rc)
    return out, ok, sz


def float_compress_pointer(ts, ft=None, prob_bits=10, checksum=False, ws=None):
    ft = ft or FLOAT_TYPE[ts[0].dtype]
    return _pointer_compress(N.lib().dietgpu_float_compress, (ft, prob_bits, int(checksum)), ts,
                             lambda n: max_float_compressed_size(ft, n), ws)


def float_decompress_pointer(archives, outs, ft=None, prob_bits=10, checksum=False, ws=None):
    ft = ft or FLOAT_TYPE[outs[0].dtype]
    return _pointer_decode(N.lib().dietgpu_float_decompress, (ft, prob_bits, int(checksum)), archives, outs, ws)


def float_decompress_accumulate(archives, accs, ft=None, prob_bits=10, ws=None):
    """accs[i] += the element dense float archive archives[i] encodes, in one
    kernel (k_decode's accumulate form) -> (ok, sz) as float_decompress_pointer.
    The accumulators' dtype selects the mode: the archives' own float type (the
    sum is formed in it), or float32 for fp16 / bf16 archives (acc + float(x));
    `ft` names the archives' type and defaults to the accumulators'.  One
    accumulator dtype per call; accumulators of two members must not overlap.
    A failing member's accumulator is untouched.  No checksum is verified."""
    ft, acc_ft = _accumulate_types("float_decompress_accumulate", archives, accs, ft)
    return _pointer_decode(N.lib().dietgpu_float_decompress_accumulate, (ft, prob_bits), archives, accs, ws,
                           tail=(acc_ft,))


def _accumulate_types(who, archives, accs, ft):
    """The argument checks of the accumulate wrappers, before the library is
    touched -> (the archives' float type, the accumulators')."""
    nb = len(archives)
    if len(accs) != nb:
        raise ValueError("archives and accs must have one entry per member")
    if nb == 0:
        raise ValueError(f"{who}: empty batch")
    if any(a.dtype != accs[0].dtype for a in accs):
        raise ValueError(f"{who}: the accumulators must share a dtype")
    if accs[0].dtype not in FLOAT_TYPE:
        raise ValueError(f"{who}: unsupported accumulator dtype {accs[0].dtype}")
    if any(not a.is_contiguous() for a in accs):
        raise ValueError(f"{who}: the accumulators must be contiguous")
    acc_ft = FLOAT_TYPE[accs[0].dtype]
    ft = ft or acc_ft
    if not (acc_ft == ft or (ft in (1, 2) and acc_ft == 3)):
        raise ValueError(f"{who}: accumulator type {acc_ft} does not go with float type {ft}")
    return ft, acc_ft


REDUCE_MAX_SOURCES = 64


def set_reduce_max_sources(ns):
    """Test / tuning hook: the most sources one k_reduce or k_sparseReduce
    launch takes (0: the largest instance, the default); more sources chain
    passes through an fp32 partial.  The results are the same bits."""
    N.lib().dietgpu_set_reduce_max_sources(int(ns))


def float_reduce(sources, outs, inits=None, ft=None, prob_bits=10, ws=None):
    """outs[b] = round((..(inits[b] + x_1) + ..) + x_K), every add in fp32, in
    one fused kernel (k_reduce) -> (ok, sz).  sources: K lists (1 <= K <= 64)
    of one dense float archive per member, x_k = sources[k][b]; all K of a
    member hold the same number of words.  inits: None (the sum starts as
    x_1), or one tensor per member of the archives' dtype or float32; outs: of
    the archives' dtype (rounded once) or float32.  `ft` names the archives'
    type (fp16, bf16 or fp32) and defaults to the outs' (so it must be given
    for fp32 outs of 16-bit archives).  outs[b] may be inits[b] itself.  A
    member with a bad archive, differing sizes or a short out fails as a whole:
    its out and init are untouched.  No checksum is verified."""
    ft, init_ft, out_ft = _reduce_types(sources, outs, inits, ft)
    K, nb = len(sources), len(outs)
    dev = outs[0].device
    ok = torch.empty([nb], dtype=torch.uint8, device=dev)
    sz = torch.empty([nb], dtype=torch.int32, device=dev)
    ws = _ws(ws, dev)
    N.check(N.lib().dietgpu_float_reduce(
        ws.h, ft, prob_bits, nb, K, N.ptr_array([a.data_ptr() for row in sources for a in row]),
        N.ptr_array([t.data_ptr() for t in inits]) if inits is not None else None, init_ft,
        N.ptr_array([o.data_ptr() for o in outs]), N.u32_array([o.numel() for o in outs]), out_ft,
        ok.data_ptr(), sz.data_ptr(), _s()))
    return ok, sz


def _reduce_types(sources, outs, inits, ft, who="float_reduce"):
    """float_reduce's and sparse_reduce's argument checks, before the library
    is touched -> (the archives' float type, the inits' (0: none), the outs')."""
    K, nb = len(sources), len(outs)
    if not 1 <= K <= REDUCE_MAX_SOURCES:
        raise ValueError(f"{who}: the number of sources ({K}) must be in 1 .. {REDUCE_MAX_SOURCES}")
    if nb == 0:
        raise ValueError(f"{who}: empty batch")
    if any(len(row) != nb for row in sources) or (inits is not None and len(inits) != nb):
        raise ValueError(f"{who}: every source list, inits and outs must have one entry per member")
    for what, ts in (("outs", outs), ("inits", inits)):
        if ts is None:
            continue
        if any(t.dtype != ts[0].dtype for t in ts):
            raise ValueError(f"{who}: the {what} must share a dtype")
        if ts[0].dtype not in FLOAT_TYPE:
            raise ValueError(f"{who}: unsupported {what} dtype {ts[0].dtype}")
        if any(not t.is_contiguous() for t in ts):
            raise ValueError(f"{who}: the {what} must be contiguous")
    out_ft = FLOAT_TYPE[outs[0].dtype]
    init_ft = FLOAT_TYPE[inits[0].dtype] if inits is not None else 0
    ft = ft or out_ft
    if ft not in (1, 2, 3):
        raise ValueError(f"{who}: fp16, bf16 or fp32 archives only, not float type {ft}")
    if out_ft not in (ft, 3):
        raise ValueError(f"{who}: out type {out_ft} does not go with float type {ft}")
    if inits is not None and init_ft not in (ft, 3):
        raise ValueError(f"{who}: init type {init_ft} does not go with float type {ft}")
    tensors = [a for row in sources for a in row] + list(outs) + list(inits or [])
    if any(not t.is_cuda for t in tensors):
        raise ValueError(f"{who}: archives, inits and outs must be CUDA tensors")
    return ft, init_ft, out_ft


# ---------------------------------------------------------------- range ----

def _range_launch(fn, head, dev, nb, in_ptrs, firsts, counts, out_ptrs, ws):
    """The C-ABI call on host arrays (ctypes arrays or array addresses)."""
    ok = torch.empty([nb], dtype=torch.uint8, device=dev)
    sz = torch.empty([nb], dtype=torch.int32, device=dev)
    ws = _ws(ws, dev)
    N.check(fn(ws.h, *head, nb, in_ptrs, firsts, counts, out_ptrs, ok.data_ptr(), sz.data_ptr(), _s()))
    return ok, sz


def _range_call(fn, head, archives, firsts, counts, outs, ws):
    nb = len(archives)
    if not (len(firsts) == len(counts) == len(outs) == nb):
        raise ValueError("archives, firsts, counts and outs must have one entry per member")
    for v in list(firsts) + list(counts):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"range bound {int(v)} is outside [0, 2^32)")
    for o, c in zip(outs, counts):
        if o.numel() < int(c) or not o.is_contiguous():
            raise ValueError("every out must be contiguous and hold its count")
    ok, sz = _range_launch(fn, head, archives[0].device, nb, N.ptr_array([a.data_ptr() for a in archives]),
                           N.u32_array([int(f) for f in firsts]), N.u32_array([int(c) for c in counts]),
                           N.ptr_array([o.data_ptr() for o in outs]), ws)
    return outs, ok, sz


def ans_decode_range(archives, firsts, counts, outs=None, prob_bits=10, ws=None):
    """Bytes [firsts[i], firsts[i] + counts[i]) of the element each byte
    archive encodes, into outs[i] (uint8 CUDA tensors of at least counts[i]
    bytes; allocated when None) -> (outs, ok, sz).  An archive may appear in
    any number of members."""
    if outs is None:
        outs = [torch.empty([int(c)], dtype=torch.uint8, device=archives[0].device) for c in counts]
    return _range_call(N.lib().dietgpu_ans_decode_batch_range, (prob_bits,), archives, firsts, counts,
                       outs, ws)


def float_decompress_range(archives, firsts, counts, outs=None, dtype=None, prob_bits=10, ws=None):
    """Float words [firsts[i], firsts[i] + counts[i]) of each dense float
    archive into outs[i] -> (outs, ok, sz).  dtype: the archives' float type
    (default: that of outs[0]).  Sparse archives: sparse_decompress_range."""
    if outs is None:
        outs = [torch.empty([int(c)], dtype=dtype, device=archives[0].device) for c in counts]
    ft = FLOAT_TYPE[dtype if dtype is not None else outs[0].dtype]
    return _range_call(N.lib().dietgpu_float_decompress_range, (ft, prob_bits), archives, firsts,
                       counts, outs, ws)


def sparse_decompress_range(archives, firsts, counts, outs=None, dtype=None, prob_bits=10, ws=None):
    """Float words [firsts[i], firsts[i] + counts[i]) of the element each
    sparse float archive (16-byte aligned) encodes, into outs[i] -> (outs, ok,
    sz): a bitmap rank finds the range's slice of the nonzero list, and only
    that slice is decoded.  dtype: the archives' float type (default: that of
    outs[0]).  An archive may appear in any number of members; its bitmap is
    counted once per call."""
    if outs is None:
        outs = [torch.empty([int(c)], dtype=dtype, device=archives[0].device) for c in counts]
    ft = FLOAT_TYPE[dtype if dtype is not None else outs[0].dtype]
    return _range_call(N.lib().dietgpu_float_decompress_sparse_range, (ft, prob_bits), archives, firsts,
                       counts, outs, ws)


def gather_rows(archive, row_words, rows, dtype, out=None, prob_bits=10, ws=None, sparse=False):
    """Rows `rows` (a list or CPU tensor of row indices, repeats allowed) of a
    [R, row_words] table stored as one archive, into one [len(rows),
    row_words] tensor: one batched range decode whose members all read
    `archive`.  dtype torch.uint8 reads a byte archive; sparse=True reads a
    sparse float archive (not with torch.uint8).  Returns the tensor;
    reads the status back (a host synchronisation) and raises if any row
    lies outside the table."""
    import numpy as np

    if sparse and dtype == torch.uint8:
        raise ValueError("gather_rows: sparse archives hold float words, not torch.uint8")

    rows = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows, dtype=np.int64).reshape(-1)
    nb = int(rows.size)
    out = out if out is not None else torch.empty([nb, row_words], dtype=dtype, device=archive.device)
    if not (out.is_contiguous() and tuple(out.shape) == (nb, row_words) and out.dtype == dtype):
        raise ValueError("out must be a contiguous [len(rows), row_words] tensor of dtype")
    if nb == 0 or row_words == 0:
        return out
    if int(rows.min()) < 0 or (int(rows.max()) + 1) * row_words > 1 << 32:
        raise N.DietGpuError("gather_rows: a row lies outside the table")
    # the host arrays of the call, built without a Python loop over the rows
    firsts = (rows * row_words).astype(np.uint32)
    counts = np.full(nb, row_words, dtype=np.uint32)
    in_ptrs = np.full(nb, archive.data_ptr(), dtype=np.uint64)
    out_ptrs = np.uint64(out.data_ptr()) + np.arange(nb, dtype=np.uint64) * np.uint64(row_words * out.element_size())
    if dtype == torch.uint8:
        fn, head = N.lib().dietgpu_ans_decode_batch_range, (prob_bits,)
    elif sparse:
        fn, head = N.lib().dietgpu_float_decompress_sparse_range, (FLOAT_TYPE[dtype], prob_bits)
    else:
        fn, head = N.lib().dietgpu_float_decompress_range, (FLOAT_TYPE[dtype], prob_bits)
    ok, _ = _range_launch(fn, head, archive.device, nb, in_ptrs.ctypes.data, firsts.ctypes.data,
                          counts.ctypes.data, out_ptrs.ctypes.data, ws)
    if not bool(ok.all()):
        raise N.DietGpuError("gather_rows: a row lies outside the table, or the archive does not "
                             "match dtype / prob_bits")
    return out


def _row_stride(out, row_words):
    """The stride in words between the rows of out [*lead, row_words], or None
    when the last dimension is not contiguous or the rows lie at no one stride."""
    if row_words != 1 and out.stride(-1) != 1:
        return None
    stride, inner = None, 1
    for d in range(out.dim() - 2, -1, -1):
        if out.size(d) != 1:
            if stride is None:
                stride = out.stride(d)
            elif out.stride(d) != stride * inner:
                return None
        inner *= out.size(d)
    return row_words if stride is None else stride


def gather_rows_device(archive, row_words, idx, dtype, out=None, out_status=None, prob_bits=10, ws=None,
                       check=False):
    """Rows idx[...] of a [R, row_words] table stored as one dense float
    archive (or, dtype torch.uint8, one byte archive) -> (out, ok), out
    [*idx.shape, row_words] and ok a uint8 tensor of idx's shape: 1 where the
    row lies inside the table and the archive matches dtype / prob_bits, 0
    where not, and such a row of `out` is untouched.  idx is a contiguous CUDA
    int32 or int64 tensor: the indices stay on the device, nothing is uploaded
    or read back, and the call (one kernel launch on the current stream)
    does not synchronise, so it can be captured in a graph and replayed on new
    indices and new archive bytes.  A caller's `out` may be a view whose last
    dimension is contiguous and whose rows lie at a constant stride.
    check=True reads ok back and raises DietGpuError on any failing row."""
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype in (torch.int32, torch.int64)
            and idx.is_contiguous()):
        raise ValueError("gather_rows_device: idx must be a contiguous CUDA int32 or int64 tensor")
    if dtype != torch.uint8 and dtype not in FLOAT_TYPE:
        raise ValueError(f"gather_rows_device: unsupported dtype {dtype}")
    row_words = int(row_words)
    if row_words < 1:
        raise ValueError("gather_rows_device: row_words must be at least 1")
    shape = [*idx.shape, row_words]
    out = out if out is not None else torch.empty(shape, dtype=dtype, device=idx.device)
    if list(out.shape) != shape or out.dtype != dtype or out.device != idx.device:
        raise ValueError(f"gather_rows_device: out must be a {dtype} tensor of shape {shape} on idx's device")
    stride = _row_stride(out, row_words)
    if stride is None or stride < row_words:
        raise ValueError("gather_rows_device: out's last dimension must be contiguous and its rows must lie at "
                         "a constant stride of at least row_words")
    ok = out_status if out_status is not None else torch.empty(idx.shape, dtype=torch.uint8, device=idx.device)
    if not (ok.dtype == torch.uint8 and ok.is_contiguous() and ok.shape == idx.shape and ok.device == idx.device):
        raise ValueError("gather_rows_device: out_status must be a contiguous uint8 tensor of idx's shape")
    ws = _ws(ws, idx.device)
    tail = (archive.data_ptr(), row_words, idx.numel(), idx.data_ptr(), int(idx.dtype == torch.int64),
            out.data_ptr(), stride, ok.data_ptr(), _s())
    if dtype == torch.uint8:
        N.check(N.lib().dietgpu_ans_gather_rows(ws.h, prob_bits, *tail))
    else:
        N.check(N.lib().dietgpu_float_gather_rows(ws.h, FLOAT_TYPE[dtype], prob_bits, *tail))
    if check and not bool(ok.all()):
        raise N.DietGpuError("gather_rows_device: a row lies outside the table, or the archive does not "
                             "match dtype / prob_bits")
    return out, ok


def gather_rows_sum(archive, row_words, idx, offsets, dtype, out=None, out_dtype=None, out_status=None,
                    prob_bits=10, ws=None, check=False):
    """embedding_bag(mode="sum") on a [R, row_words] table stored as one dense
    float16 / bfloat16 / float32 archive of `dtype` -> (out, ok).  Bag b is
    idx[offsets[b] : offsets[b + 1]] (offsets holds B + 1 boundaries; idx and
    offsets are contiguous 1-d CUDA tensors, both int32 or both int64) and
    out[b] the sum of the bag's rows: fp32 adds in list order, started from
    the first row (a one-row bag returns the row, -0.0 included), rounded once
    to out_dtype, which is `dtype` (the default) or torch.float32.  An empty
    bag gives a row of +0.0.  ok[b] = 1 where the bag's offsets are ordered and
    inside idx, all its rows lie inside the table and the archive matches
    dtype / prob_bits; 0 where not, and such a row of `out` is untouched.  One
    kernel launch on the current stream: nothing is uploaded or read back, so
    the call can be captured in a graph and replayed on new indices, offsets
    and archive bytes, and the result is the same bits on every run.  A
    caller's `out` [B, row_words] may have its rows at a stride.  check=True
    reads ok back and raises DietGpuError on any failing bag.  Not offered:
    mean / max pooling, per-sample weights, sparse archives, float64."""
    who = "gather_rows_sum"
    for name, t in (("idx", idx), ("offsets", offsets)):
        if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.int64) and t.dim() == 1
                and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous 1-d int32 or int64 tensor")
    if idx.dtype != offsets.dtype:
        raise ValueError(f"{who}: idx and offsets must share a dtype, not {idx.dtype} and {offsets.dtype}")
    if offsets.numel() < 1:
        raise ValueError(f"{who}: offsets must hold B + 1 >= 1 entries")
    if dtype == torch.uint8:
        raise ValueError(f"{who}: byte archives hold no floats to sum")
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"{who}: unsupported dtype {dtype} (float16, bfloat16 or float32 archives)")
    out_dtype = out_dtype if out_dtype is not None else (out.dtype if out is not None else dtype)
    if out_dtype not in (dtype, torch.float32):
        raise ValueError(f"{who}: out dtype {out_dtype} does not go with {dtype} archives (their own dtype, or "
                         "torch.float32)")
    row_words = int(row_words)
    if row_words < 1:
        raise ValueError(f"{who}: row_words must be at least 1")
    if not (idx.is_cuda and offsets.is_cuda and idx.device == offsets.device):
        raise ValueError(f"{who}: idx and offsets must be CUDA tensors on one device")
    bags = offsets.numel() - 1
    shape = [bags, row_words]
    out = out if out is not None else torch.empty(shape, dtype=out_dtype, device=idx.device)
    if list(out.shape) != shape or out.dtype != out_dtype or out.device != idx.device:
        raise ValueError(f"{who}: out must be a {out_dtype} tensor of shape {shape} on idx's device")
    stride = _row_stride(out, row_words)
    if stride is None or stride < row_words:
        raise ValueError(f"{who}: out's last dimension must be contiguous and its rows must lie at a constant "
                         "stride of at least row_words")
    ok = out_status if out_status is not None else torch.empty([bags], dtype=torch.uint8, device=idx.device)
    if not (ok.dtype == torch.uint8 and ok.is_contiguous() and list(ok.shape) == [bags] and ok.device == idx.device):
        raise ValueError(f"{who}: out_status must be a contiguous uint8 tensor of {bags} entries")
    ws = _ws(ws, idx.device)
    N.check(N.lib().dietgpu_float_gather_rows_sum(
        ws.h, FLOAT_TYPE[dtype], prob_bits, archive.data_ptr(), row_words, bags, idx.numel(), idx.data_ptr(),
        offsets.data_ptr(), int(idx.dtype == torch.int64), out.data_ptr(), int(out_dtype == torch.float32), stride,
        ok.data_ptr(), _s()))
    if check and not bool(ok.all()):
        raise N.DietGpuError(f"{who}: a bag's offsets or rows lie outside idx or the table, or the archive does "
                             "not match dtype / prob_bits")
    return out, ok


def sparse_compress(ts, ft=None, prob_bits=10, checksum=False, ws=None):
    ft = ft or FLOAT_TYPE[ts[0].dtype]
    return _pointer_compress(N.lib().dietgpu_float_compress_sparse, (ft, prob_bits, int(checksum)), ts,
                             lambda n: max_sparse_float_compressed_size(ft, n), ws)


def sparse_decompress(archives, outs, ft=None, prob_bits=10, checksum=False, ws=None):
    ft = ft or FLOAT_TYPE[outs[0].dtype]
    return _pointer_decode(N.lib().dietgpu_float_decompress_sparse, (ft, prob_bits, int(checksum)), archives, outs,
                           ws)


def sparse_decompress_accumulate(archives, accs, ft=None, prob_bits=10, ws=None):
    """accs[i][j] += word j of the element sparse float archive archives[i]
    (16-byte aligned) encodes, for every j whose word is not +0.0 bitwise
    (k_sparseExpand's accumulate form) -> (ok, sz) as sparse_decompress.  The
    other accumulator words are neither read nor written: an accumulator word
    of -0.0 under a zero word stays -0.0, where float_decompress_accumulate's
    -0.0 + (+0.0) gives +0.0.  Dtype rules, arguments and checks as
    float_decompress_accumulate; sz is the element's size for every member."""
    ft, acc_ft = _accumulate_types("sparse_decompress_accumulate", archives, accs, ft)
    return _pointer_decode(N.lib().dietgpu_float_decompress_sparse_accumulate, (ft, prob_bits), archives, accs, ws,
                           tail=(acc_ft,))


def sparse_reduce(sources, outs, inits=None, ft=None, prob_bits=10, ws=None):
    """float_reduce for sparse float archives (16-byte aligned), in one fused
    kernel per pass (k_sparseReduce) -> (ok, sz): a = float(inits[b][i]); for
    each source k in order, a = a + float(x_k[i]) in fp32 where bit i of x_k's
    bitmap is set (the word is not +0.0 bitwise), a unchanged where it is
    clear; outs[b][i] = round(a).  A clear bit is skipped, never added as
    +0.0, so an init word of -0.0 under clear bits stays -0.0: the bits of
    own.float(), one sparse_decompress_accumulate per source, one rounding.
    inits=None: the sum starts as the decoded word x_1[i] and runs over
    x_2 .. x_K.  Arguments, dtype rules and checks as float_reduce; sz is n of
    the first source for every member."""
    ft, init_ft, out_ft = _reduce_types(sources, outs, inits, ft, who="sparse_reduce")
    K, nb = len(sources), len(outs)
    dev = outs[0].device
    ok = torch.empty([nb], dtype=torch.uint8, device=dev)
    sz = torch.empty([nb], dtype=torch.int32, device=dev)
    ws = _ws(ws, dev)
    N.check(N.lib().dietgpu_float_reduce_sparse(
        ws.h, ft, prob_bits, nb, K, N.ptr_array([a.data_ptr() for row in sources for a in row]),
        N.ptr_array([t.data_ptr() for t in inits]) if inits is not None else None, init_ft,
        N.ptr_array([o.data_ptr() for o in outs]), N.u32_array([o.numel() for o in outs]), out_ft,
        ok.data_ptr(), sz.data_ptr(), _s()))
    return ok, sz


def sparse_reduce_scratch_bytes(ft, nb, num_sources, max_capacity):
    """The workspace bytes a sparse_reduce call of nb members, num_sources
    sources and outs of at most max_capacity words takes at most (the plan's,
    csrc/sparse_plan.h planSparseReduce; host arithmetic only).  It is bounded
    by the sources of one kernel launch, not by num_sources."""
    v = N.lib().dietgpu_float_reduce_sparse_scratch_bytes(int(ft), int(nb), int(num_sources), int(max_capacity))
    if v == 0:
        raise N.DietGpuError(N.lib().dietgpu_last_error().decode(errors="replace"))
    return v


def profile(on=True):
    N.lib().dietgpu_profile_enable(int(on))


def profile_filter(family=None):
    """Record only `family` (None = all families)."""
    N.lib().dietgpu_profile_filter(family.encode() if family else None)


def profile_reset():
    N.lib().dietgpu_profile_reset()


def profile_query(family):
    import ctypes

    ms = ctypes.c_double(0)
    n = ctypes.c_uint64(0)
    N.lib().dietgpu_profile_query(family.encode(), ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value
