"""Multi-GPU sharding of a codec batch.

Every batch element is compressed independently with its own statistics
and archive (reference README.md:110; ans/GpuANSEncode.cuh:686-711), so a
batch shards by contiguous element ranges with no data-path collective:
one process per GPU runs the full codec on its local HBM.  The only
exchange is an all-gather of the per-element compressed sizes -- RCCL over
xGMI on MI355X (backend "nccl"), gloo in the CPU tests -- from which every
rank derives the global packing offsets of the archives.
"""
import torch
import torch.distributed as dist


def shard_range(nb, rank, world):
    """Contiguous [start, stop) of ceil(nb / world) elements for `rank`."""
    per = -(-nb // world)
    start = min(nb, rank * per)
    return start, min(nb, start + per)


def gather_sizes(local_sizes, nb, group=None):
    """All-gather per-element compressed sizes (int32, one per local element)
    into the global [nb] vector (int64).  Shards are padded to the common
    per-rank length so a single all_gather_into_tensor suffices."""
    world = dist.get_world_size(group)
    per = -(-nb // world)
    buf = torch.zeros(per, dtype=torch.int32, device=local_sizes.device)
    buf[: local_sizes.numel()] = local_sizes.to(torch.int32)
    out = torch.empty(per * world, dtype=torch.int32, device=local_sizes.device)
    dist.all_gather_into_tensor(out, buf, group=group)
    return out[:nb].to(torch.int64)


_ALIGN = 16  # archives are packed at 16 B aligned offsets


def _pad(sizes, align=_ALIGN):
    """roundUp(sizes, align): a number or a tensor of them."""
    return (sizes + (align - 1)) // align * align


def archive_offsets(sizes, align=_ALIGN):
    """Exclusive prefix of roundUp(size, align): where each element's archive
    lands when the batch is packed back to back (archives are 16 B aligned,
    SURVEY 8(b))."""
    r = _pad(sizes, align)
    return torch.cumsum(r, 0) - r


class _GpuCodec:
    """What the two codecs of the compressed collectives share: the check of a
    decode's per-archive status and the read of a dense float header."""

    @staticmethod
    def _raise_on_failure(ok):
        if not bool((ok != 0).all()):
            raise RuntimeError("compressed collective: an archive failed to decode")

    def info(self, archive):
        """(numel, dtype) of the element `archive` encodes."""
        return _archive_info(archive)


class GpuFloatCodec(_GpuCodec):
    """The float codec on the local GPU (ops.compress_data /
    ops.decompress_data: k_pcompress or k_hist -> k_encode, then k_decode) for the compressed collectives."""

    def __init__(self, checksum=False):
        self.checksum = checksum

    def compress(self, tensors):
        from . import ops

        comp, sizes, _ = ops.compress_data(True, tensors, self.checksum)
        return comp, sizes

    def decompress(self, archives, outs):
        from . import ops

        status = torch.empty(len(archives), dtype=torch.uint8, device=outs[0].device)
        ops.decompress_data(True, archives, outs, self.checksum, out_status=status)
        self._raise_on_failure(status)

    def accumulate(self, archives, accs):
        """accs[i] += the element archives[i] encodes, in place (k_decode's
        accumulate form; the accumulators' dtype is the archives' own or, for
        fp16 / bf16 archives, float32)."""
        from . import ops

        status = torch.empty(len(archives), dtype=torch.uint8, device=accs[0].device)
        ops.decompress_data_accumulate(archives, accs, out_status=status)
        self._raise_on_failure(status)

    def reduce(self, own, archives, out_dtype):
        """round_out_dtype((...((own + x_1) + x_2) + ...)) over the elements
        x_k of `archives`, every add in float32, in one fused kernel pass
        (k_reduce; ops.reduce_data): no accumulator between the peers.
        own=None: the sum starts as x_1.  float16, bfloat16 and float32."""
        from . import ops

        device = archives[0].device
        n = own.numel() if own is not None else self.info(archives[0])[0]
        out = torch.empty(n, dtype=out_dtype, device=device)
        status = torch.empty(1, dtype=torch.uint8, device=device)
        ops.reduce_data(list(archives), len(archives), [out], None if own is None else [own], out_status=status)
        self._raise_on_failure(status)
        return out


class GpuSparseFloatCodec(_GpuCodec):
    """The sparse float codec on the local GPU (codec.sparse_compress /
    sparse_decompress / sparse_decompress_accumulate / sparse_reduce: bitmap +
    the dense codec on the nonzero words) for the compressed collectives, for tensors that are
    mostly exact zeros (MoE, embedding or pruned gradients).  Lossless like
    GpuFloatCodec, so the moving collectives return the same bits.

    In the reducing collectives the zero words of a peer's tensor are skipped,
    not added: element i of the result is round((...(own + x_r1) + ...)) over
    the peers whose word i is nonzero (bitwise, so a peer's -0.0 is added), in
    the documented order.  That equals GpuFloatCodec's result except where the
    running sum is -0.0 and a peer's word is +0.0: the dense sum turns +0.0
    there, this one stays -0.0 (and a signalling NaN in the running sum is
    quieted by the dense add only)."""

    def __init__(self, prob_bits=10, workspace_bytes=256 << 20):
        self.prob_bits = prob_bits
        self.workspace_bytes = workspace_bytes
        self._ws = {}

    def _run(self, f, device, *args, **kw):
        """f, a function of codec.py, with this codec's prob_bits and its
        workspace on `device` (made at the first call there)."""
        from . import codec

        if device not in self._ws:
            self._ws[device] = codec.Workspace(self.workspace_bytes, device)
        return f(*args, prob_bits=self.prob_bits, ws=self._ws[device], **kw)

    def compress(self, tensors):
        from . import codec

        return self._run(codec.sparse_compress, tensors[0].device, tensors)

    def decompress(self, archives, outs):
        from . import codec

        ok, _ = self._run(codec.sparse_decompress, outs[0].device, archives, outs)
        self._raise_on_failure(ok)

    def accumulate(self, archives, accs):
        """accs[i] += the element archives[i] encodes, at its nonzero words only
        (k_sparseExpand's accumulate form); dtypes as GpuFloatCodec.accumulate."""
        from . import codec

        # (a float32 accumulator serves three archive types: the header tells)
        ft = self.info(archives[0])[1] if accs[0].dtype == torch.float32 else accs[0].dtype
        ok, _ = self._run(codec.sparse_decompress_accumulate, accs[0].device, archives, accs, ft=codec.FLOAT_TYPE[ft])
        self._raise_on_failure(ok)

    def sparse_reduce(self, own, archives, out_dtype):
        """This codec's fused reduction (_fused_entry).  Not named `reduce`:
        that name promises GpuFloatCodec's sum, in which a peer's +0.0 is
        added; here it is skipped, as in `accumulate`.
        round_out_dtype of own.float() with the elements of `archives` added
        in order, every add in float32 and only where the peer's word is
        nonzero (accumulate's rule), in one fused call (k_sparseReduce;
        codec.sparse_reduce): no accumulator between the peers.  own=None: the
        sum starts as the first archive's element.  float16, bfloat16 and
        float32; the same bits as the per-peer loop."""
        from . import codec

        device = archives[0].device
        n = own.numel() if own is not None else self.info(archives[0])[0]
        out = torch.empty(n, dtype=out_dtype, device=device)
        ok, _ = self._run(codec.sparse_reduce, device, [[a] for a in archives], [out],
                          inits=None if own is None else [own], ft=codec.FLOAT_TYPE[out_dtype])
        self._raise_on_failure(ok)
        return out

    def reduce_fits(self, numel, dtype, num_archives):
        """Whether one fused reduce of num_archives archives of numel words
        takes its scratch from this codec's workspace (the plan's bytes,
        codec.sparse_reduce_scratch_bytes): a call that does not would fall to
        the arena's hipMalloc path every time."""
        from . import codec

        need = codec.sparse_reduce_scratch_bytes(codec.FLOAT_TYPE[dtype], 1, num_archives, numel)
        return need <= max(int(self.workspace_bytes), 256)

    def info(self, archive):
        """(numel, dtype) of the element a sparse float archive encodes: numel
        from the sparse header, dtype from the dense header behind the bitmap
        (two small reads on the host)."""
        n = int(archive[:4].cpu().numpy().view("<u4")[0])
        at = 16 + _pad((n + 7) // 8)  # the sparse header, then the bitmap
        return n, super().info(archive[at:at + 32])[1]


def _check_sizes(sizes, what):
    """Archive sizes seen by every rank: 0 marks an element whose compression
    was abandoned (a bounded cross-workgroup wait ran out, see
    dietgpu_device_error_count); no valid archive is shorter than its headers.
    Raising here, where every rank sees the same sizes, keeps the ranks in
    step (a zero-length slot would otherwise alias the next archive and could
    decode into the wrong output)."""
    bad = (torch.as_tensor(sizes) <= 0).nonzero().view(-1).tolist()
    if bad:
        raise RuntimeError(f"{what}: compression of element(s) {bad[:8]} was abandoned (archive size 0)")


def _pack(comp, sizes, length, dev):
    """Pack the archive rows comp[i, :sizes[i]] back to back at the 16 B
    aligned offsets archive_offsets(sizes) into a buffer of `length` bytes:
    one masked gather over the [nb, cols] archive matrix (the 16 B tails of
    each row ride along as don't-care padding), no per-element launches."""
    cols = comp.shape[1]
    if cols % _ALIGN:
        comp = torch.nn.functional.pad(comp, (0, _ALIGN - cols % _ALIGN))
        cols = comp.shape[1]
    padded = _pad(torch.as_tensor(sizes, dtype=torch.int64)).to(comp.device)
    buf = torch.zeros(max(int(length), _ALIGN), dtype=torch.uint8, device=dev)
    mask = torch.arange(cols, device=comp.device)[None, :] < padded[:, None]
    flat = comp[mask]
    buf[: flat.numel()] = flat.to(dev)
    return buf


def _unpack(buf, sizes, base=0):
    """_pack's counterpart: the archive views buf[o:o + sizes[i]] of a buffer
    packed from `sizes` (a list) that starts at byte `base` of buf, o = base +
    the padded exclusive prefix of the sizes."""
    views = []
    for n in sizes:
        views.append(buf[base:base + n])
        base += _pad(n)
    return views


def _gather_table(numels, sizes, group, dev):
    """The one metadata exchange: this rank's k rows of (numel, archive size)
    are all-gathered (2 * k int64 per rank); returns every rank's rows as the
    host table t[rank][row] = [numel, size] (plain lists: [world, k, 2])."""
    meta = torch.tensor(list(zip(numels, sizes)), dtype=torch.int64, device=dev)
    world = dist.get_world_size(group)
    table = torch.empty([world * len(numels), 2], dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(table, meta, group=group)
    return table.view(world, len(numels), 2).tolist()


def all_gather_compressed(tensors, group=None, codec=None):
    """All-gather a list of float tensors in compressed form (SURVEY.md 8(f)
    rank 3: the compressed collectives the reference was built for,
    README.md:94-96).

    Every rank passes the same number k of tensors of one float dtype (shapes
    may differ between ranks).  Each rank compresses its tensors locally, the
    ranks all-gather (numel, archive size) per tensor, then ONE
    all_gather_into_tensor moves the packed archives (each rank's slot is the
    largest per-rank packed size) and every rank decompresses all of them.
    Returns the flat decoded tensors rank-major: [rank 0's k, rank 1's, ...].
    The codec is lossless: the result equals an uncompressed all-gather bit
    for bit.
    """
    codec = codec or GpuFloatCodec()
    world = dist.get_world_size(group)
    if len(tensors) == 0:
        return []
    dtype, dev = tensors[0].dtype, tensors[0].device
    flat = [t.contiguous().view(-1) for t in tensors]
    comp, sizes = codec.compress(flat)
    table = _gather_table([t.numel() for t in flat], sizes.tolist(), group, dev)  # [rank][tensor]
    asizes = [[size for _, size in rows] for rows in table]
    _check_sizes([size for rows in asizes for size in rows], "all_gather_compressed")
    span = max(max(sum(_pad(size) for size in rows) for rows in asizes), _ALIGN)  # per-rank packing, from 0
    send = _pack(comp, asizes[dist.get_rank(group)], span, dev)
    recv = torch.empty(world * span, dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    archives = [a for r in range(world) for a in _unpack(recv, asizes[r], r * span)]
    outs = [torch.empty(numel, dtype=dtype, device=dev) for rows in table for numel, _ in rows]
    codec.decompress(archives, outs)
    return outs


def _all_to_all_archives(flat, travels, what, group, codec, check_table=None):
    """The transport of all_to_all_compressed and reduce_scatter_compressed
    (`what` names the caller in messages): flat[j] is bound for rank j.

    travels(source, destination, numel) -> bool is the rule of who sends to
    whom; every rank evaluates it alike.  What travels from this rank is
    compressed in one batch (no codec call when nothing does); one all-gather
    exchanges the whole [source][destination] table of (numel, archive size),
    so every rank can run check_table(table) and then the size check over
    exactly the travelling entries, and a bad table raises on every rank
    before the payload moves; one all_to_all_single with the padded sizes as
    splits moves the packed archives (skipped on every rank alike when nothing
    travels anywhere).  Returns (archives, numels) of what this rank received,
    ascending source rank."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = flat[0].device
    numels = [t.numel() for t in flat]
    going = [j for j in range(world) if travels(rank, j, numels[j])]
    sizes = [0] * world
    comp = torch.zeros([0, _ALIGN], dtype=torch.uint8, device=dev)
    if going:
        comp, csz = codec.compress([flat[j] for j in going])
        for j, size in zip(going, csz.tolist()):
            sizes[j] = size
    table = _gather_table(numels, sizes, group, dev)  # row j of a rank goes to rank j
    if check_table is not None:
        check_table(table)
    # what travels, as (source, destination, archive size), sources ascending
    moving = [(src, dst, size) for src, row in enumerate(table) for dst, (numel, size) in enumerate(row)
              if travels(src, dst, numel)]
    _check_sizes([size for _, _, size in moving], what)
    lens = [0] * world  # what this rank sends to each destination
    rlens = [0] * world  # ... and receives from each source
    for src, dst, size in moving:
        if src == rank:
            lens[dst] = _pad(size)
        if dst == rank:
            rlens[src] = _pad(size)
    recv = torch.empty(max(sum(rlens), _ALIGN), dtype=torch.uint8, device=dev)
    if moving:  # (the same on every rank)
        send = _pack(comp, [sizes[j] for j in going], sum(lens), dev)
        dist.all_to_all_single(recv[: sum(rlens)], send[: sum(lens)],
                               output_split_sizes=rlens, input_split_sizes=lens, group=group)
    arrivals = [(src, size) for src, dst, size in moving if dst == rank]
    archives = _unpack(recv, [size for _, size in arrivals])
    return archives, [table[src][rank][0] for src, _ in arrivals]


def all_to_all_compressed(tensors, group=None, codec=None):
    """All-to-all of float tensors in compressed form: tensors[j] (one float
    dtype, any sizes) goes to rank j; returns the world tensors received,
    tensor r from rank r (flat).  This rank's outgoing tensors are compressed
    in one batch, the (numel, size) pairs are exchanged with one small
    all_to_all_single, the packed archives with one all_to_all_single whose
    split sizes are the packed lengths."""
    codec = codec or GpuFloatCodec()
    if len(tensors) != dist.get_world_size(group):
        raise ValueError("all_to_all_compressed: one tensor per destination rank")
    dtype, dev = tensors[0].dtype, tensors[0].device
    # everything travels, this rank's tensor to itself and empty ones included
    archives, numels = _all_to_all_archives([t.contiguous().view(-1) for t in tensors], lambda src, dst, numel: True,
                                            "all_to_all_compressed", group, codec)
    outs = [torch.empty(n, dtype=dtype, device=dev) for n in numels]
    codec.decompress(archives, outs)
    return outs


_FLOAT_DTYPES = {1: torch.float16, 2: torch.bfloat16, 3: torch.float32, 4: torch.float64}


def _archive_info(archive):
    """(numel, dtype) of a dense float archive, from its header (32 bytes read
    on the host)."""
    h = archive[:32].cpu().numpy().view("<u4")
    if h.size < 3 or int(h[0]) != 0xf00f0001 or int(h[2]) & 0xf not in _FLOAT_DTYPES:
        raise RuntimeError("reduce_archives: not a dense float archive")
    return int(h[1]), _FLOAT_DTYPES[int(h[2]) & 0xf]


def _acc_dtype(dtype, acc_dtype):
    if acc_dtype is None:
        return torch.float32 if dtype in (torch.float16, torch.bfloat16) else dtype
    if acc_dtype != dtype and not (acc_dtype == torch.float32 and dtype in (torch.float16, torch.bfloat16)):
        raise ValueError(f"acc_dtype {acc_dtype} does not go with {dtype}: the tensors' dtype, or float32 for "
                         "float16 / bfloat16")
    return acc_dtype


_FUSED_REDUCE_MAX = 64  # sources of one fused call (codec.REDUCE_MAX_SOURCES)


def _fused_entry(codec):
    """The codec's fused reduction f(own, archives, out_dtype), or None: its
    `reduce` (every peer's word added: GpuFloatCodec) or its `sparse_reduce`
    (a peer's zero words skipped: GpuSparseFloatCodec)."""
    return getattr(codec, "reduce", None) or getattr(codec, "sparse_reduce", None)


def _fused_reduce(codec, dtype, acc_dtype, num_archives, numel=None):
    """The routing rule of reduce_archives: the fused
    kernel takes the reduction when the codec has one (_fused_entry), the adds
    are float32 adds of float16, bfloat16 or float32 tensors, there are 1 ..
    64 archives, and the call's scratch fits the codec's workspace
    (codec.reduce_fits(numel, dtype, num_archives), where the codec has such a
    bound: GpuSparseFloatCodec decodes the nonzero lists of one launch's
    sources into its workspace; GpuFloatCodec has none, for it the clause is
    always true).  Everything else (a codec without a fused reduction, a
    16-bit accumulator that rounds at every add, float64, a shard too large
    for the workspace) keeps the per-peer loop.  Both give the same bits."""
    if not (_fused_entry(codec) is not None and acc_dtype == torch.float32
            and dtype in (torch.float16, torch.bfloat16, torch.float32) and 1 <= num_archives <= _FUSED_REDUCE_MAX):
        return False
    fits = getattr(codec, "reduce_fits", None)
    return fits is None or numel is None or bool(fits(numel, dtype, num_archives))


def reduce_archives(own, archives, codec, acc_dtype=None):
    """The local part of a compressed reduction: `own` (this rank's flat,
    uncompressed contribution) plus the elements of `archives` (the peers'
    archives, ascending rank order), added one after the other in that order,

        round_dtype((...((own + x_1) + x_2) + ...)),

    every add correctly rounded in acc_dtype (default: float32 for float16 /
    bfloat16 tensors, else the tensors' dtype) and the result rounded once to
    the tensors' dtype.  With float32 adds and a codec that has a fused
    reduction (GpuFloatCodec.reduce; GpuSparseFloatCodec.sparse_reduce while
    the call's scratch fits its workspace) the whole sum is one call of it,
    the running sum in registers (_fused_reduce states the rule); otherwise one
    codec.accumulate call per peer.  No decoded temporary either way, and the
    same bits.  The accumulator starts as `own` converted to acc_dtype, not as
    +0.0: with no archives the result is `own` bit for bit (-0.0 included).
    own=None: the first archive's element takes the place of `own` (its numel
    and dtype come from codec.info(archive), or from a dense float header when
    the codec has no info).
    With GpuSparseFloatCodec a peer's zero words are skipped: the sum runs
    over the peers whose word is nonzero, which is the same value except that
    a running sum of -0.0 stays -0.0 where a peer holds +0.0."""
    if own is None and not archives:
        raise ValueError("reduce_archives: nothing to reduce")
    numel, dtype = ((own.numel(), own.dtype) if own is not None
                    else getattr(codec, "info", _archive_info)(archives[0]))
    if _fused_reduce(codec, dtype, _acc_dtype(dtype, acc_dtype), len(archives), numel):
        flat = None if own is None else own.contiguous().view(-1)
        return _fused_entry(codec)(flat, archives, dtype)
    if own is None:
        n, dtype = getattr(codec, "info", _archive_info)(archives[0])
        own = torch.empty(n, dtype=dtype, device=archives[0].device)
        codec.decompress([archives[0]], [own])
        archives = archives[1:]
    dtype = own.dtype
    acc = own.contiguous().view(-1).to(_acc_dtype(dtype, acc_dtype), copy=True)
    for a in archives:
        codec.accumulate([a], [acc])
    return acc.to(dtype)


def reduce_scatter_compressed(tensors, group=None, codec=None, acc_dtype=None):
    """Reduce-scatter (sum) of float tensors with compressed traffic:
    tensors[j] is this rank's contribution to rank j's result; every rank's
    tensors[j] has the same numel and dtype.  Returns this rank's flat reduced
    tensor: element i is

        round_dtype((...((x_j + x_r1) + x_r2) + ...)),

    x_j this rank's own tensors[j] (never compressed), r1 < r2 < ... the
    other ranks ascending, every add done in acc_dtype (reduce_archives).  The
    order is fixed, so the result is deterministic and reproducible; it is not
    the order of RCCL's ring, so it is not bit-equal to dist.reduce_scatter.
    With codec=GpuSparseFloatCodec() the archives are sparse and a peer's zero
    words are skipped: element i is that sum over the peers whose word i is
    nonzero, equal to the dense codec's result except that a running sum of
    -0.0 stays -0.0 where a peer's word is +0.0.

    The W - 1 outgoing tensors are compressed in one batch; one all-gather
    exchanges the whole (source, destination) table of (numel, archive size),
    so an abandoned archive or a numel mismatch raises on every rank before
    the payload moves; one all_to_all_single moves the packed archives."""
    codec = codec or GpuFloatCodec()
    world = dist.get_world_size(group)
    if len(tensors) != world:
        raise ValueError("reduce_scatter_compressed: one tensor per destination rank")
    _acc_dtype(tensors[0].dtype, acc_dtype)
    flat = [t.contiguous().view(-1) for t in tensors]

    def same_numels(table):
        for j in range(world):
            col = [row[j][0] for row in table]
            if col != col[:1] * world:
                raise RuntimeError(f"reduce_scatter_compressed: the ranks' tensors[{j}] differ in numel: {col}")

    # the tensors that travel: every destination but the rank itself, empties aside
    archives, _ = _all_to_all_archives(flat, lambda src, dst, numel: src != dst and numel > 0,
                                       "reduce_scatter_compressed", group, codec, same_numels)
    return reduce_archives(flat[dist.get_rank(group)], archives, codec, acc_dtype)


def all_reduce_compressed(tensor, group=None, codec=None, acc_dtype=None):
    """All-reduce (sum) of a float tensor with compressed traffic: a
    reduce_scatter_compressed of the contiguous shards shard_range(numel, r, W)
    of the flattened tensor, then an all_gather_compressed of the reduced
    shards.  Element i of rank j's shard is summed in the order documented
    there (rank j's own value first, the other ranks ascending, in acc_dtype,
    rounded once), and the lossless all-gather hands every rank the same
    bits.  Shards may be empty (numel < W).  Returns a tensor of the input's
    shape.  codec=GpuSparseFloatCodec(): both steps move sparse archives, and
    the reduction skips the peers' zero words (reduce_scatter_compressed)."""
    codec = codec or GpuFloatCodec()
    world = dist.get_world_size(group)
    flat = tensor.contiguous().view(-1)
    if flat.numel() == 0:
        return tensor.clone()
    ranges = [shard_range(flat.numel(), r, world) for r in range(world)]
    mine = reduce_scatter_compressed([flat[a:b] for a, b in ranges], group=group, codec=codec, acc_dtype=acc_dtype)
    # (a rank whose shard is empty sends one word that nobody keeps: every
    # rank knows the shard sizes)
    send = mine if mine.numel() else torch.zeros(1, dtype=flat.dtype, device=flat.device)
    got = all_gather_compressed([send], group=group, codec=codec)
    return torch.cat([g[: b - a] for g, (a, b) in zip(got, ranges)]).view(tensor.shape)
