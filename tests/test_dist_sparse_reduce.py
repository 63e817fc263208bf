"""gloo tests (CPU, world 2 and 3) of the reducing compressed collectives of
dietgpu_fork_amd/dist.py with a SPARSE codec: reduce_scatter_compressed,
all_reduce_compressed and reduce_archives against the documented summation
order, in which a peer's zero words are skipped, bit for bit.

The codec is a stand-in backed by the CPU oracle's sparse compressor; its
accumulate is the sparse model of tests/sparse_accumulate_cases.py, so these
tests cover the collectives' bookkeeping, the order and the codec's `info`,
and tests/test_gpu_sparse_accumulate.py the kernel."""
import os

import numpy as np
import pytest
import torch

from tests import sparse_accumulate_cases as S
from tests.dist_cases import FT_OF, OracleCodec, numels, run_ranks, save_bits, sizes_for

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
ZERO_RANK = 1  # the rank whose contributions are all zero


def contribution(dtype, src, dst, n, tag=0):
    """What rank src contributes to rank dst's result: 90 % zeros (rank
    ZERO_RANK: all zeros), -0.0 among the nonzero words, an exact cancellation
    against rank 0 at [3], and at [5] rank 0 holds -0.0 where every other rank
    holds +0.0."""
    ft = FT_OF[dtype]
    x = S.random_acc(ft, 1, n, seed=1000 * tag + 10 * src + dst)
    g = torch.Generator().manual_seed(77 + 1000 * tag + 10 * src + dst)
    x[torch.rand(n, generator=g) < 0.9] = 0.0
    x[1::7] = -0.0
    if src == ZERO_RANK:
        x = torch.zeros(n, dtype=dtype)
    if n > 5:
        if src == 0:
            x[3] = 1.5
            x[5] = -0.0
        else:
            x[3] = -1.5 if src == 2 else 0.0
            x[5] = 0.0
    return x


def documented_sum(dtype, parts, own, acc_dtype=None):
    """round_dtype((...((x_own + x_r1) + x_r2) + ...)) over the peers whose
    word is nonzero, r1 < r2 < ... the other ranks ascending, every add in
    acc_dtype."""
    ft = FT_OF[dtype]
    ad = acc_dtype or (torch.float32 if ft <= 2 else dtype)
    mode = 1 if ad == dtype else 2
    acc = parts[own].to(ad)
    for r, p in enumerate(parts):
        if r != own:
            acc = S.expected(acc, S.float_to_words(p, ft), ft, mode)
    return acc.to(dtype)


def _reduce_worker(rank, world, outdir):
    from dietgpu_fork_amd import dist as D

    codec = OracleCodec(sparse=True)
    for di, dtype in enumerate(DTYPES):
        for n in sizes_for(world):
            ts = [contribution(dtype, rank, j, m, tag=di) for j, m in enumerate(numels(world, n))]
            keep = [t.clone() for t in ts]
            got = D.reduce_scatter_compressed(ts, codec=codec)
            assert got.dtype == dtype and got.dim() == 1
            assert all(torch.equal(S.bits(a), S.bits(b)) for a, b in zip(ts, keep))
            save_bits(outdir, f"rs_{di}_{n}_{rank}", got)
            x = contribution(dtype, rank, 99, n, tag=di).view(-1, 1) if n else contribution(dtype, rank, 99, n)
            got = D.all_reduce_compressed(x, codec=codec)
            assert got.shape == x.shape and got.dtype == dtype
            save_bits(outdir, f"ar_{di}_{n}_{rank}", got.reshape(-1))
    msg = "no error"
    try:  # rank 1's tensors[0] is one word longer than everybody else's
        D.reduce_scatter_compressed([contribution(torch.bfloat16, rank, j, 500 + (rank == 1 and j == 0))
                                     for j in range(world)], codec=codec)
    except RuntimeError as e:
        msg = str(e)
    with open(os.path.join(outdir, f"err{rank}.txt"), "w") as f:
        f.write(msg)


@pytest.mark.parametrize("world", [2, 3])
def test_sparse_reduce_scatter_and_all_reduce_follow_the_documented_order(tmp_path, world):
    run_ranks(_reduce_worker, world, tmp_path)
    for di, dtype in enumerate(DTYPES):
        it = S.bits(torch.zeros(1, dtype=dtype)).dtype
        for n in sizes_for(world):
            for rank in range(world):
                m = numels(world, n)[rank]
                parts = [contribution(dtype, src, rank, m, tag=di) for src in range(world)]
                want = documented_sum(dtype, parts, rank)
                got = torch.from_numpy(np.load(tmp_path / f"rs_{di}_{n}_{rank}.npy")).view(dtype)
                assert got.numel() == m and S.same_bits(got, want), (dtype, n, rank, S.mismatch_report(got, want))
                if m > 5 and rank == 0:
                    # rank 0's -0.0 under the peers' +0.0 stays -0.0 (the dense collectives give +0.0)
                    assert S.bits(got)[5].item() == S.bits(torch.tensor([-0.0], dtype=dtype))[0].item()
                    # and the exact cancellation 1.5 + (-1.5) at world 3 is +0.0
                    assert world == 2 or S.bits(got)[3].item() == 0
                if m > 5 and rank == ZERO_RANK:
                    assert not parts[ZERO_RANK].any()  # its own contribution is all zero: the peers' sum
            full = [contribution(dtype, src, 99, n, tag=di) for src in range(world)]
            per = -(-n // world)
            want = torch.cat([documented_sum(dtype, [f[j * per:(j + 1) * per] for f in full], j)
                              for j in range(world)]) if n else torch.zeros(0, dtype=dtype)
            outs = [torch.from_numpy(np.load(tmp_path / f"ar_{di}_{n}_{rank}.npy")).view(dtype) for rank in range(world)]
            assert S.same_bits(outs[0], want), (dtype, n, S.mismatch_report(outs[0], want))
            for o in outs[1:]:  # every rank returns identical bits
                assert torch.equal(o.view(it), outs[0].view(it))
    for rank in range(world):  # the numel mismatch raised on every rank
        msg = (tmp_path / f"err{rank}.txt").read_text()
        assert "reduce_scatter_compressed" in msg and "differ in numel" in msg and "tensors[0]" in msg, msg


def test_the_inputs_tell_the_sparse_sum_from_the_dense_one():
    """Rank 0's shard at world 3: the skipped zeros and the order both show."""
    from tests import accumulate_cases as A

    parts = [contribution(torch.float32, src, 0, 12345, tag=2) for src in range(3)]
    sparse = documented_sum(torch.float32, parts, 0)
    dense = A.model(A.model(parts[0], parts[1], 1), parts[2], 1)
    assert not S.same_bits(sparse, dense)
    assert bool(torch.signbit(sparse[5])) and not bool(torch.signbit(dense[5]))
    parts = [contribution(torch.float32, src, 2, 12345 + 200, tag=2) for src in range(3)]
    ascending = S.expected(S.expected(parts[0], S.float_to_words(parts[1], 3), 3, 1), S.float_to_words(parts[2], 3), 3, 1)
    assert not S.same_bits(documented_sum(torch.float32, parts, 2), ascending)


def test_reduce_archives_reads_the_codecs_info():
    from dietgpu_fork_amd import dist as D

    codec = OracleCodec(sparse=True)
    for dtype in DTYPES:
        parts = [contribution(dtype, src, 0, 4097, tag=3) for src in (0, 2, 3, 4)]
        comp, sizes = codec.compress(parts[1:])
        archives = [comp[i, : int(sizes[i])] for i in range(3)]
        assert codec.info(archives[0]) == (4097, dtype)
        got = D.reduce_archives(parts[0], archives, codec)
        assert got.dtype == dtype and S.same_bits(got, documented_sum(dtype, parts, 0))
        # own=None: the first archive's element takes its place; a sparse
        # archive has no dense header up front, so the codec's info is what reads it
        got = D.reduce_archives(None, archives, codec)
        assert S.same_bits(got, documented_sum(dtype, parts[1:], 0))
        with pytest.raises(RuntimeError, match="not a dense float archive"):
            D._archive_info(archives[0])
        # no peers: the input bit for bit, -0.0 included
        got = D.reduce_archives(parts[0], [], codec)
        assert torch.equal(S.bits(got), S.bits(parts[0])) and bool(torch.signbit(got[5]))
