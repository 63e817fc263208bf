"""gloo tests (CPU, world 2 and 3) of the reducing compressed collectives of
dietgpu_fork_amd/dist.py: reduce_scatter_compressed, all_reduce_compressed
and reduce_archives against the documented summation order, bit for bit.

The codec is a stand-in backed by the CPU oracle; its accumulate is the CPU
model of tests/accumulate_cases.py, so these tests cover the collectives'
bookkeeping and order, and tests/test_gpu_accumulate.py the kernel."""
import os

import numpy as np
import pytest
import torch

from tests import accumulate_cases as A
from tests.dist_cases import FT_OF, OracleCodec, numels, run_ranks, save_bits, sizes_for

DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def contribution(dtype, src, dst, n, tag=0):
    """What rank src contributes to rank dst's result; values that round and
    cancel, signed zeros among them."""
    x = A.random_acc(FT_OF[dtype], 1, n, seed=1000 * tag + 10 * src + dst)
    x[::7] = -0.0
    if src > 0 and n > 3:
        x[3] = -contribution(dtype, 0, dst, n, tag)[3]  # an exact cancellation against rank 0
    return x


def documented_sum(dtype, parts, own, acc_dtype=None):
    """round_dtype((...((x_own + x_r1) + x_r2) + ...)), r1 < r2 < ... the other
    ranks ascending, every add in acc_dtype."""
    ft = FT_OF[dtype]
    ad = acc_dtype or (torch.float32 if ft <= 2 else dtype)
    mode = 1 if ad == dtype else 2
    acc = parts[own].to(ad)
    for r, p in enumerate(parts):
        if r != own:
            acc = A.model(acc, p, mode)
    return acc.to(dtype)


def _reduce_worker(rank, world, outdir):
    from dietgpu_fork_amd import dist as D

    codec = OracleCodec()
    for di, dtype in enumerate(DTYPES):
        for n in sizes_for(world):
            ts = [contribution(dtype, rank, j, m, tag=di) for j, m in enumerate(numels(world, n))]
            keep = [t.clone() for t in ts]
            got = D.reduce_scatter_compressed(ts, codec=codec)
            assert got.dtype == dtype and got.dim() == 1
            assert all(torch.equal(A.bits(a), A.bits(b)) for a, b in zip(ts, keep))
            save_bits(outdir, f"rs_{di}_{n}_{rank}", got)
            x = contribution(dtype, rank, 99, n, tag=di).view(-1, 1) if n else contribution(dtype, rank, 99, n)
            got = D.all_reduce_compressed(x, codec=codec)
            assert got.shape == x.shape and got.dtype == dtype
            save_bits(outdir, f"ar_{di}_{n}_{rank}", got.reshape(-1))
    # the sum kept in bf16 itself
    ts = [contribution(torch.bfloat16, rank, j, 4097, tag=7) for j in range(world)]
    save_bits(outdir, f"rsbf_{rank}", D.reduce_scatter_compressed(ts, codec=codec, acc_dtype=torch.bfloat16))


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_scatter_and_all_reduce_follow_the_documented_order(tmp_path, world):
    run_ranks(_reduce_worker, world, tmp_path)
    for di, dtype in enumerate(DTYPES):
        it = A.TORCH_INT[dtype]
        for n in sizes_for(world):
            for rank in range(world):
                m = numels(world, n)[rank]
                parts = [contribution(dtype, src, rank, m, tag=di) for src in range(world)]
                want = documented_sum(dtype, parts, rank)
                got = torch.from_numpy(np.load(tmp_path / f"rs_{di}_{n}_{rank}.npy")).view(dtype)
                assert got.numel() == m and A.same_bits(got, want), (dtype, n, rank, A.mismatch_report(got, want))
                if m > 3:  # rank 0 and 1 cancel exactly at [3]: not -0.0
                    assert world > 2 or A.bits(got)[3].item() == 0
            # all-reduce: shard j is summed on rank j, own value first
            full = [contribution(dtype, src, 99, n, tag=di) for src in range(world)]
            per = -(-n // world)
            want = torch.cat([documented_sum(dtype, [f[j * per:(j + 1) * per] for f in full], j)
                              for j in range(world)]) if n else torch.zeros(0, dtype=dtype)
            outs = [torch.from_numpy(np.load(tmp_path / f"ar_{di}_{n}_{rank}.npy")).view(dtype) for rank in range(world)]
            assert A.same_bits(outs[0], want), (dtype, n, A.mismatch_report(outs[0], want))
            for o in outs[1:]:  # every rank returns identical bits
                assert torch.equal(o.view(it), outs[0].view(it))
    for rank in range(world):
        parts = [contribution(torch.bfloat16, src, rank, 4097, tag=7) for src in range(world)]
        want = documented_sum(torch.bfloat16, parts, rank, acc_dtype=torch.bfloat16)
        got = torch.from_numpy(np.load(tmp_path / f"rsbf_{rank}.npy")).view(torch.bfloat16)
        assert A.same_bits(got, want)
        # a bf16 running sum rounds at every add: it differs from the fp32-accumulated one
        assert world == 2 or not A.same_bits(got, documented_sum(torch.bfloat16, parts, rank))


def test_the_order_matters_in_the_inputs_used():
    """The documented order is told apart from the plain ascending one by the
    inputs above (so the comparison can fail): world 3, rank 2's shard."""
    parts = [contribution(torch.float32, src, 2, 12345 + 200, tag=2) for src in range(3)]
    own_first = documented_sum(torch.float32, parts, 2)
    ascending = (parts[0] + parts[1]) + parts[2]
    assert not A.same_bits(own_first, ascending)


def _error_worker(rank, world, outdir):
    from dietgpu_fork_amd import dist as D

    msgs = []
    # rank 1's tensors[0] is one word longer than everybody else's
    ts = [contribution(torch.bfloat16, rank, j, 500 + (rank == 1 and j == 0)) for j in range(world)]
    # then: rank 1 reports its first outgoing archive as abandoned
    for tensors, codec in ((ts, OracleCodec()),
                           ([contribution(torch.bfloat16, rank, j, 500) for j in range(world)],
                            OracleCodec(poison=0 if rank == 1 else None))):
        try:
            D.reduce_scatter_compressed(tensors, codec=codec)
            msgs.append("no error")
        except RuntimeError as e:
            msgs.append(str(e))
    try:
        D.all_reduce_compressed(contribution(torch.float16, rank, 0, 3000),
                                codec=OracleCodec(poison=0 if rank == 1 else None))
        msgs.append("no error")
    except RuntimeError as e:
        msgs.append(str(e))
    with open(os.path.join(outdir, f"err{rank}.txt"), "w") as f:
        f.write("\n".join(msgs))


@pytest.mark.parametrize("world", [2, 3])
def test_numel_mismatch_and_abandoned_archive_raise_on_every_rank(tmp_path, world):
    run_ranks(_error_worker, world, tmp_path)
    for rank in range(world):
        msgs = (tmp_path / f"err{rank}.txt").read_text().split("\n")
        assert len(msgs) == 3, msgs
        assert "reduce_scatter_compressed" in msgs[0] and "differ in numel" in msgs[0] and "tensors[0]" in msgs[0], msgs
        assert "reduce_scatter_compressed" in msgs[1] and "abandoned" in msgs[1], msgs
        assert "reduce_scatter_compressed" in msgs[2] and "abandoned" in msgs[2], msgs


def test_reduce_archives_locally():
    from dietgpu_fork_amd import dist as D

    codec = OracleCodec()
    for dtype in DTYPES:
        parts = [contribution(dtype, src, 0, 4097, tag=3) for src in range(4)]
        comp, sizes = codec.compress(parts[1:])
        archives = [comp[i, : int(sizes[i])] for i in range(3)]
        got = D.reduce_archives(parts[0], archives, codec)
        assert got.dtype == dtype and A.same_bits(got, documented_sum(dtype, parts, 0))
        # own=None: the first archive's element takes its place
        got = D.reduce_archives(None, archives, codec)
        assert A.same_bits(got, documented_sum(dtype, parts[1:], 0))
        # no peers: the input bit for bit, -0.0 included, in a new tensor
        got = D.reduce_archives(parts[0], [], codec)
        assert torch.equal(A.bits(got), A.bits(parts[0])) and bool(torch.signbit(got[0])) and got is not parts[0]
    with pytest.raises(ValueError, match="nothing to reduce"):
        D.reduce_archives(None, [], codec)
    with pytest.raises(ValueError, match="does not go with"):
        D.reduce_archives(parts[0], [], codec, acc_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="not a dense float archive"):
        D.reduce_archives(None, [torch.zeros(64, dtype=torch.uint8)], codec)
