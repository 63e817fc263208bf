"""The harness of the compressed collectives' tests (dietgpu_fork_amd/dist.py):
the gloo process launcher, the oracle-backed stand-in codec and the small
helpers of tests/test_dist.py, tests/test_dist_reduce.py,
tests/test_dist_sparse_reduce.py and tests/test_dist_protocol.py on the CPU,
and the world-1 NCCL process group of the GPU modules."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import accumulate_cases as A
from tests import sparse_accumulate_cases as S
from tests.util import FT_OF


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, worker, world, port, outdir, args):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        worker(rank, world, outdir, *args)
    finally:
        dist.destroy_process_group()


def run_ranks(worker, world, tmp_path, *args):
    """worker(rank, world, outdir, *args) in `world` processes that form a
    gloo group; returns when all of them have ended."""
    mp.spawn(_rank, args=(worker, world, free_port(), str(tmp_path), args), nprocs=world, join=True)


@pytest.fixture(scope="module")
def pg():
    """World 1 over RCCL on GPU 0, for the module that imports this name."""
    import dietgpu_fork_amd  # noqa: F401

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class OracleCodec:
    """CPU stand-in for dist.GpuFloatCodec or, with sparse=True, for
    dist.GpuSparseFloatCodec: the oracle's archives (the same as the GPU
    path's), the CPU model's accumulate (tests/accumulate_cases.model, or
    tests/sparse_accumulate_cases.expected, which skips the zero words).
    poison: report the archive of that outgoing index as abandoned (size 0).
    log: a list that receives [method, numels in, numels out] per call."""

    def __init__(self, sparse=False, poison=None, log=None):
        self.sparse, self.poison, self.log = sparse, poison, log
        if sparse:  # the dense stand-in has no info: reduce_archives reads the dense header itself
            self.info = self._sparse_info

    def _note(self, method, ins, outs):
        if self.log is not None:
            self.log.append([method, [int(n) for n in ins], [int(n) for n in outs]])

    def compress(self, tensors):
        from oracle import oracle as O

        enc = O.sparse_compress if self.sparse else O.float_compress
        arch = [enc(A.float_to_words(t, FT_OF[t.dtype]), FT_OF[t.dtype], 10) for t in tensors]
        comp = torch.zeros(len(arch), max(a.size for a in arch), dtype=torch.uint8)
        for i, a in enumerate(arch):
            comp[i, : a.size] = torch.from_numpy(a)
        sizes = torch.tensor([a.size for a in arch], dtype=torch.int32)
        if self.poison is not None:
            sizes[self.poison] = 0
        self._note("compress", [t.numel() for t in tensors], sizes)
        return comp, sizes

    @staticmethod
    def _sparse_info(archive):
        """(numel, dtype) from the sparse header and the dense one behind the bitmap."""
        a = archive.numpy()
        n = int(a[0:4].view(np.uint32)[0])
        at = 16 + (((n + 7) // 8 + 15) // 16) * 16
        assert int(a[at:at + 4].view(np.uint32)[0]) == 0xf00f0001
        return n, A.TORCH_FLOAT[int(a[at + 8]) & 0xf]

    def _words(self, archive):
        """(words, float type) of the element an archive encodes."""
        from oracle import oracle as O

        if self.sparse:
            ft = FT_OF[self._sparse_info(archive)[1]]
            st, words = O.sparse_decompress(archive.numpy(), ft, 10)
        else:
            ft = int(archive[8]) & 0xf  # the header's type word
            st, words = O.float_decompress(archive.numpy(), ft, 10)
        assert st == 0
        return words, ft

    def decompress(self, archives, outs):
        self._note("decompress", [a.numel() for a in archives], [o.numel() for o in outs])
        for a, o in zip(archives, outs):
            words, ft = self._words(a)
            assert words.size == o.numel() and FT_OF[o.dtype] == ft
            o.copy_(A.words_to_float(words, ft))

    def accumulate(self, archives, accs):
        self._note("accumulate", [a.numel() for a in archives], [acc.numel() for acc in accs])
        for a, acc in zip(archives, accs):
            words, ft = self._words(a)
            mode = 1 if FT_OF[acc.dtype] == ft else 2
            acc.copy_(S.expected(acc, words, ft, mode) if self.sparse
                      else A.model(acc, A.words_to_float(words, ft), mode))


def save_bits(outdir, name, t):
    np.save(os.path.join(outdir, name + ".npy"), A.bits(t).numpy())


def numels(world, n):
    """tensors[j]'s numel: n for every j, except that the large case varies it."""
    return [n + 100 * j if n > 1000 else n for j in range(world)]


def sizes_for(world):
    return (0, 1, world - 1, 12345)
