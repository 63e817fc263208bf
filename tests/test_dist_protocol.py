"""What the compressed collectives of dietgpu_fork_amd/dist.py send (CPU,
gloo, world 2 and 3): which torch.distributed calls, in which order, with
which dtype, sizes and splits, and which codec calls with which batches.

Every rank wraps all_gather_into_tensor and all_to_all_single and runs the
collectives with the logging stand-in codec (tests/dist_cases.OracleCodec).
The expected log is worked out here, in the parent process, from the oracle's
archive sizes and the rules the docstrings of dist.py state; dist.py is not
used for it.  The other collective tests compare results; this one pins the
traffic, so a change of dist.py that moves different bytes, or asks the codec
for other batches, shows here."""
import json
import os

import pytest
import torch
import torch.distributed as dist

from tests import accumulate_cases as A
from tests.dist_cases import OracleCodec, run_ranks

K = 3  # tensors per rank in the all-gather
U8, I64 = "torch.uint8", "torch.int64"


def pad(n):
    return -(-n // 16) * 16


def gather_input(rank, j):
    return A.random_acc(2, 1, 100 * (rank + 1) + j, seed=10 * rank + j)


def a2a_input(src, dst):  # rank 0's tensor to itself is empty
    return A.random_acc(2, 1, 50 * src + 7 * dst, seed=100 + 10 * src + dst)


def _marked(x, src):
    """x with every (src + 2)th word 1.0: the sources' archives of one size
    of tensor then differ in size, so the log tells their order."""
    x[::src + 2] = 1.0
    return x


def rs_input(src, dst, n):
    return _marked(A.random_acc(2, 1, n, seed=200 + 10 * src + dst), src)


def ar_input(rank, n):
    return _marked(A.random_acc(1, 1, n, seed=300 + rank), rank)


def reduce_sizes(world):
    return (0, 1, world - 1, 5000)


def _attempt(f, *args, **kw):
    try:
        f(*args, **kw)
        return "no error"
    except (RuntimeError, ValueError) as e:
        return f"{type(e).__name__}: {e}"


def _worker(rank, world, outdir):
    from dietgpu_fork_amd import dist as D

    log = []
    gather, exchange = dist.all_gather_into_tensor, dist.all_to_all_single

    def logged_gather(out, inp, group=None):
        log.append(["all_gather_into_tensor", str(inp.dtype), inp.numel(), out.numel()])
        return gather(out, inp, group=group)

    def logged_exchange(out, inp, output_split_sizes=None, input_split_sizes=None, group=None):
        log.append(["all_to_all_single", str(inp.dtype), inp.numel(), out.numel(),
                    list(input_split_sizes), list(output_split_sizes)])
        return exchange(out, inp, output_split_sizes=output_split_sizes, input_split_sizes=input_split_sizes,
                        group=group)

    dist.all_gather_into_tensor, dist.all_to_all_single = logged_gather, logged_exchange
    logs = {}

    def section(name):
        nonlocal log
        log = logs[name] = []
        return OracleCodec(log=log)

    D.all_gather_compressed([gather_input(rank, j) for j in range(K)], codec=section("ag"))
    D.all_to_all_compressed([a2a_input(rank, d) for d in range(world)], codec=section("a2a"))
    for n in reduce_sizes(world):
        D.reduce_scatter_compressed([rs_input(rank, d, n) for d in range(world)], codec=section(f"rs{n}"))
        D.all_reduce_compressed(ar_input(rank, n), codec=section(f"ar{n}"))

    # what must raise on every rank with nothing moved: rank 1 reports its
    # first outgoing archive as abandoned, or its tensors[0] is a word longer
    def poisoned(name):
        codec = section(name)
        codec.poison = 0 if rank == 1 else None
        return codec

    raised = {}
    raised["ag_poison"] = _attempt(D.all_gather_compressed, [gather_input(rank, j) for j in range(K)],
                                   codec=poisoned("ag_poison"))
    raised["a2a_poison"] = _attempt(D.all_to_all_compressed, [a2a_input(rank, d) for d in range(world)],
                                    codec=poisoned("a2a_poison"))
    raised["rs_poison"] = _attempt(D.reduce_scatter_compressed, [rs_input(rank, d, 500) for d in range(world)],
                                   codec=poisoned("rs_poison"))
    raised["ar_poison"] = _attempt(D.all_reduce_compressed, ar_input(rank, 3000), codec=poisoned("ar_poison"))
    raised["rs_numel"] = _attempt(D.reduce_scatter_compressed,
                                  [rs_input(rank, d, 500 + (rank == 1 and d == 0)) for d in range(world)],
                                  codec=section("rs_numel"))
    # argument errors: before any communication, the list's length first
    extra = [rs_input(rank, d, 8) for d in range(world + 1)]
    raised["a2a_count"] = _attempt(D.all_to_all_compressed, extra, codec=section("a2a_count"))
    raised["rs_count"] = _attempt(D.reduce_scatter_compressed, extra, codec=section("rs_count"),
                                  acc_dtype=torch.float16)
    raised["rs_acc"] = _attempt(D.reduce_scatter_compressed, extra[:world], codec=section("rs_acc"),
                                acc_dtype=torch.float16)
    raised["ar_acc"] = _attempt(D.all_reduce_compressed, ar_input(rank, 64), codec=section("ar_acc"),
                                acc_dtype=torch.bfloat16)
    with open(os.path.join(outdir, f"log{rank}.json"), "w") as f:
        json.dump({"logs": logs, "raised": raised}, f)


@pytest.fixture(scope="module", params=[2, 3], ids=["world2", "world3"])
def ranks(request, tmp_path_factory):
    """(world, [what rank r logged]) of one run of _worker per world size."""
    world = request.param
    out = tmp_path_factory.mktemp(f"protocol{world}")
    run_ranks(_worker, world, out)
    return world, [json.loads((out / f"log{r}.json").read_text()) for r in range(world)]


_SIZE = {}


def size(t):
    """The archive size of a tensor: the oracle's, each tensor compressed once."""
    from oracle import oracle as O

    ft = {torch.float16: 1, torch.bfloat16: 2}[t.dtype]
    key = (ft, A.bits(t).numpy().tobytes())
    if key not in _SIZE:
        _SIZE[key] = int(O.float_compress(A.float_to_words(t, ft), ft, 10).size)
    return _SIZE[key]


def gather_lines(world, rank, tensors):
    """all_gather_compressed of tensors[r][i], as rank `rank` logs it."""
    k = len(tensors[0])
    span = max(max(sum(pad(size(t)) for t in ts) for ts in tensors), 16)
    return [["compress", [t.numel() for t in tensors[rank]], [size(t) for t in tensors[rank]]],
            ["all_gather_into_tensor", I64, 2 * k, 2 * k * world],
            ["all_gather_into_tensor", U8, span, world * span],
            ["decompress", [size(t) for ts in tensors for t in ts], [t.numel() for ts in tensors for t in ts]]]


def table_line(world):
    return ["all_gather_into_tensor", I64, 2 * world, 2 * world * world]


def reduce_lines(world, rank, tensors):
    """reduce_scatter_compressed of tensors[src][dst], as rank `rank` logs it:
    a tensor travels unless it is the rank's own or empty."""
    def travels(src, dst):
        return src != dst and tensors[src][dst].numel() > 0

    going = [tensors[rank][d] for d in range(world) if travels(rank, d)]
    lines = [["compress", [t.numel() for t in going], [size(t) for t in going]]] if going else []
    lines.append(table_line(world))
    if any(travels(s, d) for s in range(world) for d in range(world)):
        ins = [pad(size(tensors[rank][d])) if travels(rank, d) else 0 for d in range(world)]
        outs = [pad(size(tensors[s][rank])) if travels(s, rank) else 0 for s in range(world)]
        lines.append(["all_to_all_single", U8, sum(ins), sum(outs), ins, outs])
    lines += [["accumulate", [size(tensors[s][rank])], [tensors[rank][rank].numel()]]
              for s in range(world) if travels(s, rank)]
    return lines


def reduced(parts, own):
    """The documented sum of 16-bit tensors: own first, the others ascending, in float32."""
    acc = parts[own].float()
    for r, p in enumerate(parts):
        if r != own:
            acc = A.model(acc, p, 2)
    return acc.to(parts[own].dtype)


def test_all_gather_traffic(ranks):
    world, got = ranks
    tensors = [[gather_input(r, j) for j in range(K)] for r in range(world)]
    for rank in range(world):
        assert got[rank]["logs"]["ag"] == gather_lines(world, rank, tensors), rank


def test_all_to_all_traffic(ranks):
    world, got = ranks
    t = [[a2a_input(s, d) for d in range(world)] for s in range(world)]
    assert t[0][0].numel() == 0 and size(t[0][0]) > 0  # the empty element travels as an archive
    for rank in range(world):
        ins = [pad(size(t[rank][d])) for d in range(world)]
        outs = [pad(size(t[s][rank])) for s in range(world)]
        want = [["compress", [x.numel() for x in t[rank]], [size(x) for x in t[rank]]],
                table_line(world),
                ["all_to_all_single", U8, sum(ins), sum(outs), ins, outs],
                ["decompress", [size(t[s][rank]) for s in range(world)], [t[s][rank].numel() for s in range(world)]]]
        assert got[rank]["logs"]["a2a"] == want, rank


def test_reduce_scatter_traffic(ranks):
    world, got = ranks
    for n in reduce_sizes(world):
        tensors = [[rs_input(s, d, n) for d in range(world)] for s in range(world)]
        for rank in range(world):
            want = reduce_lines(world, rank, tensors)
            assert got[rank]["logs"][f"rs{n}"] == want, (n, rank)
            assert all(line[0] != "decompress" for line in want)
            # n = 0: the table alone; else one accumulate per peer
            assert len(want) == (1 if n == 0 else 3 + world - 1)
            if n == 5000:  # the peers' archives differ in size: their order shows
                assert len({size(tensors[s][rank]) for s in range(world) if s != rank}) == world - 1


def test_all_reduce_traffic(ranks):
    world, got = ranks
    for n in reduce_sizes(world):
        if n == 0:  # an empty tensor is returned as it is: no call at all
            assert all(got[rank]["logs"]["ar0"] == [] for rank in range(world))
            continue
        per = -(-n // world)
        full = [ar_input(r, n) for r in range(world)]
        shards = [[f[min(n, d * per):min(n, (d + 1) * per)] for d in range(world)] for f in full]
        # the all-gather's tensors: each rank's reduced shard, one zero word where it is empty
        mine = [[reduced([shards[s][r] for s in range(world)], r)] if shards[r][r].numel()
                else [torch.zeros(1, dtype=torch.float16)] for r in range(world)]
        for rank in range(world):
            want = reduce_lines(world, rank, shards) + gather_lines(world, rank, mine)
            assert got[rank]["logs"][f"ar{n}"] == want, (n, rank)


def test_nothing_moves_after_a_bad_table(ranks):
    """An abandoned archive or a numel mismatch raises on every rank after the
    table all-gather, before any payload call and any decode."""
    world, got = ranks
    for rank in range(world):
        logs, raised = got[rank]["logs"], got[rank]["raised"]
        for name, table in (("ag_poison", ["all_gather_into_tensor", I64, 2 * K, 2 * K * world]),
                            ("a2a_poison", table_line(world)), ("rs_poison", table_line(world)),
                            ("ar_poison", table_line(world)), ("rs_numel", table_line(world))):
            assert raised[name].startswith("RuntimeError"), (rank, name, raised[name])
            assert [line[0] for line in logs[name]] == ["compress", "all_gather_into_tensor"], (rank, name)
            assert logs[name][1] == table, (rank, name)


def test_argument_errors_come_before_any_call(ranks):
    world, got = ranks
    for rank in range(world):
        for name, text in (("a2a_count", "one tensor per destination rank"),
                           ("rs_count", "one tensor per destination rank"),  # though its acc_dtype is wrong too
                           ("rs_acc", "does not go with"), ("ar_acc", "does not go with")):
            raised = got[rank]["raised"][name]
            assert raised.startswith("ValueError") and text in raised, (rank, name, raised)
            assert got[rank]["logs"][name] == [], (rank, name)
