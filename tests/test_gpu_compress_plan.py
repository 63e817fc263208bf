"""The compress drivers (csrc/codec.hip) launch what the compress plan
(csrc/compress_plan.h) names: for shapes that between them
take both compressors and every normalisation route, the plan fetched through
the test hook predicts the launches of each profile family, and the archives
are the oracle's byte for byte.

The routes stated as literals follow from the rule whatever the kernels'
occupancy is (tests/cpp/compress_plan_check.cpp checks that on the host); the
prologue route depends on k_encode's occupancy, so shapes that may take it are
only checked for agreement with the plan."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV, workspace_fixture  # noqa: F401
from tests.util import NP_SIGNED, TORCH_WORD, exp_bytes, float_words, sparsify

pytestmark = pytest.mark.gpu


ws = workspace_fixture(256 << 20)


@pytest.fixture
def profiled(C):
    C.profile_filter(None)
    C.profile(True)
    try:
        yield
    finally:
        C.profile(False)


def _launches(C):
    return {f: C.profile_query(f)[1] for f in ("compress", "hist", "normalize", "encode", "coalesce")}


def _expected_launches(plan, ft):
    three = not plan["single_pass"]
    return {"compress": int(plan["single_pass"]),
            "hist": plan["run_hist"],
            "normalize": int(three and plan["normalise"] in ("in-reduce", "kernel")),
            "encode": int(three and plan["encode_runs"]),
            "coalesce": int(ft == 4)}


# (id, ft, nb, n, checksum, mode, user_hist, literal expectations of the plan)
CASES = [
    ("bf16-1x1", 2, 1, 1, False, "auto", False, {}),
    ("bf16-1x5000", 2, 1, 5000, False, "auto", False, {}),
    ("bf16-1x2^19", 2, 1, 1 << 19, False, "auto", False, {}),
    ("bf16-8x524288", 2, 8, 524288, False, "auto", False, {"single_pass": 0, "refused": "size-rule"}),
    ("bf16-16x1e6", 2, 16, 1000000, False, "auto", False, {"single_pass": 1, "team": 31}),
    ("bf16-33x1e6", 2, 33, 1000000, False, "auto", False, {"single_pass": 0, "team": 31}),
    ("bytes-ck-1x5000", 0, 1, 5000, True, "auto", False, {"single_pass": 1}),
    ("bytes-ck-1x100000-three", 0, 1, 100000, True, "three-kernel", False,
     {"single_pass": 0, "refused": "forced", "chunks": 25, "hist": "checksum", "normalise": "in-hist"}),
    ("bytes-ck-1x2^20-three", 0, 1, 1 << 20, True, "three-kernel", False,
     {"single_pass": 0, "chunks": 256, "hist": "checksum", "normalise": "in-reduce"}),
    ("bytes-userhist-4x65536", 0, 4, 65536, False, "auto", True,
     {"single_pass": 0, "refused": "user-hist", "run_hist": 0, "normalise": "kernel"}),
    ("fp64-1x300000", 4, 1, 300000, False, "auto", False, {"single_pass": 0, "refused": "two-segments"}),
]


@pytest.mark.parametrize("name,ft,nb,n,checksum,mode,user_hist,literal", CASES, ids=[c[0] for c in CASES])
def test_drivers_launch_what_the_plan_names(C, ws, profiled, name, ft, nb, n, checksum, mode, user_hist, literal):
    # three contents, cycled over the batch: the oracle encodes each once
    if ft == 0:
        contents = [exp_bytes(n, lam=[10.0, 40.0, 100.0][k], seed=30 + k) for k in range(min(nb, 3))]
        refs = [O.ans_encode(w, 10, checksum) for w in contents]
    else:
        contents = [float_words(ft, n, seed=40 + k) for k in range(min(nb, 3))]
        refs = [O.float_compress(w, ft, 10, checksum) for w in contents]
    host = np.stack([contents[i % len(contents)] for i in range(nb)])
    # rows a multiple of 16 bytes apart: the single-pass compressor takes nothing else
    rows = torch.zeros([nb, (n + 15) // 16 * 16], dtype=TORCH_WORD[ft], device=DEV)
    x = rows[:, :n]
    x.copy_(torch.from_numpy(host.view(NP_SIGNED[ft])))
    hist = None
    if user_hist:
        hist = torch.from_numpy(np.stack([O.histogram(host[i]) for i in range(nb)]).astype(np.int32)).to(DEV)
    # as the stride entry points derive it
    aligned16 = x.data_ptr() % 16 == 0 and (x.stride(0) * x.element_size()) % 16 == 0

    with C.compress_path(mode):
        plan = C.test_compress_plan(ft, nb, n, checksum, user_hist, aligned16)
        C.profile_reset()
        if ft == 0:
            out, sizes = C.ans_encode_stride(x, prob_bits=10, checksum=checksum, ws=ws, histogram=hist)
        else:
            out, sizes = C.float_compress_stride(x, ft=ft, prob_bits=10, checksum=checksum, ws=ws)
        torch.cuda.synchronize()
    print(name, plan)
    for key, want in literal.items():
        assert plan[key] == want, (key, plan)
    assert not plan["too_many_items"]
    assert _launches(C) == _expected_launches(plan, ft), plan

    sizes = sizes.cpu().tolist()
    out = out.cpu().numpy()
    for i in range(nb):
        ref = refs[i % len(refs)]
        assert sizes[i] == ref.size, (i, sizes[i], ref.size)
        assert np.array_equal(out[i, : ref.size], ref), f"archive {i} differs from the oracle's"


def test_sparse_list_arrives_counted_and_normalised(C, ws, profiled):
    """One sparse element: the sparse compressor counts and normalises the
    nonzero list's histogram itself (the dense plan is not single-pass, so
    nothing else would), and the dense stage goes straight to k_encode."""
    n = 200000
    w = sparsify(float_words(3, n, seed=50), frac_zero=0.9, seed=51)
    t = torch.from_numpy(w.view(np.int32)).to(DEV).view(torch.float32)
    assert not C.test_compress_plan(3, 1, n)["single_pass"]
    C.profile_reset()
    out, sizes = C.sparse_compress([t], ws=ws)
    torch.cuda.synchronize()
    got = _launches(C)
    assert got["hist"] == 0 and got["compress"] == 0, got
    back = torch.empty_like(t)
    ok, sz = C.sparse_decompress([out[0, : int(sizes[0])]], [back], ws=ws)
    assert ok.cpu().tolist() == [1] and sz.cpu().tolist() == [n]
    assert np.array_equal(back.view(torch.int32).cpu().numpy().view(np.uint32), w)
