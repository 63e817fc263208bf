"""Inputs and the model of the fused multi-archive reduce tests
(tests/test_gpu_reduce.py on the GPU, tests/test_reduce_inputs.py on the CPU;
DESIGN.md 5.2g).

The model is torch on the CPU, never the code under test:
a = init.float() (or x_1.float() without an init), a = a + x_k.float() in
source order, then .to(out dtype).  ft: 1 fp16, 2 bf16, 3 fp32.  Seeded,
numpy and torch only (tests/accumulate_cases.py holds the shared pieces)."""
import torch

from tests import accumulate_cases as A

FTS = (1, 2, 3)
# (init form, out form): "none" / "T" (the archives' type) / "f32"
FORMS = [(i, o) for i in ("none", "T", "f32") for o in ("T", "f32")]
# straddles one, two and three passes for any per-launch source limit 2 .. 8
K_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 15, 64)


def form_dtype(ft, form):
    """The torch dtype of an init / out form (None for "none")."""
    return None if form == "none" else (torch.float32 if form == "f32" else A.TORCH_FLOAT[ft])


def model(xs, init=None, out_dtype=torch.float32, order=None, per_add=None):
    """The reduce as the feature defines it.  xs: float CPU tensors of one
    type; order: a permutation of the sources (wrong-kernel models);
    per_add: a 16-bit dtype the running sum is rounded to after every add (the
    accumulator the feature does NOT have)."""
    xs = [xs[i] for i in order] if order is not None else list(xs)
    if init is not None:
        a = init.float()
    else:
        a, xs = xs[0].float(), xs[1:]
    if per_add is not None:
        a = a.to(per_add).float()
    for x in xs:
        a = a + x.float()
        if per_add is not None:
            a = a.to(per_add).float()
    return a.to(out_dtype)


def model_from_zero(xs, out_dtype=torch.float32):
    """A sum that starts from +0.0 instead of the first term (wrong: +0.0 +
    -0.0 is +0.0)."""
    a = torch.zeros_like(xs[0], dtype=torch.float32)
    for x in xs:
        a = a + x.float()
    return a.to(out_dtype)


def sources(ft, K, n, seed=70):
    """K vectors of n random finite values of the type over a wide exponent
    range, both signs (accumulate_cases.random_acc, seeds seed .. seed + K - 1)."""
    return [A.random_acc(ft, 1, n, seed=seed + k) for k in range(K)]


def order_probe(ft):
    """The three-term order probe: init 1.0, then 2^-24, 2^-24, -1.0 and every
    permutation of those three.  (1 + 2^-24) ties to 1, so init-first orders
    lose the small terms that a small-terms-first order keeps.  Returns (init
    fp32 [6], [x_1, x_2, x_3] each [6] of the type): word p holds permutation
    p."""
    import itertools

    vals = (2.0 ** -24, 2.0 ** -24, -1.0)
    perms = list(itertools.permutations(range(3)))
    xs = [torch.tensor([vals[p[k]] for p in perms], dtype=torch.float64).to(A.TORCH_FLOAT[ft]) for k in range(3)]
    return torch.ones(len(perms), dtype=torch.float32), xs


def differing_fraction(a, b):
    """The share of words whose bits differ (NaN-free inputs)."""
    return float((A.bits(a) != A.bits(b)).double().mean())
