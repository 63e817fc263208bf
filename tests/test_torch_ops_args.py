"""torch.ops.dietgpu argument checks that fire before any device is touched
(csrc/torch_ops.cpp), so they run without a GPU: empty lists, CPU tensors,
out-of-range arguments of the size operators, and the row capacity of byte
mode on lists of mixed dtypes.  tests/test_gpu_torch_ops.py holds the
rejections that need device tensors."""
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import codec as C

D = torch.ops.dietgpu
FLOATS = {1: torch.float16, 2: torch.bfloat16, 3: torch.float32, 4: torch.float64}


def cpu(n, dtype=torch.uint8):
    return torch.zeros(n, dtype=dtype)


I32 = torch.int32

EMPTY_LIST = {
    "compress_data-float": lambda: D.compress_data(True, []),
    "compress_data-bytes": lambda: D.compress_data(False, []),
    "compress_data_simple": lambda: D.compress_data_simple(True, []),
    "decompress_data": lambda: D.decompress_data(True, [], []),
    "decompress_data_simple": lambda: D.decompress_data_simple(False, []),
    "decompress_data_split_size": lambda: D.decompress_data_split_size(True, [], cpu(4, torch.float16),
                                                                      torch.tensor([4], dtype=I32)),
    "decompress_data_range": lambda: D.decompress_data_range(True, [], [], torch.zeros(0, dtype=torch.int64)),
    "max_float_compressed_output_size": lambda: D.max_float_compressed_output_size([]),
    "max_any_compressed_output_size": lambda: D.max_any_compressed_output_size([]),
}


@pytest.mark.parametrize("case", EMPTY_LIST)
def test_empty_list_raises(case):
    with pytest.raises(RuntimeError, match="must not be empty|nonzero length"):
        EMPTY_LIST[case]()


CPU_TENSOR = {
    "compress_data-float": lambda: D.compress_data(True, [cpu(16, torch.float16)]),
    "compress_data-bytes": lambda: D.compress_data(False, [cpu(16)]),
    "compress_data_simple": lambda: D.compress_data_simple(False, [cpu(16)]),
    "compress_data_split_size": lambda: D.compress_data_split_size(True, cpu(16, torch.bfloat16),
                                                                  torch.tensor([16], dtype=I32)),
    "decompress_data": lambda: D.decompress_data(True, [cpu(64)], [cpu(16, torch.float16)]),
    "decompress_data_simple": lambda: D.decompress_data_simple(True, [cpu(64)]),
    "decompress_data_split_size": lambda: D.decompress_data_split_size(False, [cpu(64)], cpu(16),
                                                                      torch.tensor([16], dtype=I32)),
    "decompress_data_range": lambda: D.decompress_data_range(False, [cpu(64)], [cpu(16)],
                                                            torch.zeros(1, dtype=torch.int64)),
}


@pytest.mark.parametrize("case", CPU_TENSOR)
def test_cpu_tensor_raises(case):
    with pytest.raises(RuntimeError, match="GPU tensor"):
        CPU_TENSOR[case]()


@pytest.mark.parametrize("size", [-1, -(1 << 40), 1 << 32, 1 << 40])
def test_size_operators_reject_sizes_outside_u32(size):
    with pytest.raises(RuntimeError, match="size out of range"):
        D.max_any_compressed_size(size)
    with pytest.raises(RuntimeError, match="size out of range"):
        D.max_float_compressed_size(cpu(0, torch.bfloat16), size)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool])
def test_float_size_operators_reject_an_integer_dtype(dtype):
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        D.max_float_compressed_size(cpu(0, dtype), 4096)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        D.max_float_compressed_output_size([cpu(4096, dtype)])


SIZES = [0, 1, 7, 4095, 4096, 4097, 12345, 70001]


def test_size_operators_equal_the_codec_bounds():
    for n in SIZES:
        assert D.max_any_compressed_size(n) == C.max_compressed_size(n)
        for ft, dt in FLOATS.items():
            assert D.max_float_compressed_size(cpu(0, dt), n) == C.max_float_compressed_size(ft, n)
    for ft, dt in FLOATS.items():
        ts = [cpu(n, dt) for n in (7, 12345, 4097)]
        assert tuple(D.max_float_compressed_output_size(ts)) == (3, C.max_float_compressed_size(ft, 12345))


# byte mode: (list as (numel, dtype), bytes of the widest member).  The bound
# grows with the number of 4096-byte blocks.  In the first two mixed lists the
# widest member in bytes is neither the first tensor nor the one of the most
# elements: the reference's rule, the largest numel() times the first
# tensor's width, sizes the rows for 1000 and 4097 bytes (one and two blocks
# where two and five are needed); in the third it sizes them for 6392.
ANY_LISTS = {
    "uint8": ([(7, torch.uint8), (4097, torch.uint8), (1, torch.uint8)], 4097),
    "int32": ([(4095, torch.int32), (4096, torch.int32)], 4 * 4096),
    "fp64": ([(12345, torch.float64), (1, torch.float64)], 8 * 12345),
    "mixed-uint8-first": ([(1000, torch.uint8), (1100, torch.int32)], 4400),
    "mixed-three": ([(4097, torch.uint8), (4095, torch.int32), (2500, torch.float64), (0, torch.int32)], 20000),
    "mixed-wide-first": ([(100, torch.float64), (799, torch.uint8)], 800),
}


@pytest.mark.parametrize("case", ANY_LISTS)
def test_max_any_compressed_output_size_takes_the_widest_member_in_bytes(case):
    spec, widest = ANY_LISTS[case]
    ts = [cpu(n, dt) for n, dt in spec]
    assert widest == max(t.numel() * t.element_size() for t in ts)
    by_first_width = max(t.numel() for t in ts) * ts[0].element_size()
    # (the lists of one dtype keep the value they had; the mixed ones tell the two rules apart)
    assert (C.max_compressed_size(by_first_width) != C.max_compressed_size(widest)) == case.startswith("mixed")
    assert tuple(D.max_any_compressed_output_size(ts)) == (len(ts), C.max_compressed_size(widest))
