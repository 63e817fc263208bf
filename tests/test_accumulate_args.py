"""Argument checks of decode-and-accumulate that fire before any device is
touched, so they run without a GPU: torch.ops.dietgpu.decompress_data_accumulate
(csrc/torch_ops.cpp), the C ABI's dietgpu_float_decompress_accumulate
(csrc/capi.cpp) and the Python wrappers.  Every rejection is matched to its
message and leaves the caller's tensors as they were.  Also the new
operator's schema, and that the eleven schemas before it are unchanged.
tests/test_gpu_accumulate.py holds the rejections that need device tensors."""
import pytest
import torch

import dietgpu_fork_amd  # noqa: F401  (registers torch.ops.dietgpu)
from dietgpu_fork_amd import _native as N
from dietgpu_fork_amd import ops

D = torch.ops.dietgpu

SCHEMAS = {
    "max_float_compressed_output_size": "dietgpu::max_float_compressed_output_size(Tensor[] ts) -> (int, int)",
    "max_float_compressed_size": "dietgpu::max_float_compressed_size(Tensor dtype, int size) -> int",
    "max_any_compressed_output_size": "dietgpu::max_any_compressed_output_size(Tensor[] ts) -> (int, int)",
    "max_any_compressed_size": "dietgpu::max_any_compressed_size(int bytes) -> int",
    "compress_data": "dietgpu::compress_data(bool compress_as_float, Tensor[] ts_in, bool checksum=False, Tensor? "
                     "temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor, "
                     "Tensor, int)",
    "compress_data_split_size": "dietgpu::compress_data_split_size(bool compress_as_float, Tensor t_in, Tensor "
                                "t_in_split_sizes, bool checksum=False, Tensor? temp_mem=None, Tensor? "
                                "out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor[], Tensor, int)",
    "compress_data_simple": "dietgpu::compress_data_simple(bool compress_as_float, Tensor[] ts_in, bool "
                            "checksum=False, int? temp_mem=67108864) -> Tensor[]",
    "decompress_data": "dietgpu::decompress_data(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, bool "
                       "checksum=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? "
                       "out_decompressed_words=None) -> int",
    "decompress_data_split_size": "dietgpu::decompress_data_split_size(bool compress_as_float, Tensor[] ts_in, "
                                  "Tensor t_out, Tensor t_out_split_sizes, bool checksum=False, Tensor? "
                                  "temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> "
                                  "int",
    "decompress_data_simple": "dietgpu::decompress_data_simple(bool compress_as_float, Tensor[] ts_in, bool "
                              "checksum=False, int? temp_mem=67108864) -> Tensor[]",
    "decompress_data_range": "dietgpu::decompress_data_range(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, "
                             "Tensor t_first, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? "
                             "out_decompressed_words=None) -> int",
}
NEW = ("dietgpu::decompress_data_accumulate(Tensor[] ts_in, Tensor[] ts_acc, Tensor? temp_mem=None, Tensor? "
       "out_status=None, Tensor? out_sizes=None) -> int")


def schema(name):
    return str(getattr(D, name).default._schema)


def test_the_twelfth_operator():
    assert ops.OPS[-1] == "decompress_data_accumulate" and len(ops.OPS) == 12
    assert schema("decompress_data_accumulate") == NEW
    assert ops.decompress_data_accumulate is D.decompress_data_accumulate


@pytest.mark.parametrize("name", SCHEMAS)
def test_the_eleven_schemas_are_unchanged(name):
    assert tuple(SCHEMAS) == ops.OPS[:11]
    assert schema(name) == SCHEMAS[name]


def arch():
    return torch.arange(64, dtype=torch.uint8)


def acc(dtype=torch.float32, n=16):
    return torch.arange(n, dtype=torch.float64).to(dtype)


# name -> (archives, accumulators, message)
OP_REJECTS = {
    "empty": (lambda: ([], []), "same, nonzero length"),
    "more-archives": (lambda: ([arch(), arch()], [acc()]), "same, nonzero length"),
    "more-accumulators": (lambda: ([arch()], [acc(), acc()]), "same, nonzero length"),
    "mixed-accumulator-dtypes": (lambda: ([arch(), arch()], [acc(), acc(torch.bfloat16)]),
                                 r"accumulators \(ts_acc\) must share a dtype"),
    "integer-accumulator": (lambda: ([arch()], [acc(torch.int32)]), "must be float16, bfloat16, float32 or float64"),
    "byte-accumulator": (lambda: ([arch()], [acc(torch.uint8)]), "must be float16, bfloat16, float32 or float64"),
    "cpu-tensors": (lambda: ([arch()], [acc()]), "inputs must be GPU tensors"),
    "cpu-tensors-bf16": (lambda: ([arch()], [acc(torch.bfloat16)]), "inputs must be GPU tensors"),
}


@pytest.mark.parametrize("case", OP_REJECTS)
def test_operator_rejects(case):
    make, msg = OP_REJECTS[case]
    ins, accs = make()
    keep = [t.clone() for t in ins + accs]
    with pytest.raises(RuntimeError, match=msg):
        D.decompress_data_accumulate(ins, accs)
    assert all(torch.equal(a, b) for a, b in zip(ins + accs, keep))


def test_operator_rejects_positional_flags_of_decompress_data():
    """No compress_as_float and no checksum flag: decompress_data's argument
    list does not fit."""
    with pytest.raises(RuntimeError):
        D.decompress_data_accumulate(True, [arch()], [acc()], False)


# (float_type, acc_type) pairs the C ABI refuses; it checks them, and the
# prob bits, before it looks at the stack or any pointer
BAD_PAIRS = [(1, 2), (1, 4), (2, 1), (2, 4), (3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 3), (2, 0), (2, 5), (3, -1)]
GOOD_PAIRS = [(1, 1), (2, 2), (3, 3), (4, 4), (1, 3), (2, 3)]


def capi(ft, pb, acc_type):
    rc = N.lib().dietgpu_float_decompress_accumulate(None, ft, pb, 1, None, None, None, acc_type, None, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


@pytest.mark.parametrize("ft,acc_type", BAD_PAIRS)
def test_c_abi_rejects_a_bad_pair(ft, acc_type):
    rc, msg = capi(ft, 10, acc_type)
    assert rc == N.DIETGPU_ERR_INVALID
    assert f"acc_type {acc_type} does not go with float_type {ft}" in msg


@pytest.mark.parametrize("ft", [0, 5, -1])
def test_c_abi_rejects_a_bad_float_type(ft):
    rc, msg = capi(ft, 10, 3)
    assert rc == N.DIETGPU_ERR_INVALID and "float_type must be 1..4" in msg


@pytest.mark.parametrize("pb", [0, 8, 12])
def test_c_abi_rejects_prob_bits(pb):
    rc, msg = capi(2, pb, 3)
    assert rc == N.DIETGPU_ERR_INVALID and f"unhandled pdf precision {pb}" in msg


@pytest.mark.parametrize("ft,acc_type", GOOD_PAIRS)
def test_c_abi_passes_a_good_pair_on_to_the_next_check(ft, acc_type):
    rc, msg = capi(ft, 10, acc_type)
    assert rc == N.DIETGPU_ERR_INVALID and "null dietgpu_stack" in msg


def test_c_abi_is_declared():
    assert "dietgpu_float_decompress_accumulate" in N.EXPORTED


def test_python_wrapper_rejects_before_the_device():
    from dietgpu_fork_amd import codec as C

    a, f32 = arch(), acc()
    keep = f32.clone()
    with pytest.raises(ValueError, match="one entry per member"):
        C.float_decompress_accumulate([a, a], [f32])
    with pytest.raises(ValueError, match="empty batch"):
        C.float_decompress_accumulate([], [])
    with pytest.raises(ValueError, match="share a dtype"):
        C.float_decompress_accumulate([a, a], [f32, acc(torch.float16)])
    with pytest.raises(ValueError, match="unsupported accumulator dtype"):
        C.float_decompress_accumulate([a], [acc(torch.int32)])
    with pytest.raises(ValueError, match="must be contiguous"):
        C.float_decompress_accumulate([a], [acc(n=32)[::2]])
    for ft, dt in ((3, torch.float16), (4, torch.float32), (1, torch.bfloat16), (2, torch.float64)):
        with pytest.raises(ValueError, match="does not go with"):
            C.float_decompress_accumulate([a], [acc(dt)], ft=ft)
    assert torch.equal(f32, keep)


def test_acc_dtype_rule_of_the_collectives():
    from dietgpu_fork_amd import dist as Dd

    assert Dd._acc_dtype(torch.bfloat16, None) == torch.float32 == Dd._acc_dtype(torch.float16, None)
    assert Dd._acc_dtype(torch.float32, None) == torch.float32 and Dd._acc_dtype(torch.float64, None) == torch.float64
    assert Dd._acc_dtype(torch.bfloat16, torch.bfloat16) == torch.bfloat16
    for dt, ad in ((torch.float32, torch.bfloat16), (torch.float64, torch.float32), (torch.float16, torch.bfloat16)):
        with pytest.raises(ValueError, match="does not go with"):
            Dd._acc_dtype(dt, ad)
