"""CPU tests of the sparse range decode's boundary: the C ABI declares and
exports dietgpu_float_decompress_sparse_range, every host check of
floatDecompressSparseRange fires before any device work (there is no device
here: a check that came late would surface as a HIP error instead), an empty
batch succeeds, and codec.sparse_decompress_range validates its lists before
touching a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dietgpu_float_decompress_sparse_range"
FAKE = 0x7F0000000000  # a 16 B-aligned address that is never dereferenced


@pytest.fixture(scope="module")
def N():
    from dietgpu_fork_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def stack(N):
    # a caller-provided region: creating it makes no HIP call
    return N.Stack(0, FAKE + (1 << 30), 1 << 20)


def call(N, stack, ft=2, pb=10, nb=1, arch=FAKE, out=FAKE + 4096, first=0, count=8):
    rc = N.lib().dietgpu_float_decompress_sparse_range(
        stack.h, ft, pb, nb, N.ptr_array([arch]), N.u32_array([first]), N.u32_array([count]), N.ptr_array([out]),
        None, None, None)
    return rc, N.lib().dietgpu_last_error().decode()


def test_header_declares_and_library_exports(N):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dietgpu_c.h")).read(), flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)", text)
    assert m
    ref = re.search(r"int\s+dietgpu_float_decompress_range\s*\(([^)]*)\)", text)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    assert norm(m.group(1)) == norm(ref.group(1))  # exactly the dense range call's parameters
    assert hasattr(N.lib(), NAME) and NAME in N.EXPORTED
    hooks = open(os.path.join(ROOT, "include", "dietgpu_testhooks.h")).read()
    assert "dietgpu_test_sparse_range_config" in hooks
    N.testlib()
    assert "dietgpu_test_sparse_range_config" in N.TEST_EXPORTED


@pytest.mark.parametrize("kw, msg", [
    (dict(pb=12), "pdf precision"),
    (dict(ft=0), "float_type"),
    (dict(ft=5), "float_type"),
    (dict(arch=FAKE + 8), "16-byte aligned"),
    (dict(ft=2, out=FAKE + 4097), "aligned to its word size"),
    (dict(ft=3, out=FAKE + 4098), "aligned to its word size"),
    (dict(ft=4, out=FAKE + 4100), "aligned to its word size"),
], ids=["pb12", "ft0", "ft5", "archive_align", "out_align_bf16", "out_align_fp32", "out_align_fp64"])
def test_bad_arguments_are_rejected_before_device_work(N, stack, kw, msg):
    rc, err = call(N, stack, **kw)
    assert rc == N.DIETGPU_ERR_INVALID, (rc, err)
    assert msg in err and "HIP error" not in err
    assert stack.max_usage() == 0  # nothing was allocated either


def test_empty_batch_succeeds(N, stack):
    rc = N.lib().dietgpu_float_decompress_sparse_range(stack.h, 2, 10, 0, None, None, None, None, None, None, None)
    assert rc == N.DIETGPU_OK
    assert stack.max_usage() == 0


def test_python_wrapper_validates_before_the_device(N):
    from dietgpu_fork_amd import codec as C

    a = torch.zeros(64, dtype=torch.uint8)
    o = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a, a], [0], [8], [o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [0, 1], [8], [o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [0], [8], [o, o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [1 << 32], [8], [o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [0], [-1], [o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [-1], [8], [o])
    with pytest.raises(ValueError):
        C.sparse_decompress_range([a], [0], [1 << 32], [o])
    with pytest.raises(ValueError):
        C.gather_rows(a, 8, [0], torch.uint8, sparse=True)
    assert ctypes.sizeof(ctypes.c_void_p) == 8
