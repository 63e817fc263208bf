"""Full-size GPU runs of the BASELINE.json configurations the bench quotes:
c3 (1024 x 4 MiB bytes at 4 bit/symbol, ansEncodeBatchStride /
ansDecodeBatchStride) and c5 at G=1 (8192 x 1 MiB bf16, the batch the
multi-GPU bench shards).  Too large for a full oracle comparison in test
time, so each checks the whole-batch roundtrip bit for bit on the device,
the 16 B archive-size contract (GpuANSUtils.cuh:33 kBlockAlignment), and
byte identity with the oracle for sampled elements (first, middle, last)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_harness import C, DEV  # noqa: F401

pytestmark = pytest.mark.gpu


def test_c3_full(C):
    nb, n = 1024, 4 << 20
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(0, 16, (nb, n), generator=g, device=DEV, dtype=torch.uint8)
    ws = C.Workspace(1 << 30)
    arch, sizes = C.ans_encode_stride(x, prob_bits=10, ws=ws)
    s = sizes.cpu().numpy()
    assert (s > 0).all() and (s % 16 == 0).all()
    # 4 bit/symbol: about half the input (per-block states and headers aside)
    assert 0.49 * n < s.mean() < 0.53 * n
    out, ok, osz = C.ans_decode_stride(arch, n, prob_bits=10, ws=ws)
    assert bool((ok == 1).all()) and bool((osz == n).all())
    assert torch.equal(out, x)
    del out
    for i in (0, nb // 2 - 1, nb - 1):
        ref = O.ans_encode(x[i].cpu().numpy(), 10, False)
        assert s[i] == ref.size, i
        np.testing.assert_array_equal(arch[i, : ref.size].cpu().numpy(), ref, err_msg=f"element {i}")


def test_c5_single_gpu(C):
    nb, n = 8192, 524288
    x = torch.empty([nb, n], dtype=torch.bfloat16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    for r in range(0, nb, 512):
        x[r:r + 512] = torch.randn([512, n], generator=g, device=DEV).to(torch.bfloat16)
    ws = C.Workspace(1 << 30)
    arch, sizes = C.float_compress_stride(x, prob_bits=10, ws=ws)
    s = sizes.cpu().numpy()
    assert (s > 0).all() and (s % 16 == 0).all()
    assert C.device_error_count(reset=True) == 0
    out, ok, osz = C.float_decompress_stride(arch, n, torch.bfloat16, prob_bits=10, ws=ws)
    assert bool((ok == 1).all()) and bool((osz == n).all())
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))
    del out
    for i in (0, nb // 2 - 1, nb - 1):
        ref = O.float_compress(x[i].view(torch.int16).cpu().numpy().view(np.uint16), 2)
        assert s[i] == ref.size, i
        np.testing.assert_array_equal(arch[i, : ref.size].cpu().numpy(), ref, err_msg=f"element {i}")


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, 2), (torch.float16, 1), (torch.float32, 3)])
def test_batch1_large_tensor(C, dtype, ft):
    """One 128*512*1024-word tensor (a single element of 64 M words, the
    three-kernel path): bit-exact roundtrip and an archive byte-identical to
    the oracle's."""
    words = 128 * 512 * 1024
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(1, words, generator=g, device=DEV).to(dtype)
    ws = C.Workspace(1 << 30)
    arch, sizes = C.float_compress_stride(x, prob_bits=10, ws=ws)
    s = int(sizes[0])
    iw = torch.int16 if x.element_size() == 2 else torch.int32
    ref = O.float_compress(x[0].view(iw).cpu().numpy().view(np.uint16 if iw == torch.int16 else np.uint32), ft)
    assert s == ref.size and s % 16 == 0
    np.testing.assert_array_equal(arch[0, :s].cpu().numpy(), ref)
    out, ok, osz = C.float_decompress_stride(arch, words, dtype, prob_bits=10, ws=ws)
    assert int(ok[0]) == 1 and int(osz[0]) == words
    assert torch.equal(out.view(iw), x.view(iw))


def test_batch1_1e9_bf16(C):
    """The largest point of the reference's published batch-1 curve
    (README.md:118: 1.07e9 bf16 words): its max-size bound (2.41e9 bytes)
    exceeds INT32_MAX, so every archive offset past 2^31 is exercised.
    Roundtrip bit for bit, the size against the bound, and the float header
    read back from the archive (too large for an oracle run in test time:
    parity unpinned at this size beyond the roundtrip and the header)."""
    n = 1_070_000_000
    x = torch.empty([1, n], dtype=torch.bfloat16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(107)
    flat = x.view(-1)
    for i in range(0, n, 1 << 28):
        m = min(1 << 28, n - i)
        flat[i:i + m] = (torch.randn(m, generator=g, device=DEV).view(torch.int32) >> 16).to(torch.int16).view(
            torch.bfloat16)
    ws = C.Workspace(3 << 30)
    arch, sizes = C.float_compress_stride(x, prob_bits=10, ws=ws)
    s = int(sizes[0])
    assert 0 < s <= arch.shape[1] and s % 16 == 0
    assert arch.shape[1] > (1 << 31)  # offsets beyond INT32_MAX are in play
    assert 0.66 * 2 * n < s < 0.69 * 2 * n
    hdr = arch[0, :32].cpu().numpy().view(np.uint32)
    assert hdr[1] == n and (hdr[2] & 0xf) == 2
    assert C.device_error_count(reset=True) == 0
    out, ok, osz = C.float_decompress_stride(arch, n, torch.bfloat16, prob_bits=10, ws=ws)
    assert bool((ok == 1).all()) and int(osz[0]) == n
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))


def test_fp64_1e8_float_benchmark_point(C):
    """The largest dense point of the fork's own float_benchmark
    (FloatBenchmark.cu:421-427: batch 1 x 1e8 fp64 words, pb 9, floatCompress
    pointer API, N(0,1)): the two-pass fp64 archive is byte-identical to the
    serial oracle's (the whole 1e8-word element, not a sample), its header
    reads back through floatGetCompressedInfo, and the roundtrip is exact."""
    import ctypes

    from dietgpu_fork_amd import _native as N

    n = 100_000_000
    g = torch.Generator(device=DEV).manual_seed(108)
    x = torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    ws = C.Workspace(3 << 30)
    arch, sizes = C.float_compress_pointer([x], prob_bits=9, ws=ws)
    s = int(sizes[0])
    assert 0 < s <= arch.shape[1] and s % 16 == 0
    assert C.device_error_count(reset=True) == 0
    ref = O.float_compress(x.view(torch.int64).cpu().numpy().view(np.uint64), 4, 9)
    assert s == ref.size
    np.testing.assert_array_equal(arch[0, :s].cpu().numpy(), ref)
    del ref
    sz = torch.zeros([1], dtype=torch.int32, device=DEV)
    ty = torch.zeros([1], dtype=torch.int32, device=DEV)
    ck = torch.zeros([1], dtype=torch.int32, device=DEV)
    N.check(N.lib().dietgpu_float_get_compressed_info(ws.h, N.ptr_array([arch[0].data_ptr()]), 1, sz.data_ptr(),
                                                      ty.data_ptr(), ck.data_ptr(),
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert int(sz[0]) == n and int(ty[0]) == 4
    y = torch.empty_like(x)
    ok, osz = C.float_decompress_pointer([arch[0, :s]], [y], prob_bits=9, ws=ws)
    assert int(ok[0]) == 1 and int(osz[0]) == n
    assert torch.equal(y.view(torch.int64), x.view(torch.int64))
