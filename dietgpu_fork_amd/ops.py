"""PyTorch-ROCm operator surface: ``torch.ops.dietgpu.*``.

The operators are native: ``TORCH_LIBRARY(dietgpu)`` in
``csrc/torch_ops.cpp``, built into ``_lib/libdietgpu_torch.so`` and loaded
with ``torch.ops.load_library`` exactly as the reference's harnesses load its
``DietGpu.cpp`` extension.  This module only loads that library and forwards
``ops.<name>(...)`` to ``torch.ops.dietgpu.<name>``.  "ref": one of the
reference's ten operators (dietgpu/DietGpu.cpp:921-978) with its schema,
validation and return values; "ext": not in the reference.

    operator                          from  list        what it does
    max_float_compressed_output_size  ref   OPS         rows and row bytes for a float list
    max_float_compressed_size         ref   OPS         archive bound of `size` words
    max_any_compressed_output_size    ref   OPS         rows and row bytes for a byte list
    max_any_compressed_size           ref   OPS         archive bound of `bytes` bytes
    compress_data                     ref   OPS         a tensor list into archive rows
    compress_data_split_size          ref   OPS         the splits of one tensor
    compress_data_simple              ref   OPS         a tensor list, own scratch, fresh archives
    decompress_data                   ref   OPS         archives into the given tensors
    decompress_data_split_size        ref   OPS         archives into the splits of one tensor
    decompress_data_simple            ref   OPS         archives into fresh tensors
    decompress_data_range             ext   OPS         a word range of each archive
    decompress_data_accumulate        ext   OPS         adds each archive's element to an accumulator
    gather_rows                       ext   MORE_OPS    rows of a table held by one archive, by device indices
    reduce_data                       ext   REDUCE_OPS  sums several archives per member in one kernel
    gather_rows_sum                   ext   POOL_OPS    sums bags of rows of a table held by one archive
"""
import os

import torch

from . import _native as N

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libdietgpu_torch.so")

OPS = (
    "max_float_compressed_output_size",
    "max_float_compressed_size",
    "max_any_compressed_output_size",
    "max_any_compressed_size",
    "compress_data",
    "compress_data_split_size",
    "compress_data_simple",
    "decompress_data",
    "decompress_data_split_size",
    "decompress_data_simple",
    # extension (not in the reference)
    "decompress_data_range",
    "decompress_data_accumulate",
)

# later extensions, kept apart from the twelve above: gather_rows gathers rows
# of a table held by one archive, named by an index tensor on the device
MORE_OPS = ("gather_rows",)

# reduce_data decodes num_sources archives per member and sums them in one
# kernel (the fused reduce of the reducing collectives)
REDUCE_OPS = ("reduce_data",)

# gather_rows_sum sums bags of rows of a table held by one archive in one
# kernel: embedding_bag(mode="sum") on a compressed table
POOL_OPS = ("gather_rows_sum",)

_LOADED = False


def register():
    """Load the native operator library (idempotent); fails loudly when it or
    the HIP codec library it links is missing."""
    global _LOADED
    if _LOADED:
        return
    N.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"dietgpu_fork_amd: operator library not built ({LIB_PATH}); run "
                          "`python -c 'import __graft_entry__ as g; g.build()'`")
    torch.ops.load_library(LIB_PATH)
    _LOADED = True


def __getattr__(name):
    if name in OPS or name in MORE_OPS or name in REDUCE_OPS or name in POOL_OPS:
        register()
        return getattr(torch.ops.dietgpu, name)
    raise AttributeError(name)
