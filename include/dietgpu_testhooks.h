/*
 * dietgpu_testhooks.h -- test-only entry points (libdietgpu_testhooks.so).
 *
 * Not part of the drop-in boundary (include/dietgpu_c.h) and not linked into
 * the product library libdietgpu_amd.so: the GPU tests load this library
 * beside it.  Return codes as in dietgpu_c.h; dietgpu_test_last_error()
 * holds the message of this thread's last failed call.
 */
#ifndef DIETGPU_TESTHOOKS_H
#define DIETGPU_TESTHOOKS_H

#include <stddef.h>
#include <stdint.h>

#include "dietgpu_c.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* dietgpu_test_last_error(void);
/* Enqueue on `stream` a kernel of `workgroups` 256-thread workgroups that
 * each hold `lds_bytes` of LDS for `micros` microseconds (<= 1 s) and exit:
 * compute units held by another kernel while the compressor runs
 * (tests/test_gpu_progress.py). */
int dietgpu_test_occupy(void* stream, uint32_t micros, uint32_t workgroups, uint32_t lds_bytes);
/* hist_dev[b * 256 + s] = count of byte value s in element b of a stride
 * batch (nb <= 65535 elements of `size` bytes, `stride` bytes apart),
 * computed by the compressor's own histogram kernel (k_hist<0>, chunked as
 * the three-kernel path chunks it).  Replaces the reference's
 * ansHistogramBatch as its ANSStatisticsTest.cu:44-95 calls it
 * (ans/GpuANSStatistics.cuh:113-143). */
int dietgpu_test_histogram(dietgpu_stack* res, uint32_t nb, const void* in_dev, uint32_t size,
                           uint32_t stride, uint32_t* hist_dev, void* stream);

/* magic_dev[q] (q = 0 .. 2048) = the 32-bit division magic of pdf q as the
 * compressors compute it in registers (encMagicReg, csrc/encode.h: v_rcp_f64,
 * two Newton steps, an exact fix-up); q 0 -> 0, q 1 -> 0xffffffff.  Checked
 * against the closed form ceil(2^(32 + ceil(log2 q) - 1) / q) by the GPU tests;
 * the magic replaces the division x / pdf of the reference's encode step
 * (ans/GpuANSEncode.cuh:63-89). */
int dietgpu_test_enc_magic(uint32_t* magic_dev, void* stream);

/* StackDeviceMemory::copyToDevice on its own, the upload every entry point
 * uses for its parameter tables: `bytes` from src_host (pageable) to dst_dev
 * in the order of `stream`.  Up to 64 KiB in whole words the bytes ride in
 * kernel arguments, up to 2 MiB they go through the process-wide pinned
 * staging ring (csrc/staging_plan.h), above that straight to the copy engine.
 * As for the library's own tables, src_host may be reused as soon as the call
 * returns.  tests/test_gpu_uploads.py. */
int dietgpu_test_upload(void* dst_dev, const void* src_host, size_t bytes, void* stream);
/* Waits for every upload still in the staging ring and puts the ring's head
 * at offset 0, so that a test knows where its next uploads land. */
int dietgpu_test_upload_reset(void);

/* Calls the C++ range-decode entry points (floatDecompressRange,
 * ansDecodeBatchRange) for one element with `use_checksum` set in their
 * config (for the float codec: FloatCodecConfig.useChecksum) -- the C ABI's
 * range entry points carry no checksum flag.  Returns what a C-ABI call would:
 * DIETGPU_ERR_INVALID when the config is rejected (before the arguments are
 * looked at), DIETGPU_OK after a decode.  float_type 0 = the byte codec. */
int dietgpu_test_range_config(dietgpu_stack* res, int float_type, int use_checksum, const void* in,
                              uint32_t first, uint32_t count, void* out, uint8_t* out_success_dev,
                              uint32_t* out_size_dev, void* stream);

/* The same for floatDecompressSparseRange (float_type 1..4, `in` a sparse
 * archive). */
int dietgpu_test_sparse_range_config(dietgpu_stack* res, int float_type, int use_checksum, const void* in,
                                     uint32_t first, uint32_t count, void* out, uint8_t* out_success_dev,
                                     uint32_t* out_size_dev, void* stream);

/* Calls floatDecompressSparseAccumulate for one member with `use_checksum`
 * set in its config and any acc_type (FloatType values; the C ABI refuses a
 * bad pair itself and carries no checksum flag).  DIETGPU_ERR_INVALID when the
 * entry point throws, DIETGPU_OK after an accumulate. */
int dietgpu_test_sparse_accumulate_config(dietgpu_stack* res, int float_type, int use_checksum, int acc_type,
                                          const void* in, void* acc, uint32_t acc_capacity,
                                          uint8_t* out_success_dev, uint32_t* out_size_dev, void* stream);

/* Calls floatReduceArchives for one member of num_sources archives `in` with
 * `use_checksum` set in its config (the C ABI carries no checksum flag): no
 * init, an output of float_type.  DIETGPU_ERR_INVALID when the entry point
 * throws, DIETGPU_OK after a reduce. */
int dietgpu_test_reduce_config(dietgpu_stack* res, int float_type, int use_checksum, uint32_t num_sources,
                               const void** in, void* out, uint32_t out_capacity, uint8_t* out_success_dev,
                               uint32_t* out_size_dev, void* stream);

/* Calls floatReduceSparseArchives for one member of num_sources sparse
 * archives `in` with `use_checksum` set in its config and any init / out types
 * (FloatType values; the C ABI refuses bad types itself and carries no
 * checksum flag); init may be null.  DIETGPU_ERR_INVALID when the entry point
 * throws, DIETGPU_OK after a reduce. */
int dietgpu_test_sparse_reduce_config(dietgpu_stack* res, int float_type, int use_checksum, uint32_t num_sources,
                                      const void** in, const void* init, int init_type, void* out,
                                      uint32_t out_capacity, int out_type, uint8_t* out_success_dev,
                                      uint32_t* out_size_dev, void* stream);

/* The same for the row gather's C++ entry points (floatGatherRows,
 * ansGatherRows; float_type 0 = the byte codec): num_idx int64 indices at
 * idx_dev, rows of row_words words at a stride of row_words. */
int dietgpu_test_gather_config(dietgpu_stack* res, int float_type, int use_checksum, const void* in,
                               uint32_t row_words, uint32_t num_idx, const void* idx_dev, void* out,
                               uint8_t* out_success_dev, void* stream);

/* The same for the pooled row gather's C++ entry point (floatGatherRowsSum),
 * whose C ABI carries no checksum flag and refuses float_type 4 itself:
 * num_bags + 1 int64 offsets at offsets_dev, num_idx int64 indices at idx_dev,
 * rows of row_words words (fp32 when out_is_fp32) at a stride of row_words. */
int dietgpu_test_gather_sum_config(dietgpu_stack* res, int float_type, int use_checksum, const void* in,
                                   uint32_t row_words, uint32_t num_bags, uint32_t num_idx, const void* idx_dev,
                                   const void* offsets_dev, void* out, int out_is_fp32, uint8_t* out_success_dev,
                                   void* stream);

/* The compress plan (csrc/compress_plan.h) of a dense compress call with no
 * caller-counted rows: which compressor takes the batch and what it launches.
 * Enumerations as in that header. */
typedef struct dietgpu_test_plan {
  uint32_t single_pass; /* 1: k_pcompress; 0: k_hist -> k_encode */
  uint32_t refused;     /* Refused: why not single-pass (0 when it is) */
  uint32_t team;        /* k_pcompress items of the largest element */
  /* single-pass (zero otherwise) */
  uint32_t too_many_items; /* the call is refused */
  uint32_t rounds, teams_per_round, xcd, grid, max_r, items;
  /* three kernels (zero otherwise) */
  uint32_t chunk_words, chunks, groups;
  uint32_t run_hist;  /* k_hist launches per slice of elements: 0 or 1 */
  uint32_t raw_ck;
  uint32_t hist;      /* HistKernel */
  uint32_t normalise; /* Normalise (kKernel, not zero, when single-pass) */
  uint32_t encode_wgs, encode_runs, coalesce_from_flags;
} dietgpu_test_plan;

/* out = the plan the dense compress driver computes on the current device, in
 * the current dietgpu_set_compress_path mode, for nb >= 1 elements of at most
 * max_size bytes (float_type 0, the byte codec) or words (1..4). */
int dietgpu_test_compress_plan(int float_type, uint32_t nb, uint32_t max_size, int checksum, int user_hist,
                               int aligned16, dietgpu_test_plan* out);

#ifdef __cplusplus
}
#endif

#endif /* DIETGPU_TESTHOOKS_H */
