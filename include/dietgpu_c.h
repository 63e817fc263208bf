/*
 * dietgpu_c.h -- C ABI of the MI355X-native dietgpu codec (libdietgpu_amd.so).
 *
 * The drop-in boundary.  Every entry point is a plain-pointer restatement of
 * one function of the reference's C++ API (NSagan271/dietgpu_fork, paths
 * relative to /root/reference/dietgpu), so an FFI (ctypes, cffi, JNI, cgo)
 * binds it without C++ types:
 *
 *   dietgpu_get_max_compressed_size          ans/GpuANSCodec.h:23   (GpuANSEncode.cu:13)
 *   dietgpu_ans_encode_batch_stride          ans/GpuANSCodec.h:64-98
 *   dietgpu_ans_encode_batch_pointer         ans/GpuANSCodec.h:100-131
 *   dietgpu_ans_encode_batch_split_size      ans/GpuANSCodec.h:133-167
 *   dietgpu_ans_decode_batch_stride          ans/GpuANSCodec.h:173-226
 *   dietgpu_ans_decode_batch_pointer         ans/GpuANSCodec.h:228-262
 *   dietgpu_ans_decode_batch_split_size      ans/GpuANSCodec.h:264-300
 *   dietgpu_ans_get_compressed_info          ans/GpuANSCodec.h:306-322
 *   dietgpu_ans_get_compressed_info_device   ans/GpuANSCodec.h:324-340
 *   dietgpu_get_max_float_compressed_size    float/GpuFloatCodec.h:32
 *   dietgpu_get_max_sparse_float_compressed_size float/GpuFloatCodec.h:33
 *   dietgpu_float_compress                   float/GpuFloatCodec.h:118-158
 *   dietgpu_float_compress_split_size        float/GpuFloatCodec.h:160-187
 *   dietgpu_float_compress_sparse            float/GpuFloatCodec.h:189-203
 *   dietgpu_float_decompress                 float/GpuFloatCodec.h:209-242
 *   dietgpu_float_decompress_split_size      float/GpuFloatCodec.h:244-280
 *   dietgpu_float_decompress_sparse          float/GpuFloatCodec.h:282-293
 *   dietgpu_float_get_compressed_info        float/GpuFloatCodec.h:299-309
 *   dietgpu_float_get_compressed_info_device float/GpuFloatCodec.h:311-321
 *   dietgpu_stack_*                          utils/StackDeviceMemory.h:127-272
 * MI355X extensions (no reference counterpart; zero host->device copies):
 *   dietgpu_float_compress_batch_stride, dietgpu_float_decompress_batch_stride
 *   dietgpu_ans_decode_batch_range, dietgpu_float_decompress_range (words
 *   [first, first + count) of an archive; no checksum flag: a range cannot be
 *   checked against a whole element's checksum)
 *   dietgpu_float_decompress_sparse_range (the same of a sparse archive: a
 *   bitmap rank, then a range decode of the nonzero list's slice)
 *   dietgpu_ans_gather_rows, dietgpu_float_gather_rows (rows of a table held
 *   by one archive, named by indices in device memory; one launch)
 *   dietgpu_float_gather_rows_sum (bags of such rows, each summed in fp32
 *   into one output row: embedding_bag(mode="sum"); one launch)
 *
 * Conventions: `stream` is a hipStream_t (NULL = default stream); the
 * `res` arena is the reference's StackDeviceMemory& first argument; float
 * sizes / capacities are in float words, ANS sizes in bytes, *_size_dev
 * outputs are device arrays of uint32.  ANSCodecConfig / FloatCodecConfig are
 * passed flattened as (prob_bits, use_checksum[, float_type]).  float_type:
 * 1 fp16, 2 bf16, 3 fp32, 4 fp64.  Every call returns DIETGPU_OK or an error
 * code; dietgpu_last_error() returns the message (thread-local).  Checksum
 * mismatches on decode return DIETGPU_ERR_CHECKSUM after all outputs are
 * written (the reference returns ANSDecodeStatus / FloatDecompressStatus).
 */
#ifndef DIETGPU_C_H
#define DIETGPU_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIETGPU_OK 0
#define DIETGPU_ERR_INVALID 1
#define DIETGPU_ERR_HIP 2
#define DIETGPU_ERR_CHECKSUM 3

typedef struct dietgpu_stack dietgpu_stack;

const char* dietgpu_last_error(void);
const char* dietgpu_version(void);

/* StackDeviceMemory: ptr == NULL allocates `bytes` (may be 0); otherwise the
 * caller-owned region [ptr, ptr+bytes) is managed without ownership. */
dietgpu_stack* dietgpu_stack_create(int device, void* ptr, size_t bytes);
void dietgpu_stack_destroy(dietgpu_stack* res);
size_t dietgpu_stack_max_usage(const dietgpu_stack* res);
void dietgpu_stack_reset_max_usage(dietgpu_stack* res);
size_t dietgpu_stack_size_total(const dietgpu_stack* res);

uint32_t dietgpu_get_max_compressed_size(uint32_t uncompressed_bytes);
uint32_t dietgpu_get_max_float_compressed_size(int float_type, uint32_t words);
uint32_t dietgpu_get_max_sparse_float_compressed_size(int float_type, uint32_t words);

/* ---- ANS byte codec ---- */
int dietgpu_ans_encode_batch_stride(dietgpu_stack* res, int prob_bits, int use_checksum,
                                    uint32_t num_in_batch, const void* in_dev,
                                    uint32_t in_per_batch_size, uint32_t in_per_batch_stride,
                                    const uint32_t* histogram_dev, void* out_dev,
                                    uint32_t out_per_batch_stride, uint32_t* out_batch_size_dev,
                                    void* stream);
int dietgpu_ans_encode_batch_pointer(dietgpu_stack* res, int prob_bits, int use_checksum,
                                     uint32_t num_in_batch, const void** in,
                                     const uint32_t* in_size, const uint32_t* histogram_dev,
                                     void** out, uint32_t* out_size_dev, void* stream);
int dietgpu_ans_encode_batch_split_size(dietgpu_stack* res, int prob_bits, int use_checksum,
                                        uint32_t num_in_batch, const void* in_dev,
                                        const uint32_t* in_split_sizes,
                                        const uint32_t* histogram_dev, void* out_dev,
                                        uint32_t out_stride, uint32_t* out_size_dev,
                                        void* stream);
int dietgpu_ans_decode_batch_stride(dietgpu_stack* res, int prob_bits, int use_checksum,
                                    uint32_t num_in_batch, const void* in_dev,
                                    uint32_t in_per_batch_stride, void* out_dev,
                                    uint32_t out_per_batch_stride,
                                    uint32_t out_per_batch_capacity, uint8_t* out_success_dev,
                                    uint32_t* out_size_dev, void* stream);
int dietgpu_ans_decode_batch_pointer(dietgpu_stack* res, int prob_bits, int use_checksum,
                                     uint32_t num_in_batch, const void** in, void** out,
                                     const uint32_t* out_capacity, uint8_t* out_success_dev,
                                     uint32_t* out_size_dev, void* stream);
int dietgpu_ans_decode_batch_split_size(dietgpu_stack* res, int prob_bits, int use_checksum,
                                        uint32_t num_in_batch, const void** in, void* out_dev,
                                        const uint32_t* out_split_sizes,
                                        uint8_t* out_success_dev, uint32_t* out_size_dev,
                                        void* stream);
int dietgpu_ans_get_compressed_info(dietgpu_stack* res, const void** in, uint32_t num_in_batch,
                                    uint32_t* out_sizes_dev, uint32_t* out_checksum_dev,
                                    void* stream);
int dietgpu_ans_get_compressed_info_device(dietgpu_stack* res, const void** in_dev,
                                           uint32_t num_in_batch, uint32_t* out_sizes_dev,
                                           uint32_t* out_checksum_dev, void* stream);

/* ---- float codec ---- */
int dietgpu_float_compress(dietgpu_stack* res, int float_type, int prob_bits, int use_checksum,
                           uint32_t num_in_batch, const void** in, const uint32_t* in_size,
                           void** out, uint32_t* out_size_dev, void* stream);
int dietgpu_float_compress_split_size(dietgpu_stack* res, int float_type, int prob_bits,
                                      int use_checksum, uint32_t num_in_batch,
                                      const void* in_dev, const uint32_t* in_split_sizes,
                                      void* out_dev, uint32_t out_stride,
                                      uint32_t* out_size_dev, void* stream);
int dietgpu_float_compress_sparse(dietgpu_stack* res, int float_type, int prob_bits,
                                  int use_checksum, uint32_t num_in_batch, const void** in,
                                  const uint32_t* in_size, void** out, uint32_t* out_size_dev,
                                  void* stream);
int dietgpu_float_decompress(dietgpu_stack* res, int float_type, int prob_bits,
                             int use_checksum, uint32_t num_in_batch, const void** in,
                             void** out, const uint32_t* out_capacity,
                             uint8_t* out_success_dev, uint32_t* out_size_dev, void* stream);
int dietgpu_float_decompress_split_size(dietgpu_stack* res, int float_type, int prob_bits,
                                        int use_checksum, uint32_t num_in_batch,
                                        const void** in, void* out_dev,
                                        const uint32_t* out_split_sizes,
                                        uint8_t* out_success_dev, uint32_t* out_size_dev,
                                        void* stream);
int dietgpu_float_decompress_sparse(dietgpu_stack* res, int float_type, int prob_bits,
                                    int use_checksum, uint32_t num_in_batch, const void** in,
                                    void** out, const uint32_t* out_capacity,
                                    uint8_t* out_success_dev, uint32_t* out_size_dev,
                                    void* stream);
int dietgpu_float_get_compressed_info(dietgpu_stack* res, const void** in,
                                      uint32_t num_in_batch, uint32_t* out_sizes_dev,
                                      uint32_t* out_types_dev, uint32_t* out_checksum_dev,
                                      void* stream);
int dietgpu_float_get_compressed_info_device(dietgpu_stack* res, const void** in_dev,
                                             uint32_t num_in_batch, uint32_t* out_sizes_dev,
                                             uint32_t* out_types_dev,
                                             uint32_t* out_checksum_dev, void* stream);

/* ---- MI355X extensions ---- */
int dietgpu_float_compress_batch_stride(dietgpu_stack* res, int float_type, int prob_bits,
                                        int use_checksum, uint32_t num_in_batch,
                                        const void* in_dev, uint32_t in_per_batch_words,
                                        uint64_t in_per_batch_stride_bytes, void* out_dev,
                                        uint64_t out_per_batch_stride_bytes,
                                        uint32_t* out_size_dev, void* stream);
int dietgpu_float_decompress_batch_stride(dietgpu_stack* res, int float_type, int prob_bits,
                                          int use_checksum, uint32_t num_in_batch,
                                          const void* in_dev, uint64_t in_per_batch_stride_bytes,
                                          void* out_dev, uint64_t out_per_batch_stride_bytes,
                                          uint32_t out_per_batch_capacity_words,
                                          uint8_t* out_success_dev, uint32_t* out_size_dev,
                                          void* stream);

/* Range decode: out[b][j] = word first[b] + j of the element in[b] encodes,
 * 0 <= j < count[b] (bytes for the byte codec, float words for the float
 * codec); nothing else is written.  in / first / count / out are host arrays;
 * an archive may appear in any number of members (a row gather).
 * out_success_dev[b] = 1 iff the archive is valid and the range lies inside
 * the element; out_size_dev[b] = count[b] then, else 0. */
int dietgpu_ans_decode_batch_range(dietgpu_stack* res, int prob_bits, uint32_t num_in_batch,
                                   const void** in, const uint32_t* first, const uint32_t* count,
                                   void** out, uint8_t* out_success_dev, uint32_t* out_size_dev,
                                   void* stream);
int dietgpu_float_decompress_range(dietgpu_stack* res, int float_type, int prob_bits,
                                   uint32_t num_in_batch, const void** in, const uint32_t* first,
                                   const uint32_t* count, void** out, uint8_t* out_success_dev,
                                   uint32_t* out_size_dev, void* stream);
/* ... of sparse float archives (in[b] 16-byte aligned).  out_success_dev[b] =
 * 1 iff the range lies inside in[b]'s element and the dense archive is valid
 * and holds the nonzero list's slice (a dense archive passed in fails).
 * Temporary memory: num_in_batch rows of the largest count + 32 words; a call
 * whose rows do not fit `res` returns an error as a whole. */
int dietgpu_float_decompress_sparse_range(dietgpu_stack* res, int float_type, int prob_bits,
                                          uint32_t num_in_batch, const void** in,
                                          const uint32_t* first, const uint32_t* count, void** out,
                                          uint8_t* out_success_dev, uint32_t* out_size_dev,
                                          void* stream);

/* Decode-and-accumulate: acc[b][i] += word i of the element dense float
 * archive in[b] encodes (floatDecompressAccumulate, GpuFloatCodec.h).
 * dietgpu_float_decompress's arguments without the checksum flag, plus
 * acc_type, the accumulators' float type: float_type itself, or 3 (fp32)
 * when float_type is 1 or 2 (fp16 / bf16).  acc_capacity counts accumulator
 * words.  Accumulators of two members must not overlap (not checked).
 * Archives written with a checksum are accepted; none is verified. */
int dietgpu_float_decompress_accumulate(dietgpu_stack* res, int float_type, int prob_bits,
                                        uint32_t num_in_batch, const void** in, void** acc,
                                        const uint32_t* acc_capacity, int acc_type,
                                        uint8_t* out_success_dev, uint32_t* out_size_dev,
                                        void* stream);

/* Fused multi-archive reduce (floatReduceArchives, GpuFloatCodec.h):
 * out[b][i] = round((..(init[b][i] + x_1[i]) + ..) + x_K[i]), every add in
 * fp32, where x_k is the element dense float archive in[k * num_in_batch + b]
 * encodes (source-major; float_type 1..3, num_sources 1..64).  init may be
 * null (the sum starts as x_1), else init_type is float_type or 3 (fp32);
 * out_type is float_type (rounded once) or 3.  out_capacity counts out words.
 * A member succeeds iff all its archives are valid, hold the same number of
 * words n and out_capacity[b] >= n; a failing member's out and init are left
 * alone.  Archives written with a checksum are accepted; none is verified. */
int dietgpu_float_reduce(dietgpu_stack* res, int float_type, int prob_bits, uint32_t num_in_batch,
                         uint32_t num_sources, const void** in, const void** init, int init_type,
                         void** out, const uint32_t* out_capacity, int out_type,
                         uint8_t* out_success_dev, uint32_t* out_size_dev, void* stream);

/* ... of sparse float archives (floatDecompressSparseAccumulate,
 * GpuFloatCodec.h; in[b] 16-byte aligned): acc[b][i] += word i of the element
 * for every i whose bitmap bit is set, i.e. whose word is not +0.0 bitwise.
 * The other accumulator words are neither read nor written, so an
 * accumulator word of -0.0 (or a signalling NaN) under a zero word keeps its
 * bits, where the dense form's a + (+0.0) would not.  Same arguments;
 * out_success_dev[b] = 1 iff the dense part is valid and acc_capacity[b] >= n,
 * out_size_dev[b] = n always (dietgpu_float_decompress_sparse's status). */
int dietgpu_float_decompress_sparse_accumulate(dietgpu_stack* res, int float_type, int prob_bits,
                                               uint32_t num_in_batch, const void** in, void** acc,
                                               const uint32_t* acc_capacity, int acc_type,
                                               uint8_t* out_success_dev, uint32_t* out_size_dev,
                                               void* stream);

/* Fused reduce of sparse float archives (floatReduceSparseArchives,
 * GpuFloatCodec.h; in[.] 16-byte aligned): dietgpu_float_reduce's arguments.
 * a = float(init[b][i]); for every source k in order whose bitmap bit i is
 * set (its word is not +0.0 bitwise), a = a + float(x_k[i]) in fp32; a clear
 * bit is skipped, never added as +0.0, so an init word of -0.0 under clear
 * bits stays -0.0; out[b][i] = round(a).  init may be null: the sum starts as
 * the decoded word x_1[i] and runs over x_2 .. x_K.  A member succeeds iff
 * all its archives' dense parts are valid, all sparse headers hold the same n
 * and out_capacity[b] >= n; out_size_dev[b] = n of the first source always. */
int dietgpu_float_reduce_sparse(dietgpu_stack* res, int float_type, int prob_bits, uint32_t num_in_batch,
                                uint32_t num_sources, const void** in, const void** init, int init_type,
                                void** out, const uint32_t* out_capacity, int out_type,
                                uint8_t* out_success_dev, uint32_t* out_size_dev, void* stream);
/* The bytes of the stack that such a call takes at most, for capacities of at
 * most max_capacity words (host only; 0 for arguments the call would refuse:
 * see dietgpu_last_error).  The scratch is bounded by the sources of one
 * kernel launch (dietgpu_set_reduce_max_sources), not by num_sources. */
uint64_t dietgpu_float_reduce_sparse_scratch_bytes(int float_type, uint32_t num_in_batch, uint32_t num_sources,
                                                   uint32_t max_capacity);

/* Row gather with device-resident indices (ansGatherRows / floatGatherRows,
 * GpuANSCodec.h): the archive holds a table [R, row_words]; idx_dev holds
 * num_idx row indices in device memory, int32 or (idx_is_64 != 0) int64.
 * out_dev[i * out_row_stride_words + j] = element[idx_dev[i] * row_words + j];
 * nothing else is written.  out_success_dev[i] (optional) = 1 iff the archive
 * is valid and row idx_dev[i] lies inside the element, else 0 and the row is
 * untouched.  One launch, no host synchronisation, no allocation: the call
 * can be captured in a graph.  No checksum flag, as for a range. */
int dietgpu_ans_gather_rows(dietgpu_stack* res, int prob_bits, const void* archive_dev,
                            uint32_t row_words, uint32_t num_idx, const void* idx_dev,
                            int idx_is_64, void* out_dev, uint64_t out_row_stride_words,
                            uint8_t* out_success_dev, void* stream);
int dietgpu_float_gather_rows(dietgpu_stack* res, int float_type, int prob_bits,
                              const void* archive_dev, uint32_t row_words, uint32_t num_idx,
                              const void* idx_dev, int idx_is_64, void* out_dev,
                              uint64_t out_row_stride_words, uint8_t* out_success_dev,
                              void* stream);

/* Pooled row gather (floatGatherRowsSum, GpuFloatCodec.h): bag b =
 * idx_dev[offsets_dev[b] .. offsets_dev[b + 1]) of the [R, row_words] table,
 * num_bags + 1 offsets and num_idx indices in device memory, both int32 or
 * (idx_is_64 != 0) both int64.  out_dev[b * out_row_stride_words + j] = the
 * fp32 sum, in list order and started from the first row, of word j of the
 * bag's rows, rounded once to fp32 (out_is_fp32 != 0; required for float_type
 * 3) or to the archive's 16-bit type; an empty bag gives +0.0.
 * out_success_dev[b] (optional) = 1 iff the archive is valid, the bag's
 * offsets are ordered and inside [0, num_idx] and all its rows lie inside the
 * element; else 0 and the row is untouched.  float_type 1..3.  One launch, no
 * host synchronisation, no allocation.  No checksum flag. */
int dietgpu_float_gather_rows_sum(dietgpu_stack* res, int float_type, int prob_bits,
                                  const void* archive_dev, uint32_t row_words, uint32_t num_bags,
                                  uint32_t num_idx, const void* idx_dev, const void* offsets_dev,
                                  int idx_is_64, void* out_dev, int out_is_fp32,
                                  uint64_t out_row_stride_words, uint8_t* out_success_dev,
                                  void* stream);

/* Kernel timing hook used by bench.py: when enabled, every launch of the
 * named kernel family ("encode", "decode", "decode_range", "decode_accumulate",
 * "decode_gather", "decode_gather_sum", "hist", "coalesce", "sparse",
 * "sparse_accumulate", "sparse_reduce") is bracketed
 * by hipEvents on its own stream; query returns the summed milliseconds and
 * the launch count since the last reset (synchronises the recorded events). */
void dietgpu_profile_enable(int on);
/* record only kernel family `kernel` (NULL or "" = every family) */
void dietgpu_profile_filter(const char* kernel);
int dietgpu_profile_query(const char* kernel, double* total_ms, uint64_t* launches);
void dietgpu_profile_reset(void);

/* ---- compressor error reporting (MI355X extension) ----
 * The single-pass compressor's cross-workgroup waits (team barrier, look-back)
 * are bounded.  A wait that runs out POISONS its element instead of producing
 * a wrong archive: that element's out_size is written as 0 (no valid archive
 * is shorter than 544 bytes) and the device error word counts it.
 * dietgpu_device_error_count synchronises the current device and returns the
 * count since the last reset (reset != 0 clears it). */
uint32_t dietgpu_device_error_count(int reset);
/* Number of single-pass compressor team-barrier fallbacks since the last
 * reset (reset != 0 clears it): a workgroup that waited out the barrier
 * budget (dietgpu_set_barrier_budget) for its team's partial histograms and
 * counted its element from the input instead.  Archives are unchanged; a
 * nonzero count without a competing kernel or a forced budget means a slow
 * hand-off.  Synchronises the current device. */
uint32_t dietgpu_barrier_fallback_count(int reset);
/* Test hook: polls each such wait may make before it gives up (default
 * 1 << 24).  0 makes every wait that would have to wait fail at once, which
 * forces the error path deterministically for elements of more than one
 * team member.  Passed to the kernels as an argument. */
void dietgpu_set_spin_cap(uint32_t polls);
/* Test hook: how long (100 MHz ticks) a single-pass compressor workgroup
 * waits for the other members of its element's team before it counts the
 * element's histogram from the input itself (default 20000 = 200 us).  The
 * fallback keeps the compressor live when other kernels hold CUs; 0 forces
 * it for every team wait (archives are unchanged). */
void dietgpu_set_barrier_budget(uint32_t ticks);
/* Test hook: every k_encode workgroup of the fused three-kernel path waits
 * (63 - g % 64) * ticks (100 MHz) at its start, so the workgroups start
 * publishing in about reverse index order within every 64 (late publication
 * by dispatched lower workgroups; the single-pass k_pcompress carries no
 * hook, see tools/variants.py pskew).  Archives are unchanged; 0 = off. */
void dietgpu_set_dispatch_skew(uint32_t ticks);
/* Test hook: which compressor takes a float / byte batch that both can
 * compress.  0 (default): the size rule (csrc/codec.hip persistentPreferred;
 * INTEGRATION.md, "Which compressor runs"): a batch goes to the three-kernel
 * path when it has at most 256 work items (elements x 8-block items per
 * element) or when it fits one round of teams that cannot be XCD-aligned,
 * and to the single-pass compressor otherwise; byte archives with a
 * checksum always go single-pass (the three-kernel path has no prologue
 * normalisation for them) unless mode 2 is set; 1: the single-pass compressor whenever
 * the batch is eligible (16 B-aligned inputs, elements of at most 1 MiB of
 * symbols, no caller histogram); 2: always the three-kernel path.  Archives
 * are byte-identical whatever the mode; other values mean 0. */
void dietgpu_set_compress_path(int mode);
/* Test / tuning hook: the most sources one launch of the fused reduce's kernel
 * takes; a call with more chains passes through an fp32 partial.  0 (default)
 * and anything above the largest kernel instance (4) mean that instance.
 * The fused sparse reduce's kernel obeys the same cap.  Results are the same
 * bits whatever the value. */
void dietgpu_set_reduce_max_sources(uint32_t sources);

#ifdef __cplusplus
}
#endif

#endif /* DIETGPU_C_H */
