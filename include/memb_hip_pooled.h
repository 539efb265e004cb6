/*
 * memb_hip_pooled.h -- pooled device lookups: the sum or mean of each bag of rows, decoded and reduced by one kernel
 * (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip.h, which it includes and leaves as it is. A batch is rows[0 .. n), the row ids that
 * memb_hip_decode_rows_device takes, cut into bags by offsets[0 .. bags]: bag b owns the entries [begin, end) with
 * begin = min(offsets[b], n) and end = min(offsets[b + 1], n); it is empty when end <= begin. With v_i the fp32 row
 * that memb_hip_decode_rows_device writes for rows[i] (+0.0 for MEMB_HIP_MISSING_ROW and ids >= n_rows):
 *   sum   acc = v_begin, then acc = acc + v_i for i = begin + 1 .. end - 1 in that order, one IEEE fp32 addition each:
 *         nothing fused, nothing reassociated, subnormals kept. An empty bag is +0.0 in every column, a bag of one
 *         entry that row's bits (-0.0 included).
 *   mean  the sum, then ONE correctly rounded fp32 division by (float)(end - begin) -- missing rows count; an empty
 *         bag is +0.0.
 * The result depends on the inputs alone: never on launch geometry or options.
 *
 * A bf16 / fp16 result (memb_hip_pool_rows_device_typed; the MEMB_HIP_OUT_* of memb_hip_narrow.h) is that fp32 value
 * rounded ONCE to the nearest even value of the type, as it is stored: the bits of fp32_result.to(dtype) on the CPU.
 * The additions and the division stay fp32 and only the finished value is narrowed, so a bag of one entry is that
 * row's memb_hip_decode_rows_device_typed bits (-0.0 included), an empty bag is +0.0, fp16 results beyond +-65504 are
 * +-inf and subnormal results stay subnormal.
 */
#ifndef MEMB_HIP_POOLED_H
#define MEMB_HIP_POOLED_H

#include "memb_hip.h"
#include "memb_hip_narrow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MEMB_HIP_POOL_SUM 0
#define MEMB_HIP_POOL_MEAN 1

/*
 * Bag b goes to columns [col_off, col_off + dim) of out + b * ld (ld, col_off in floats); nothing outside those
 * columns is written, and no entry of `rows` outside [0, n) is read whatever `offsets` holds. rows (n entries), offsets
 * (bags + 1 entries) and out are device pointers; out must be 4-byte aligned. Enqueued on `stream`; returns before the
 * kernel ends. bags == 0 is a no-op; n == 0 writes zeros to every bag. A null argument, an unknown mode,
 * ld < col_off + dim or a misaligned out give MEMB_HIP_ERR_INVALID (memb_hip_last_error has the reason) and launch
 * nothing. Trained, uniform and full storages; no accumulate, no weights.
 */
int memb_hip_pool_rows_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags,
                              float* out, size_t ld, size_t col_off, int mode, void* stream);

/*
 * The same with bags' rows of out_type (MEMB_HIP_OUT_F32: the call above and its bits; MEMB_HIP_OUT_BF16 /
 * MEMB_HIP_OUT_F16: one kernel that stores the narrowed rows, no fp32 rows in memory). ld and col_off count ELEMENTS of
 * out_type and out must be aligned to its element (2 bytes for bf16 / fp16). The call allocates nothing and writes no
 * device memory but the bags' columns. An unknown out_type gives MEMB_HIP_ERR_INVALID; the other refusals are those of
 * memb_hip_pool_rows_device.
 */
int memb_hip_pool_rows_device_typed(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags,
                                    void* out, int out_type, size_t ld, size_t col_off, int mode, void* stream);

/*
 * Bytes a pooled lookup has to move, for the host arrays rows[0 .. n) and offsets[0 .. bags]: per entry of a bag the
 * row id (4) and, for a row of the model, what memb_hip_algorithmic_bytes counts as read for it (trained: 4 of
 * metadata + the bitstream; uniform: 12 + dim; full: 4 + 4 dim); per bag two offsets (8) and the 4 dim bytes stored.
 */
int memb_hip_pooled_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                      size_t bags, uint64_t* bytes);

/* The same count for bags' rows of out_type: element_bytes * dim stored per bag (2 dim for bf16 / fp16). */
int memb_hip_pooled_algorithmic_bytes_typed(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                            size_t bags, int out_type, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_POOLED_H */
