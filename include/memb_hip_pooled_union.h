/*
 * memb_hip_pooled_union.h -- pooled device lookups of several models at once: the sum or mean of each bag of AVERAGED
 * rows, and the same reduction over a dense fp32 matrix (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_pooled.h, which it includes and leaves as it is. An entry of a batch is one row id per
 * model: entry i is (rows[0][i], .., rows[count - 1][i]). With v_m the fp32 row that memb_hip_decode_rows_device of
 * model m writes for rows[m][i] (+0.0 for MEMB_HIP_MISSING_ROW and ids >= that model's n_rows), its merged row is what
 * memb_hip_decode_rows_union_device with MEMB_HIP_UNION_AVERAGE writes:
 *   u_i = (((v_0 + v_1) + v_2) ..) / (float)count    one IEEE fp32 addition each, one correctly rounded division
 * and the bags are memb_hip_pooled.h's over those rows: bag b owns the entries [min(offsets[b], n), min(offsets[b + 1], n)),
 * acc = u_begin, then acc = acc + u_i in entry order, one correctly rounded division by the entry count for the mean; an
 * empty bag is +0.0, a bag of one entry has u_i's bits, a bf16 / fp16 element is the fp32 value rounded once to nearest
 * even at its store. The result depends on the inputs alone.
 */
#ifndef MEMB_HIP_POOLED_UNION_H
#define MEMB_HIP_POOLED_UNION_H

#include "memb_hip_pooled.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One kernel for `count` models that can share it: neither the models' rows nor the merged rows are written. Bag b goes
 * to columns [col_off, col_off + dim) of out + b * ld (ld, col_off in elements of out_type, a MEMB_HIP_OUT_*). rows[m]
 * (n entries each), offsets (bags + 1 entries) and out are device pointers; ctxs and rows are host arrays of `count`
 * entries. Enqueued on `stream`; bags == 0 is a no-op; n == 0 writes zeros to every bag.
 *
 * The models it takes are those of memb_hip_decode_rows_union_device -- two to four trained models on one device with
 * one dim and one lane geometry, dim a multiple of 4, byte-key tables where the key forms differ, the first context's
 * option union_fused not 0 -- with dim <= 512 and every bag's row aligned to four elements (out, ld and col_off: 16
 * bytes of fp32, 8 of bf16 / fp16). Anything else returns MEMB_HIP_UNSUPPORTED and launches nothing;
 * memb_hip_last_error says which condition it was, and the caller merges the rows itself and pools them with
 * memb_hip_pool_dense_rows_device. A null argument, an unknown mode or out_type, ld < col_off + dim or an out that is
 * not aligned to its element give MEMB_HIP_ERR_INVALID and launch nothing.
 */
int memb_hip_pool_rows_union_device(memb_hip_ctx* const* ctxs, const uint32_t* const* rows, size_t count, size_t n,
                                    const uint32_t* offsets, size_t bags, void* out, int out_type, size_t ld,
                                    size_t col_off, int mode, void* stream);

/*
 * The kernel the last successful memb_hip_pool_rows_union_device with `first` as its first context launched, e.g.
 * "pool_trained_union<false, true, 2, 0>" (<two-level tables, nibble keys, models, out_type>); "" before any. Informational.
 */
const char* memb_hip_pool_union_kernel_name(const memb_hip_ctx* first);

/*
 * The bags of memb_hip_pooled.h over the rows of a dense fp32 matrix on `device`: entry i is values[i * ld_values ..
 * + dim) (ld_values >= dim, in floats), n entries. One wavefront per bag, any dim and alignment of out beyond that of
 * its element; no context is needed. The refusals are memb_hip_pool_rows_device_typed's, and dim == 0 or
 * ld_values < dim.
 */
int memb_hip_pool_dense_rows_device(int device, const float* values, size_t n, size_t dim, size_t ld_values,
                                    const uint32_t* offsets, size_t bags, void* out, int out_type, size_t ld,
                                    size_t col_off, int mode, void* stream);

/* The kernel memb_hip_pool_dense_rows_device launches for out_type, e.g. "pool_dense<0>"; "" for an unknown out_type. */
const char* memb_hip_pool_dense_kernel_name(int out_type);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_POOLED_UNION_H */
