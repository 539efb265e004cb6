/*
 * memb_hip_narrow.h -- device lookups straight into bf16 or fp16 rows (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip.h, which it includes and leaves as it is. Element j of row i is the fp32 value that
 * memb_hip_decode_rows_device writes there, rounded ONCE to the nearest even value of the output type: the same bits as
 * torch.tensor(value).to(torch.bfloat16 / torch.float16) on the CPU. Subnormals stay subnormal, values beyond the fp16
 * range become +-inf, the sign of zero is kept and a NaN stays a NaN (its payload may differ). Missing rows
 * (MEMB_HIP_MISSING_ROW, or ids >= n_rows) are +0.0, as in fp32.
 */
#ifndef MEMB_HIP_NARROW_H
#define MEMB_HIP_NARROW_H

#include "memb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element types of `out` */
#define MEMB_HIP_OUT_F32 0    /* float: the same call and the same bits as memb_hip_decode_rows_device */
#define MEMB_HIP_OUT_BF16 1   /* bfloat16, 2 bytes */
#define MEMB_HIP_OUT_F16 2    /* IEEE half, 2 bytes */

/*
 * memb_hip_decode_rows_device with rows of out_type: row i goes to columns [col_off, col_off + dim) of
 * out + i * ld, where ld and col_off count ELEMENTS of out_type. Nothing outside those columns is written. out must be
 * aligned to its element (2 bytes for bf16 / fp16, 4 for fp32). Enqueued on `stream`; returns before the kernel ends.
 * n == 0 is a no-op. An unknown out_type, a misaligned out, ld < col_off + dim or a null argument give
 * MEMB_HIP_ERR_INVALID and launch nothing. No accumulate or divisor exists for bf16 / fp16: a sum rounded to 8 bits of
 * mantissa after every reader is not what a caller wants -- accumulate in fp32 (memb_hip_decode_rows_device_ex).
 */
int memb_hip_decode_rows_device_typed(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, void* out, int out_type,
                                      size_t ld, size_t col_off, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_NARROW_H */
