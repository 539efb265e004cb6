/*
 * memb_hip_norms.h -- the length of a row, and rows of unit length, fused with the decode (libmemb_hip.so, MI355X /
 * gfx950).
 *
 * An extension of memb_hip.h, which it includes and leaves as it is. fp32 only.
 *
 * THE CONTRACT. For an fp32 row v of dim columns -- the bits memb_hip_decode_rows_device writes; a row that is not in the
 * model (MEMB_HIP_MISSING_ROW, any id >= n_rows) is all +0.0:
 *   piece sums     piece k holds the columns 4k .. 4k + 3, a column >= dim counts as +0.0:
 *                      q_k = ((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3
 *                  every product and every sum ONE IEEE fp32 operation, round to nearest even: nothing is fused,
 *                  subnormals are kept
 *   lane partials  for l = 0 .. 63: p_l = q_l + q_(l + 64) + q_(l + 128) + .. in ascending k, starting from q_l; +0.0
 *                  where l has no piece
 *   butterfly      for the stride s = 1, 2, 4, 8, 16, 32 in that order: p_l = p_l + p_(l xor s), all 64 at once. IEEE
 *                  addition is commutative, so all 64 end with the same bits t
 *   norm           sqrt(t), correctly rounded, a subnormal t included
 *   unit row       u_i = v_i / (norm < 1e-12f ? 1e-12f : norm), one correctly rounded fp32 division per element:
 *                  torch.nn.functional.normalize's definition (eps 1e-12), not its bits. A missing or all-zero row stays
 *                  zeros, signs kept
 * The result depends on the inputs alone: never on launch geometry, alignment, options, or which kernel ran.
 *
 * Not built: bf16 / fp16 unit rows, several models at once (ReadersUnion), sharded readers.
 */
#ifndef MEMB_HIP_NORMS_H
#define MEMB_HIP_NORMS_H

#include "memb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * norms[i] = the norm of row rows[i], i < n, computed from the compressed row: one kernel, no row is written. rows and
 * norms are device pointers; enqueued on `stream`; n == 0 is a no-op. The fused kernel exists for trained models with
 * dim a multiple of 4 and at most 512. Anything else returns MEMB_HIP_UNSUPPORTED and launches nothing
 * (memb_hip_last_error says why): the caller decodes the rows and calls memb_hip_dense_row_norms_device. A null
 * argument or a norms pointer that is not aligned to 4 bytes gives MEMB_HIP_ERR_INVALID.
 */
int memb_hip_row_norms_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* norms, void* stream);

/*
 * Columns [col_off, col_off + dim) of out + i * ld = the unit row of rows[i]; norms_or_null[i] = its norm where the
 * pointer is not null. One kernel where the fused form exists (memb_hip_row_norms_device's models, and every row of
 * out aligned to 16 bytes: out, ld, col_off); otherwise memb_hip_decode_rows_device into `out` followed by the dense
 * kernel in place on those columns -- the same bits, no temporary, no allocation. Nothing outside the named columns and
 * norms is written. A null argument, ld < col_off + dim or a pointer that is not aligned to 4 bytes gives
 * MEMB_HIP_ERR_INVALID and launches nothing.
 */
int memb_hip_decode_unit_rows_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld,
                                     size_t col_off, float* norms_or_null, void* stream);

/*
 * The same over the rows of a dense fp32 matrix on `device`: row i is values[i * ld_values .. + dim) (ld_values >= dim,
 * in floats). One wavefront per row, any dim and any alignment beyond that of a float; no context is needed.
 * memb_hip_dense_unit_rows_device may run in place (out + col_off == values and ld == ld_values); any other overlap of
 * values and out is undefined. The refusals are those above, and dim == 0, dim > 2^32 - 1, ld_values < dim or a
 * negative device.
 */
int memb_hip_dense_row_norms_device(int device, const float* values, size_t n, size_t dim, size_t ld_values, float* norms,
                                    void* stream);
int memb_hip_dense_unit_rows_device(int device, const float* values, size_t n, size_t dim, size_t ld_values, float* out,
                                    size_t ld, size_t col_off, float* norms_or_null, void* stream);

/*
 * The kernel family a call launches: memb_hip_row_norms_device (unit_rows == 0; out, ld and col_off are ignored) or
 * memb_hip_decode_unit_rows_device (unit_rows != 0) with this context and output -- "norms_trained" / "unit_trained"
 * where the fused kernel runs, else "" (the norms: MEMB_HIP_UNSUPPORTED) / "unit_dense" (behind the plain decode). A
 * null ctx names the dense entry points' kernels, "norms_dense" / "unit_dense". Informational.
 */
const char* memb_hip_norms_kernel_name(const memb_hip_ctx* ctx, int unit_rows, const void* out, size_t ld, size_t col_off);

/*
 * The bytes a perfect implementation moves for such a call, rows being a HOST array: per row its id and its compressed
 * bytes (memb_hip_algorithmic_bytes's), 4 bytes of norm where `norms` is not 0 and 4 * dim bytes of unit row where
 * unit_rows is not 0.
 */
int memb_hip_norms_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, int unit_rows, int norms,
                                     uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_NORMS_H */
