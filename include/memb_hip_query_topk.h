/*
 * memb_hip_query_topk.h -- the k nearest candidates of every query, WITHOUT the (n_queries, n) matrix of cosines in
 * device memory (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_query_matrix.h, which it includes and leaves as it is. That header answers "how similar is
 * every query to every candidate" with a matrix of n_queries * n floats -- 562 MB for 64 queries over a 2.2 M-word model
 * -- of which a caller who asks "which words are closest" keeps k per query. Here the matrix exists one slice of the
 * candidates at a time, in a workspace of the caller's, and a selection kernel keeps each query's k best across the
 * slices.
 *
 * THE CONTRACT. For query q, candidates rows[0 .. n) and 1 <= k <= MEMB_HIP_TOPK_MAX_K, take row q of what
 * memb_hip_query_matrix_device writes as `cosines` -- bit for bit, a missing id as cosine +0.0, not clamped -- and order
 * its n positions by a STABLE DESCENDING SORT:
 *   - a greater value comes first;
 *   - NaN counts as greater than every number;
 *   - equal values come lower position first, where -0.0 == +0.0 and all NaNs are equal among themselves.
 * positions[q * ld_out + j] (int64) is the j-th position of that order and values[q * ld_out + j] holds the matrix's
 * bits at that position (the sign of a zero and the payload of a NaN included). For j >= min(k, n): values is -inf and
 * positions is -1. An empty slot is recognised by its POSITION, never by its value: a real -inf entry comes before every
 * empty slot. This is torch.sort(matrix, dim=1, descending=True, stable=True) cut to k columns.
 *
 * The order is total, so there is ONE answer: the result depends on the inputs alone, never on the size of the slices
 * or of the workspace, on how a slice is cut into segments, on launch geometry or on which kernel ran.
 *
 * Not built: selection fused into query_matrix_trained's epilogue (the matrix kernel is launched as it is, and no
 * instruction of it changes), k > 64, several models at once (ReadersUnion), sharded readers, bf16 / fp16, a per-query
 * exclusion list (a caller who must drop an entry asks for k + 1 and drops it).
 */
#ifndef MEMB_HIP_QUERY_TOPK_H
#define MEMB_HIP_QUERY_TOPK_H

#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MEMB_HIP_TOPK_MAX_K 64

/*
 * Selection over ANY dense fp32 device matrix, independent of a model: for each of the n_rows rows matrix[r * ld .. + n)
 * (ld >= n, in floats) the first k columns of the order above, values[r * ld_out + j] and positions[r * ld_out + j] =
 * base + column for j < k (ld_out >= k, in elements of either output). With merge != 0 the k entries that row r of
 * `values` / `positions` ALREADY holds take part as candidates, by their value and position; entries whose position is
 * negative are empty. The caller guarantees that the held positions are distinct and lie outside [base, base + n). A
 * matrix fed slice after slice, in any order of the slices, therefore ends at the same bits as one call over all of it.
 * With merge == 0 the outputs are written only.
 *
 * Two kernels, no atomics, nothing allocated, nothing synchronised; enqueued on `stream`. The ld_out - k entries of
 * padding in an output row are never written. `workspace` is device memory of at least
 * memb_hip_dense_topk_workspace_bytes(n_rows, n, k) bytes, aligned to 8; what it holds before the call does not matter.
 * n == 0 fills the empty slots (merge == 0) or leaves what the outputs hold, in order (merge != 0); n_rows == 0 is a
 * no-op. A null matrix (with n > 0), null values, positions or workspace (where bytes are needed), k == 0 or
 * k > MEMB_HIP_TOPK_MAX_K, ld < n, ld_out < k, a negative base or device, a matrix or `values` not aligned to 4 bytes,
 * `positions` or the workspace not aligned to 8, a workspace that is too small, n > 2^31 or n_rows > 2^24 give
 * MEMB_HIP_ERR_INVALID with a message and nothing launched.
 */
int memb_hip_dense_topk_device(int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base,
                               uint32_t k, int merge, float* values, int64_t* positions, size_t ld_out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* The workspace memb_hip_dense_topk_device needs for such a call; 0 where it refuses the sizes. */
size_t memb_hip_dense_topk_workspace_bytes(size_t n_rows, size_t n, uint32_t k);

/*
 * The contract above for the n_queries fp32 rows of `queries` (ld_queries >= dim floats apart) against the candidates
 * rows[0 .. n), on the models memb_hip_query_matrix_device has its fused kernel for; any other model returns
 * MEMB_HIP_UNSUPPORTED and launches nothing (the caller takes the matrix slice by slice by other means and calls
 * memb_hip_dense_topk_device with merge). positions are indices into `rows`. A host loop over slices of the candidates:
 * the matrix kernel writes a (n_queries, slice) matrix into the workspace, the selection merges it into the outputs.
 * Nothing is allocated and nothing synchronises, so the call can be captured into a HIP graph. The slice is the largest
 * one the given workspace allows -- a multiple of 64 candidates unless one slice takes them all --, so the workspace
 * decides the slicing and never the result.
 *
 * Refused with MEMB_HIP_ERR_INVALID, a message and nothing launched: a null ctx, null queries (with n_queries > 0), null
 * rows (with n > 0), null values or positions, k == 0 or k > MEMB_HIP_TOPK_MAX_K, ld_out < k, ld_queries < dim, queries,
 * rows or values not aligned to 4 bytes, positions or the workspace not aligned to 8, a workspace smaller than
 * memb_hip_query_topk_workspace_bytes(ctx, n_queries, n, k, 1), n > 2^36 or n_queries > 2^16 (the matrix call's own
 * limits). n == 0 fills the empty slots, for every model; n_queries == 0 is a no-op. The ld_out - k entries of padding
 * in an output row are never written.
 */
int memb_hip_query_topk_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                               const uint32_t* rows, size_t n, uint32_t k, float* values, int64_t* positions,
                               size_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The recommended workspace for such a call: the segment lists of the selection and a (n_queries, slice) matrix of about
 * 32 MiB, which the selection reads back from cache; it does not grow with n beyond that slice. With minimal != 0: the
 * smallest workspace the call accepts, slices of 64 candidates. 0 for a null ctx, n_queries == 0, n == 0 (no workspace is
 * needed then, and a null one is accepted) or sizes the call refuses.
 */
size_t memb_hip_query_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, uint32_t k, int minimal);

/*
 * The kernel families memb_hip_query_topk_device launches with this context: "query_matrix_trained+topk_select+topk_merge",
 * or "" where it returns MEMB_HIP_UNSUPPORTED. For a null ctx: "topk_select+topk_merge", what
 * memb_hip_dense_topk_device launches. Informational.
 */
const char* memb_hip_query_topk_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, rows being a HOST array: what
 * memb_hip_query_matrix_algorithmic_bytes counts WITHOUT any matrix -- the candidates' ids and compressed bytes once,
 * 4 * dim per query -- plus 12 * k bytes per query, its values and positions.
 */
int memb_hip_query_topk_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t n_queries,
                                          uint32_t k, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_QUERY_TOPK_H */
