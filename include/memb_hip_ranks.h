/*
 * memb_hip_ranks.h -- where a given candidate stands among all of them: for every row of a matrix of cosines the NUMBER
 * of candidates that come before a mark in the selection's total order, without a list of the best and without the
 * (queries, candidates) matrix in device memory -- gensim's rank(a, b) and len(closer_than(a, b)), the rank of the
 * expected answer of an analogy question, "how many words lie within cosine t" (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of the headers beneath it, which are left as they are and are named here by their subject only, since
 * their own tests keep their names out of every other header: the matrix header (memb_hip_query_matrix.h, included for
 * the context type: every query against one shared list of candidates), the selection header (the k best columns of every
 * row of a matrix, whose order on values this header counts by) and the header of the list of non-candidates per row,
 * whose format and rules the lists below follow.
 *
 * THE CONTRACT. Row q of a float32 matrix has a MARK (t_q, p_q): a float32 threshold and an int64 position, in the space
 * of the positions the selection calls report -- base + column for the dense call, an index into `rows` for the fused one.
 * key(x) is the selection header's order on float32 values: every NaN has the one greatest key, -0.0 has the key of +0.0,
 * a greater number has a greater key. A candidate at position c with value v PRECEDES the mark iff
 *     key(v) > key(t_q),   or   key(v) == key(t_q) and c < p_q.
 * counts[q], an int64, is the number of candidates of row q that precede its mark. The positions row q of the list of
 * non-candidates names are not counted: int64 entries, `width` <= 64 of them per row, rows ld_excluded >= width entries
 * apart, in any order; repeats count once; a negative entry or one beyond the candidates is ignored (-1 pads a row); a
 * null list is accepted with width == 0.
 *
 * What follows from it:
 *   p_q = -1          counts the candidates strictly greater than t_q;
 *   p_q = INT64_MAX   counts the greater-or-equal ones;
 *   p_q the position of a candidate and t_q bit-equal to its value: that candidate's 0-based rank in the stable
 *                     descending sort of its row, the slot it takes in the selection's output (where that is below 64).
 * The mark need not be a candidate, and no position is treated specially: the candidate at p_q is tested like any other
 * (with t_q bit-equal to its value it never precedes itself) and is left out only where the list of non-candidates names it.
 * The count depends on the inputs alone: never on the slices, the blocks or the workspace.
 *
 * Two kernels: rank_count (a block of 256 threads inside one row counts a fixed run of columns and stores ONE partial
 * count to the workspace) and rank_fold (one wavefront per row takes off what the row's non-candidates contributed, adds
 * the row's partials and writes or adds to counts[q]). No atomics.
 *
 * Not built: the list of the preceding candidates themselves (gensim's closer_than as words, beyond 64 of them), several
 * models at once (ReadersUnion), sharded readers (ShardedReader), bf16 / fp16, pooled-bag candidates, and ranks under the
 * 3CosMul score.
 */
#ifndef MEMB_HIP_RANKS_H
#define MEMB_HIP_RANKS_H

#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The counts of the contract over ANY dense fp32 device matrix, independent of a model: matrix[r * ld + c] for n_rows rows
 * and n columns, the candidate of column c having position base + c. `thresholds` are n_rows float32 and `marks` n_rows
 * int64 on the device; `excluded` is the list of non-candidates (int64 positions on the device, width per row, ld_excluded
 * apart). counts[r] for r < n_rows is written; with accumulate != 0 the count is ADDED to what counts[r] holds, so a
 * matrix fed slice after slice (each with its own base), in any order, ends at the count of one call over all of it.
 * The workspace holds one 32-bit partial count per block of rank_count; memb_hip_dense_ranks_workspace_bytes says how
 * large. Enqueued on `stream`, nothing allocated, nothing synchronised.
 *
 * n_rows == 0 is a no-op; n == 0 writes zeros, or leaves counts alone under accumulate. MEMB_HIP_ERR_INVALID with a message
 * and nothing launched: a negative device or base, a null matrix with n > 0, ld < n, null thresholds, marks or counts, a
 * pointer not aligned (matrix and thresholds to 4 bytes, marks, counts, excluded and workspace to 8), width > 64,
 * ld_excluded < width, a null list with width > 0, n_rows > 2^16, n > 2^31, a workspace too small.
 */
int memb_hip_dense_ranks_device(int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base,
                                const float* thresholds, const int64_t* marks, const int64_t* excluded, size_t width,
                                size_t ld_excluded, int accumulate, int64_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream);

/* The bytes of workspace memb_hip_dense_ranks_device needs; 0 where nothing is needed or the sizes are refused. */
size_t memb_hip_dense_ranks_workspace_bytes(size_t n_rows, size_t n);

/*
 * The counts of the contract over the cosines of the matrix header's call of the n_queries query vectors
 * (queries[q * ld_queries .. + dim)) against the candidates rows[0 .. n): bit for bit the dense call over that
 * (n_queries, n) matrix with base 0, which is never whole in device memory. Positions -- of the marks and of the list of
 * non-candidates -- are indices into `rows`. counts[q] for q < n_queries is written.
 *
 * For each slice of the candidates: the matrix kernel (query_matrix_trained) into the workspace, rank_count over the
 * slice, rank_fold into counts (adding from the second slice on). The workspace holds the partial counts of a slice, then
 * 4 * n_queries * slice bytes; it is aligned to 8 bytes, memb_hip_query_ranks_workspace_bytes says how large, and its size
 * decides the slicing, never the result. Enqueued on `stream`, nothing allocated, nothing synchronised.
 *
 * n_queries == 0 is a no-op; with n == 0 rank_fold writes zeros, for every model. MEMB_HIP_UNSUPPORTED with nothing
 * launched for the models the matrix header has no fused kernel for (the caller takes the cosine matrix in slices and
 * calls memb_hip_dense_ranks_device with accumulate). MEMB_HIP_ERR_INVALID with a message and nothing launched: what the
 * matrix call and the list of non-candidates refuse (null or misaligned pointers, ld_queries < dim, width > 64,
 * ld_excluded < width), null or misaligned thresholds, marks or counts (4 / 8 / 8 bytes), n_queries > 2^16, n > 2^36, a
 * workspace too small or not aligned to 8 bytes.
 */
int memb_hip_query_ranks_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                                const uint32_t* rows, size_t n, const float* thresholds, const int64_t* marks,
                                const int64_t* excluded, size_t width, size_t ld_excluded, int64_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * The bytes of workspace memb_hip_query_ranks_device needs: the recommended size (slices of about 32 MiB of cosines), or
 * with `minimal` the least it accepts (slices of 64 candidates). 0 where nothing is needed (n == 0 or n_queries == 0), the
 * sizes are refused or ctx is null.
 */
size_t memb_hip_query_ranks_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, int minimal);

/*
 * The kernel families memb_hip_query_ranks_device launches with this context, joined by '+': query_matrix_trained,
 * rank_count and rank_fold; "" where the call returns MEMB_HIP_UNSUPPORTED. For a null ctx: "rank_count+rank_fold", what
 * memb_hip_dense_ranks_device launches. Informational.
 */
const char* memb_hip_query_ranks_kernel_name(const memb_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_RANKS_H */
