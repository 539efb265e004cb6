/*
 * memb_hip_within.h -- the candidates that precede a mark, THEMSELVES: for every row of a matrix of cosines the positions
 * (and values) of all candidates that come before a mark in the selection's total order, as one CSR list, without the
 * (queries, candidates) matrix in device memory -- gensim's closer_than(a, b) as words however many they are, "every word
 * within cosine t of these words" (a radius search), neighbour graphs, thresholded retrieval (libmemb_hip.so, MI355X /
 * gfx950).
 *
 * An extension of the headers beneath it, which are left as they are and are named here by their subject only, since
 * their own tests keep their names out of every other header: the matrix header (memb_hip_query_matrix.h, included for
 * the context type: every query against one shared list of candidates), the selection header (the k best columns of every
 * row of a matrix, whose order on values this header lists by), the header of the list of non-candidates per row, whose
 * format and rules the lists below follow, and the count header (per row the NUMBER of candidates that precede a mark),
 * whose predicate this header shares word for word.
 *
 * THE PREDICATE. Row q of a float32 matrix has a MARK (t_q, p_q): a float32 threshold and an int64 position, in the space
 * of the positions the calls report -- base + column for the dense call, an index into `rows` for the fused one. key(x) is
 * the selection header's order on float32 values: every NaN has the one greatest key, -0.0 has the key of +0.0, a greater
 * number has a greater key. A candidate at position c with value v PRECEDES the mark iff
 *     key(v) > key(t_q),   or   key(v) == key(t_q) and c < p_q.
 * The positions row q of the list of non-candidates names are never listed: int64 entries, `width` <= 64 of them per row,
 * rows ld_excluded >= width entries apart, in any order; repeats count once; a negative entry or one beyond the
 * candidates is ignored (-1 pads a row); a null list is accepted with width == 0. So p_q = -1 lists the candidates
 * strictly greater than t_q and p_q = INT64_MAX the greater-or-equal ones.
 *
 * THE OUTPUT, in CSR form.
 *   positions  int64: the position of every candidate of row q that precedes its mark and is no non-candidate,
 *              ASCENDING within a row;
 *   values     float32: the matrix's bits at those positions; the pointer may be null, and then nothing is written;
 *   offsets    int64, n_rows + 1 of them, SUPPLIED by the caller: row q's segment is [offsets[q], offsets[q + 1]);
 *   cursors    int64, n_rows of them: after the call cursors[q] is the number of entries row q FOUND -- by definition
 *              the count header's counts[q], whatever the offsets are.
 * WRITES ARE BOUNDED. An entry is stored only at a destination d with max(offsets[q], 0) <= d < min(offsets[q + 1],
 * capacity), `capacity` being the entries positions (and values) hold. Offsets that are too small lose the entries behind
 * the segment's end, and cursors[q] > offsets[q + 1] - offsets[q] says so; nothing is ever written outside the row's
 * segment or the buffers.
 * ACCUMULATE. With accumulate != 0 row q goes on at offsets[q] + cursors[q] and cursors[q] grows by what the call found:
 * a matrix fed slice after slice (each with its own base) in ascending order of the bases ends bit for bit where one call
 * over all of it ends. In any other order the same set lands in each row, in the order it was fed.
 * The result depends on the inputs alone: never on the slices, the blocks or the workspace.
 *
 * Three kernels per call, each block of the first and the last inside one row over a fixed run of 2048 columns:
 * within_count (how many of the run's columns are listed: one 32-bit total per block), within_starts (one wavefront per
 * row: an exclusive scan of the row's totals into each block's absolute int64 start, then the cursor) and within_write
 * (the run again, the same predicate, an ordered compaction by ballots and prefix population counts). No atomics.
 *
 * Not built: several models at once (ReadersUnion), sharded readers (ShardedReader), bf16 / fp16, pooled-bag candidates,
 * lists under the 3CosMul score, and output sorted by cosine (a sort of each segment by its values).
 */
#ifndef MEMB_HIP_WITHIN_H
#define MEMB_HIP_WITHIN_H

#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The lists of the contract over ANY dense fp32 device matrix, independent of a model: matrix[r * ld + c] for n_rows rows
 * and n columns, the candidate of column c having position base + c. `thresholds` are n_rows float32 and `marks` n_rows
 * int64 on the device; `excluded` is the list of non-candidates (int64 positions on the device, width per row, ld_excluded
 * apart); offsets (n_rows + 1), cursors (n_rows), positions and values (capacity entries each; values may be null) are on
 * the device too. The workspace holds an int64 start and a 32-bit total per block of within_count;
 * memb_hip_dense_within_workspace_bytes says how large. Enqueued on `stream`, nothing allocated, nothing synchronised.
 *
 * n_rows == 0 is a no-op; n == 0 writes zero cursors, or leaves them alone under accumulate. MEMB_HIP_ERR_INVALID with a
 * message and nothing launched: a negative device or base, a null matrix with n > 0, ld < n, null thresholds, marks,
 * offsets, cursors or positions, a pointer not aligned (matrix, thresholds and values to 4 bytes, marks, offsets, cursors,
 * positions, excluded and workspace to 8), width > 64, ld_excluded < width, a null list with width > 0, n_rows > 2^16,
 * n > 2^31, capacity > 2^62, a workspace too small.
 */
int memb_hip_dense_within_device(int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base,
                                 const float* thresholds, const int64_t* marks, const int64_t* excluded, size_t width,
                                 size_t ld_excluded, int accumulate, const int64_t* offsets, int64_t* cursors,
                                 int64_t* positions, float* values, size_t capacity, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The bytes of workspace memb_hip_dense_within_device needs; 0 where nothing is needed or the sizes are refused. */
size_t memb_hip_dense_within_workspace_bytes(size_t n_rows, size_t n);

/*
 * The lists of the contract over the cosines of the matrix header's call of the n_queries query vectors
 * (queries[q * ld_queries .. + dim)) against the candidates rows[0 .. n): bit for bit the dense call over that
 * (n_queries, n) matrix with base 0, which is never whole in device memory. Positions -- of the marks, of the list of
 * non-candidates and of the output -- are indices into `rows`.
 *
 * For each slice of the candidates, in ascending order: the matrix kernel (query_matrix_trained) into the workspace, then
 * within_count, within_starts and within_write over the slice, accumulating from the second slice on. The workspace holds
 * the starts and totals of a slice, then 4 * n_queries * slice bytes; it is aligned to 8 bytes,
 * memb_hip_query_within_workspace_bytes says how large, and its size decides the slicing, never the result. Enqueued on
 * `stream`, nothing allocated, nothing synchronised.
 *
 * n_queries == 0 is a no-op; with n == 0 within_starts writes zero cursors, for every model. MEMB_HIP_UNSUPPORTED with
 * nothing launched for the models the matrix header has no fused kernel for (the caller takes the cosine matrix in slices
 * and calls memb_hip_dense_within_device with accumulate). MEMB_HIP_ERR_INVALID with a message and nothing launched: what
 * the matrix call and the list of non-candidates refuse (null or misaligned pointers, ld_queries < dim, width > 64,
 * ld_excluded < width), null or misaligned thresholds, marks, offsets, cursors or positions, misaligned values,
 * n_queries > 2^16, n > 2^36, capacity > 2^62, a workspace too small or not aligned to 8 bytes.
 */
int memb_hip_query_within_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                                 const uint32_t* rows, size_t n, const float* thresholds, const int64_t* marks,
                                 const int64_t* excluded, size_t width, size_t ld_excluded, const int64_t* offsets,
                                 int64_t* cursors, int64_t* positions, float* values, size_t capacity, void* workspace,
                                 size_t workspace_bytes, void* stream);

/*
 * The bytes of workspace memb_hip_query_within_device needs: the recommended size (slices of about 32 MiB of cosines), or
 * with `minimal` the least it accepts (slices of 64 candidates). 0 where nothing is needed (n == 0 or n_queries == 0), the
 * sizes are refused or ctx is null.
 */
size_t memb_hip_query_within_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, int minimal);

/*
 * The kernel families memb_hip_query_within_device launches with this context, joined by '+': query_matrix_trained,
 * within_count, within_starts and within_write; "" where the call returns MEMB_HIP_UNSUPPORTED. For a null ctx:
 * "within_count+within_starts+within_write", what memb_hip_dense_within_device launches. Informational.
 */
const char* memb_hip_query_within_kernel_name(const memb_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_WITHIN_H */
