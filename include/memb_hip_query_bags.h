/*
 * memb_hip_query_bags.h -- the cosine similarity of every query vector against every pooled BAG of rows, as a matrix or
 * as the k nearest bags of every query, fused with the pooling (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_pooled.h and memb_hip_query_matrix.h, which it includes and leaves as they are; the selection
 * of its second form is the one of the header of the k nearest candidates, which a caller of that form includes beside
 * this one for its limit on k (64) and for the selection over a dense matrix. fp32 only, one model: retrieval over
 * summed or averaged word vectors -- n_queries query vectors against a corpus of `bags` sentences -- without the
 * (bags, dim) matrix of pooled rows in device memory (1.2 GB for a million sentences at dim 300) and, in the nearest-k
 * form, without the (n_queries, bags) matrix either.
 *
 * A corpus is rows[0 .. n) cut by offsets[0 .. bags] into bags, exactly as memb_hip_pool_rows_device cuts it: bag b owns
 * the entries [min(offsets[b], n), min(offsets[b + 1], n)), an empty bag (a non-ascending offset included) is a row of
 * +0.0, and MEMB_HIP_MISSING_ROW and any id >= n_rows are an all +0.0 row that counts.
 *
 * THE CONTRACT adds no arithmetic of its own. x_b is the fp32 row memb_hip_pool_rows_device writes for bag b with the
 * given mode, MEMB_HIP_POOL_SUM or MEMB_HIP_POOL_MEAN: the sequential order of memb_hip_pooled.h, ONE correctly rounded
 * division by the bag's entry count for the mean, +0.0 for an empty bag. cosines[q * ld_out + b] and dots[q * ld_out + b]
 * are the pair contract of memb_hip_pairs.h applied to (queries[q], x_b), word for word -- piece products, lane partials,
 * the butterfly, cos = dot / (max(na, 1e-12f) * max(nb, 1e-12f)), NOT clamped --, and norms[b] is that contract's norm of
 * x_b, bit for bit memb_hip_dense_row_norms_device's. In other words: memb_hip_query_matrix_device's contract with the
 * pooled rows for its candidates. The result depends on the inputs alone: never on launch geometry, on how queries or
 * bags are blocked, on alignment, on slicing or on which kernel ran. No matrix instructions, for the reason
 * memb_hip_query_matrix.h gives: their summation order is not the contract's.
 *
 * By construction the bits equal "pool into an fp32 matrix with memb_hip_pool_rows_device, then
 * memb_hip_dense_pair_similarity_device over (query, pooled row)": that is both the fallback where the fused kernel does
 * not exist and a second oracle where it does.
 *
 * The nearest-k form is the contract of the k nearest candidates over row q of that matrix: a stable descending sort (a
 * greater value first), NaN first, equal values (-0.0 == +0.0) lower bag index first, 1 <= k <= 64, empty slots (from
 * min(k, bags) on) position -1 and value -inf; positions are bag indices. The order is total, so there is ONE answer.
 *
 * Not built: leaving missing entries out of their bags (missing='skip'), the chunked order of memb_hip_pooled_chunked.h
 * for long bags (ONE enormous bag is walked by one wavefront), bf16 / fp16, several models at once (ReadersUnion),
 * sharded readers (ShardedReader), k > 64, bags on the query side inside the kernel (callers pool their queries first,
 * with memb_hip_pool_rows_device).
 */
#ifndef MEMB_HIP_QUERY_BAGS_H
#define MEMB_HIP_QUERY_BAGS_H

#include "memb_hip_pooled.h"
#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cosines[q * ld_out + b] and dots[q * ld_out + b] for q < n_queries and b < bags, norms[b] for b < bags, computed from
 * the compressed rows of the bags: one kernel, no pooled row and no decoded row is written, no atomics, nothing is
 * allocated. queries (n_queries rows of dim floats, ld_queries >= dim floats apart), rows (n ids), offsets (bags + 1
 * entries) and the outputs are device pointers; each output pointer may be null, at least one must not be; ld_out >=
 * bags, in floats (looked at where cosines or dots is given); enqueued on `stream`. bags == 0 or n_queries == 0 is a
 * no-op, for every model; n == 0 writes the results of empty bags. The fused kernel exists for trained models with dim a
 * multiple of 4 and at most 512, whatever the words per wavefront. Anything else returns MEMB_HIP_UNSUPPORTED and launches
 * nothing (memb_hip_last_error says why): the caller pools a slice of the bags and calls
 * memb_hip_dense_pair_similarity_device. A null ctx, null queries (with n_queries > 0), null rows (with n > 0) or offsets
 * (with bags > 0), three null outputs, an unknown mode, ld_queries < dim, ld_out < bags, a pointer that is not aligned to
 * 4 bytes, bags > 2^36, n > 2^37 or n_queries > 2^16 give MEMB_HIP_ERR_INVALID with a message and nothing launched.
 * Nothing outside the named outputs is written -- nothing between the rows of an output with ld_out > bags --, and
 * whatever the offsets hold, no entry outside [0, n) is read.
 */
int memb_hip_query_bags_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                               const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, int mode,
                               float* cosines, float* dots, size_t ld_out, float* norms, void* stream);

/*
 * The kernel family memb_hip_query_bags_device launches with this context: "query_bags_trained", or "" where it returns
 * MEMB_HIP_UNSUPPORTED (and for a null ctx). Informational.
 */
const char* memb_hip_query_bags_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, rows and offsets being HOST arrays: what
 * memb_hip_pooled_algorithmic_bytes counts for the bags WITHOUT the 4 * dim bytes stored per bag, plus
 * memb_hip_query_matrix_algorithmic_bytes's terms: 4 * dim per query, 4 bytes per (query, bag) for each of `cosines` and
 * `dots` that is not 0, 4 bytes per bag where `norms` is not 0.
 */
int memb_hip_query_bags_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                          size_t bags, size_t n_queries, int cosines, int dots, int norms, uint64_t* bytes);

/*
 * The k nearest bags of every query: values[q * ld_out + j] (fp32) and positions[q * ld_out + j] (int64, bag indices) for
 * j < k, the nearest-k contract above over row q of the matrix above. A host loop over slices of the bags, with the
 * offsets pointer advanced per slice: query_bags_trained writes a (n_queries, slice) matrix into the workspace, the
 * library's selection kernels (topk_select, topk_merge) merge it into the outputs. Nothing is allocated and nothing
 * synchronises, so the call can be captured into a HIP graph. The slice is the largest one the given workspace allows --
 * a multiple of 64 bags unless one slice takes them all --, so the workspace decides the slicing and never the result.
 * On the models memb_hip_query_bags_device has its kernel for; any other model returns MEMB_HIP_UNSUPPORTED and launches
 * nothing (the caller takes the matrix slice by slice by other means and runs the dense selection with merge).
 * bags == 0 fills the empty slots, for every model; n_queries == 0 is a no-op. Refused with MEMB_HIP_ERR_INVALID, a
 * message and nothing launched: what memb_hip_query_bags_device refuses, null values or positions, k == 0 or k > 64,
 * ld_out < k, positions or the workspace not aligned to 8 bytes, a workspace smaller than
 * memb_hip_query_bags_topk_workspace_bytes(ctx, n_queries, bags, k, 1). The ld_out - k entries of padding in an output
 * row are never written.
 */
int memb_hip_query_bags_topk_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                                    const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, int mode,
                                    uint32_t k, float* values, int64_t* positions, size_t ld_out, void* workspace,
                                    size_t workspace_bytes, void* stream);

/*
 * The recommended workspace for such a call -- that of the k nearest candidates with bags for candidates: the segment
 * lists of the selection and a (n_queries, slice) matrix of about 32 MiB --, or with minimal != 0 the smallest one the
 * call accepts, slices of 64 bags. 0 for a null ctx, n_queries == 0, bags == 0 or sizes the call refuses.
 */
size_t memb_hip_query_bags_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t bags, uint32_t k,
                                                int minimal);

/*
 * The kernel families memb_hip_query_bags_topk_device launches with this context:
 * "query_bags_trained+topk_select+topk_merge", or "" where it returns MEMB_HIP_UNSUPPORTED (and for a null ctx).
 * Informational.
 */
const char* memb_hip_query_bags_topk_kernel_name(const memb_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_QUERY_BAGS_H */
