/*
 * memb_hip_query_matrix.h -- the cosine similarity of MANY query vectors against ONE shared list of candidate rows, a
 * (n_queries, n) matrix, fused with the decode (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_queries.h, which it includes and leaves as it is. fp32 only, one model: a batch of analogy
 * questions against the vocabulary, the nearest neighbours of a few dozen words at once, a word-by-word similarity matrix
 * over a word list, a handful of sentence vectors against the same candidate words. With memb_hip_query_similarity_device
 * the candidate ids are repeated once per query and every compressed row is fetched and decoded n_queries times; here it
 * is fetched and decoded ONCE.
 *
 * Query q is the fp32 row queries[q * ld_queries .. + dim) of a device matrix, ld_queries >= dim in floats; rows[0 .. n)
 * are the candidate row ids, shared by every query.
 *
 * THE CONTRACT is the one of memb_hip_queries.h, word for word: cosines[q * ld_out + i], dots[q * ld_out + i] and norms[i]
 * are bit for bit what memb_hip_query_similarity_device gives for entry i of a single group of all n rows with query q.
 * That includes MEMB_HIP_MISSING_ROW and any id >= n_rows as an all +0.0 row, the lanes without a piece keeping the bits
 * of a -0.0 product, the correctly rounded roots and the quotient
 *     cos = dot / (max(na, 1e-12f) * max(nb, 1e-12f)), NOT clamped to [-1, 1].
 * The result depends on the inputs alone: never on launch geometry, on how the queries are blocked inside the kernel, on
 * alignment, or on which kernel ran. The query norms na are not an output, as in memb_hip_queries.h:
 * memb_hip_dense_row_norms_device over `queries` gives their bits.
 *
 * NO MATRIX INSTRUCTIONS. A (n_queries, n) matrix of dot products looks like a matrix multiply, and MFMA would compute it
 * many times faster. It is not an option under this contract: the matrix instructions add the products of a row in an
 * order of their own (and fused), which is not the contract's piece sums, lane partials and butterfly, so the bits would
 * differ from every other entry point of the family. A caller who wants speed at other bits decodes the candidates
 * (memb_hip_decode_rows_device) and multiplies.
 *
 * By construction the bits also equal "decode the candidates, put query and row next to each other in an fp32 matrix,
 * call memb_hip_dense_pair_similarity_device": the fallback where the fused kernel does not exist.
 *
 * Not built: top-k or any selection (callers take torch.topk of the result), bf16 / fp16, several models at once
 * (ReadersUnion), sharded readers, a fused form for uniform or full models.
 */
#ifndef MEMB_HIP_QUERY_MATRIX_H
#define MEMB_HIP_QUERY_MATRIX_H

#include "memb_hip_queries.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cosines[q * ld_out + i] and dots[q * ld_out + i] for every q < n_queries and i < n, and norms[i] for i < n (the
 * candidate's norm, written once, not per query), computed from the compressed candidate rows: one kernel, every
 * compressed row fetched and decoded once whatever n_queries is, no row written, nothing allocated. queries, rows and the
 * outputs are device pointers; each output pointer may be null, at least one must not be; ld_out is in floats. Nothing
 * else is written: the ld_out - n floats of padding in each output row stay untouched. Enqueued on `stream`; n == 0 or
 * n_queries == 0 is a no-op for every model. The fused kernel exists for trained models with dim a multiple of 4 and at
 * most 512, whatever the words per wavefront. Anything else returns MEMB_HIP_UNSUPPORTED and launches nothing
 * (memb_hip_last_error says why): the caller decodes the candidates and calls memb_hip_dense_pair_similarity_device. A
 * null ctx, null queries (with n_queries > 0), null rows (with n > 0), three null outputs, ld_queries < dim, ld_out < n
 * while cosines or dots is given, a pointer that is not aligned to 4 bytes, n > 2^36 or n_queries > 2^16 give
 * MEMB_HIP_ERR_INVALID with a message and nothing launched.
 */
int memb_hip_query_matrix_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                                 const uint32_t* rows, size_t n, float* cosines, float* dots, size_t ld_out,
                                 float* norms, void* stream);

/*
 * The kernel family memb_hip_query_matrix_device launches with this context: "query_matrix_trained", or "" where it
 * returns MEMB_HIP_UNSUPPORTED (and for a null ctx). Informational.
 */
const char* memb_hip_query_matrix_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, rows being a HOST array: per candidate its id and its
 * compressed bytes, counted ONCE, as memb_hip_pooled_algorithmic_bytes counts an entry; 4 * dim per query; 4 bytes per
 * (query, candidate) for each of `cosines` and `dots` that is not 0; 4 bytes per candidate where `norms` is not 0.
 */
int memb_hip_query_matrix_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t n_queries,
                                            int cosines, int dots, int norms, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_QUERY_MATRIX_H */
