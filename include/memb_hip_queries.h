/*
 * memb_hip_queries.h -- the cosine similarity of query vectors against groups of candidate rows, fused with the decode
 * (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_pairs.h, which it includes and leaves as it is. fp32 only, one model: one vector against a list
 * of candidate rows, what scoring a word against candidates, re-ranking the candidates of a lexical substitution, an
 * analogy (king - man + woman against the vocabulary), the odd word out against a centroid and a sentence vector against
 * candidate words are made of. The query need not be a row of the model.
 *
 * A batch is rows[0 .. n), the candidate row ids, cut by offsets[0 .. groups] into groups exactly as
 * memb_hip_pool_rows_device cuts a batch into bags: group g owns the entries [min(offsets[g], n), min(offsets[g + 1], n)).
 * Query g is the fp32 row queries[g * ld_queries .. + dim) of a device matrix, ld_queries >= dim in floats.
 *
 * THE CONTRACT. For an entry i of group g, x is query g exactly as it lies in memory and y is the fp32 row the plain
 * decode writes for rows[i]; MEMB_HIP_MISSING_ROW and any id >= n_rows are an all +0.0 row. dot, na, nb and cos are the
 * contract of memb_hip_pairs.h applied to x and y, with nothing changed: the piece products, the lane partials that keep
 * the bits of a -0.0 product, the butterfly, the correctly rounded roots and
 *     cos = dot / (max(na, 1e-12f) * max(nb, 1e-12f)), NOT clamped to [-1, 1].
 * cosines[i] = cos, dots[i] = dot, norms[i] = nb: bit for bit what memb_hip_row_norms_device gives for rows[i]. The
 * query's norm na is not an output (an empty group would have nobody to write it): memb_hip_dense_row_norms_device over
 * `queries` gives those bits in one small launch.
 *
 * By construction the bits equal "decode the candidates, put query and row next to each other in an fp32 matrix, call
 * memb_hip_dense_pair_similarity_device": that is both the fallback where the fused kernel does not exist and a second
 * oracle where it does. The result depends on the inputs alone: never on launch geometry, options, alignment, or which
 * kernel ran.
 *
 * OFFSETS. The results are defined for non-decreasing offsets. An entry that lies in no group (before offsets[0] or from
 * offsets[groups] on) is not written. Where the offsets do not ascend, which query an entry is scored against, and
 * whether it is written at all, is unspecified, but nothing outside rows[0 .. n), offsets[0 .. groups] and the `groups`
 * rows of `queries` is read and nothing outside [0, n) of the named outputs is written.
 *
 * Not built: top-k or any selection (callers take torch.topk of the result), many queries against ONE shared candidate
 * list (a (groups, n) matrix), bf16 / fp16, several models at once (ReadersUnion), sharded readers, a fused form for
 * uniform or full models, bags as candidates in the chunked order.
 */
#ifndef MEMB_HIP_QUERIES_H
#define MEMB_HIP_QUERIES_H

#include "memb_hip_pairs.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cosines[i], dots[i] and norms[i] for every entry i < n that lies in a group, computed from the compressed candidate
 * rows: one kernel, a wavefront keeps its current group's query in registers, no row is written, nothing is allocated.
 * queries, rows (n ids), offsets (groups + 1 entries) and the outputs (n floats each) are device pointers; each output
 * pointer may be null, at least one must not be; enqueued on `stream`; n == 0 or groups == 0 is a no-op. The fused kernel
 * exists for trained models with dim a multiple of 4 and at most 512, whatever the words per wavefront. Anything else
 * returns MEMB_HIP_UNSUPPORTED and launches nothing (memb_hip_last_error says why): the caller decodes the candidates and
 * calls memb_hip_dense_pair_similarity_device. A null ctx, null queries or offsets (with groups > 0), null rows (with
 * n > 0), three null outputs, ld_queries < dim, a pointer that is not aligned to 4 bytes, n > 2^36 or groups > 2^32 - 2
 * give MEMB_HIP_ERR_INVALID with a message and nothing launched.
 */
int memb_hip_query_similarity_device(memb_hip_ctx* ctx, const float* queries, size_t groups, size_t ld_queries,
                                     const uint32_t* rows, size_t n, const uint32_t* offsets, float* cosines, float* dots,
                                     float* norms, void* stream);

/*
 * The kernel family memb_hip_query_similarity_device launches with this context: "query_trained", or "" where it returns
 * MEMB_HIP_UNSUPPORTED (and for a null ctx). Informational.
 */
const char* memb_hip_query_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, rows and offsets being HOST arrays: what
 * memb_hip_pooled_algorithmic_bytes counts for the groups as bags without the 4 * dim bytes stored per bag -- 8 bytes of
 * offsets per group, per entry that lies in a group its id and its compressed bytes --, the 4 * dim bytes of the query of
 * every group that is not empty, and per entry that lies in a group 4 bytes for each of `cosines`, `dots` and `norms`
 * that is not 0.
 */
int memb_hip_query_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                     size_t groups, int cosines, int dots, int norms, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_QUERIES_H */
