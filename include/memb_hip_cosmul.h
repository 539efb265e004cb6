/*
 * memb_hip_cosmul.h -- 3CosMul, the multiplicative objective of Levy & Goldberg for king - man + woman (gensim's
 * most_similar_cosmul): one score per candidate from the cosines of a question's terms, and the k best candidates of
 * every question without the score matrix in device memory (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of the headers beneath it, which are left as they are and are named here by their subject only, since
 * their own tests keep their names out of every other header: the matrix header (memb_hip_query_matrix.h, included for
 * the context type: every query against one shared list of candidates), the selection header (the k best columns of every
 * row of a matrix) and the header of the selection with a list of non-candidates per row, whose contract the fused call
 * below follows.
 *
 * THE CONTRACT. A question q has P_q >= 0 positive and N_q >= 0 negative terms, P_q + N_q <= MEMB_HIP_COSMUL_MAX_TERMS.
 * For a candidate whose float32 cosines against those terms are c[0 .. P_q + N_q), positives first and each group in the
 * order given:
 *     s(x)  = (1.0f + x) * 0.5f                          one rounded add, then one rounded multiply
 *     num   = 1.0f;  for each positive term in order:   num = num * s(c)
 *     den   = 1.0f;  for each negative term in order:   den = den * s(c)
 *     score = num / (den + 1e-6f)                        a rounded add, then a correctly rounded divide
 * every operation one IEEE float32 operation, never a fused multiply-add, 1e-6f being float32(0.000001). This is gensim's
 * prod((1 + cos) / 2 over positive) / (prod((1 + cos) / 2 over negative) + 0.000001). A question without negative terms
 * divides by 1.0f + 1e-6f, one without any term scores 1.0f / (1.0f + 1e-6f) everywhere. NaN propagates through the
 * operations. The cosines are taken as they are, unclamped: one just above 1 or below -1 gives what the operations give.
 * The bits depend on the inputs alone: never on the launch, the slices or the workspace.
 *
 * Not built: several models at once (ReadersUnion), sharded readers (ShardedReader), bf16 / fp16, k > 64, more than 64
 * terms per question, weights on the terms (3CosMul has none), scoring fused into the selection kernel, and pooled-bag
 * candidates.
 */
#ifndef MEMB_HIP_COSMUL_H
#define MEMB_HIP_COSMUL_H

#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MEMB_HIP_COSMUL_MAX_TERMS 64

/*
 * The scores of the contract over ANY dense fp32 device matrix of cosines, independent of a model: cosines[t * ld + c] for
 * n_terms rows and n columns, one row per term and one column per candidate. `offsets` are n_questions + 1 uint32 on the
 * device, non-decreasing: the terms of question q are the rows offsets[q] .. offsets[q + 1], the positive ones first;
 * `negatives_from` are n_questions uint32 on the device with offsets[q] <= negatives_from[q] <= offsets[q + 1], the row
 * from which on question q's terms are negative. The caller guarantees that they stay inside the matrix and that no
 * question has more than MEMB_HIP_COSMUL_MAX_TERMS terms. scores[q * ld_scores + c] for c < n is written, nothing outside
 * those columns. One kernel (cosmul_scores), one thread per (question, column); enqueued on `stream`, nothing allocated,
 * nothing synchronised.
 *
 * n_questions == 0 or n == 0 is a no-op. MEMB_HIP_ERR_INVALID with a message and nothing launched: a negative device, null
 * offsets, negatives_from or scores, a null cosines with n > 0, ld < n, ld_scores < n, a pointer not aligned to 4 bytes,
 * n_questions > 2^16 or n > 2^31.
 */
int memb_hip_cosmul_scores_device(int device, const float* cosines, size_t ld, const uint32_t* offsets,
                                  const uint32_t* negatives_from, size_t n_questions, size_t n, float* scores,
                                  size_t ld_scores, void* stream);

/*
 * The k best candidates of every question by the score of the contract, the cosines being those of the matrix header's
 * call of the n_terms term vectors (terms[t * ld_terms .. + dim)) against the candidates rows[0 .. n): bit for bit the
 * selection with a list of non-candidates over the (n_questions, n) score matrix, which is never whole in device memory --
 * (values, positions) in a stable descending order, a greater score first, NaN before every number, equal scores lower
 * position first, positions being indices into `rows`, the positions row q of `excluded` names (width entries,
 * ld_excluded apart, int64 on the device, at most 64; negative or beyond n: ignored; width == 0 accepts null) being no
 * candidates of question q, and empty slots (-inf, -1) behind the candidates there are. values and positions are
 * (n_questions, k) with rows ld_out >= k elements apart, k = 1 .. 64. offsets and negatives_from as above, on the device.
 *
 * For each slice of the candidates: the matrix kernel (query_matrix_trained) over the term vectors into the workspace,
 * cosmul_scores into a second area of it, then the two selection kernels of the list of non-candidates. The workspace
 * holds the selection's lists, then 4 * n_terms * slice bytes, then 4 * n_questions * slice bytes; it is aligned to 8
 * bytes, memb_hip_query_cosmul_workspace_bytes says how large, and its size decides the slicing, never the result.
 * Enqueued on `stream`, nothing allocated, nothing synchronised.
 *
 * n_questions == 0 is a no-op; with n == 0 the merge kernel fills the empty slots, for every model. MEMB_HIP_UNSUPPORTED
 * with nothing launched for the models the matrix header has no fused kernel for (the caller takes the cosine matrix in
 * slices and calls memb_hip_cosmul_scores_device and the dense selection). MEMB_HIP_ERR_INVALID with a message and nothing
 * launched: what the matrix call, the selection and the list of non-candidates refuse (null or misaligned pointers,
 * ld_terms < dim, k outside 1 .. 64, ld_out < k, width > 64, ld_excluded < width, n > 2^36, a workspace too small or not
 * aligned to 8 bytes), null or misaligned offsets or negatives_from, n_terms > 2^16 or n_questions > 2^16.
 */
int memb_hip_query_cosmul_nearest_device(memb_hip_ctx* ctx, const float* terms, size_t n_terms, size_t ld_terms,
                                         const uint32_t* offsets, const uint32_t* negatives_from, size_t n_questions,
                                         const uint32_t* rows, size_t n, uint32_t k, const int64_t* excluded, size_t width,
                                         size_t ld_excluded, float* values, int64_t* positions, size_t ld_out,
                                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * The bytes of workspace memb_hip_query_cosmul_nearest_device needs: the recommended size (slices of about 32 MiB of
 * cosines and scores together), or with `minimal` the least it accepts (slices of 64 candidates). 0 where nothing is
 * needed (n == 0 or n_questions == 0), the sizes are refused or ctx is null.
 */
size_t memb_hip_query_cosmul_workspace_bytes(const memb_hip_ctx* ctx, size_t n_terms, size_t n_questions, size_t n,
                                             uint32_t k, int minimal);

/*
 * The kernel families memb_hip_query_cosmul_nearest_device launches with this context, joined by '+':
 * query_matrix_trained, cosmul_scores and the two selection kernels of the list of non-candidates as their own name
 * function spells them; "" where the call returns MEMB_HIP_UNSUPPORTED. For a null ctx: "cosmul_scores", what
 * memb_hip_cosmul_scores_device launches. Informational.
 */
const char* memb_hip_query_cosmul_kernel_name(const memb_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_COSMUL_H */
