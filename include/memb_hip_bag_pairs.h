/*
 * memb_hip_bag_pairs.h -- the cosine similarity of pairs of BAGS of rows, fused with the pooling (libmemb_hip.so, MI355X /
 * gfx950).
 *
 * An extension of memb_hip_pooled.h and memb_hip_pairs.h, which it includes and leaves as they are. fp32 only, one model:
 * the cosine of two summed or averaged bags of word vectors, what n_similarity of a word-vector library and the
 * sentence-similarity benchmarks (lists of sentence pairs, one cosine each) are made of.
 *
 * A batch is rows[0 .. n) cut by offsets[0 .. 2 * pairs] into 2 * pairs bags, exactly as memb_hip_pool_rows_device cuts
 * it: bag b owns the entries [min(offsets[b], n), min(offsets[b + 1], n)), an empty bag is a row of +0.0, and
 * MEMB_HIP_MISSING_ROW and any id >= n_rows are an all +0.0 row that counts. Pair j is the bags 2j and 2j + 1.
 *
 * THE CONTRACT. x and y are the fp32 rows memb_hip_pool_rows_device writes for the bags 2j and 2j + 1 with the given
 * mode, MEMB_HIP_POOL_SUM or MEMB_HIP_POOL_MEAN: the sequential order of memb_hip_pooled.h -- acc = v_begin, then
 * acc = acc + v_i one entry after the other --, ONE correctly rounded division by the bag's entry count for the mean, +0.0
 * for an empty bag. dot, na, nb and cos are the contract of memb_hip_pairs.h applied to x and y, word for word:
 *   piece products piece k holds the columns 4k .. 4k + 3: d_k = ((x0 * y0 + x1 * y1) + x2 * y2) + x3 * y3, every product
 *                  and every sum ONE IEEE fp32 operation, round to nearest even: nothing is fused, subnormals are kept
 *   lane partials  for l = 0 .. 63: p_l = d_l + d_(l + 64) in ascending k, starting from d_l; +0.0 where l has no piece. A
 *                  lane that has piece l and no piece l + 64 keeps d_l's BITS (a product can be -0.0), it does not add
 *                  +0.0 to them
 *   butterfly      for the stride s = 1, 2, 4, 8, 16, 32 in that order: p_l = p_l + p_(l xor s), all 64 at once; dot is
 *                  the common result
 *   norms          na, nb: bit for bit what memb_hip_row_norms_device (memb_hip_dense_row_norms_device) gives for the
 *                  pooled rows x and y
 *   cosine         cos = dot / (max(na, 1e-12f) * max(nb, 1e-12f)), max(n, eps) being n < eps ? eps : n: one correctly
 *                  rounded fp32 multiplication, then one correctly rounded fp32 division. NOT clamped to [-1, 1]. A pair
 *                  with an empty, an all-missing or an all-zero bag gives +0.0, or -0.0 where dot is -0.0: whatever IEEE
 *                  gives is the contract
 * The result depends on the inputs alone: never on launch geometry, options, alignment, or which kernel ran.
 *
 * By construction the bits equal "pool into an fp32 matrix with memb_hip_pool_rows_device, then
 * memb_hip_dense_pair_similarity_device over it": that is both the fallback where the fused kernel does not exist and a
 * second oracle where it does.
 *
 * Not built: leaving missing entries out of their bags (missing='skip': for mode = sum a missing row adds +0.0, so
 * skipping it would change at most the sign of a zero; for the mean it changes the count), the chunked order of
 * memb_hip_pooled_chunked.h, bf16 / fp16, several models at once (ReadersUnion), sharded readers, one bag against many
 * or top-k search.
 */
#ifndef MEMB_HIP_BAG_PAIRS_H
#define MEMB_HIP_BAG_PAIRS_H

#include "memb_hip_pooled.h"
#include "memb_hip_pairs.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cosines[j], dots[j], norms[2j] (na) and norms[2j + 1] (nb) for pair j < pairs, computed from the compressed rows of the
 * two bags: one kernel, no row is written, nothing is allocated. rows (n ids), offsets (2 * pairs + 1 entries) and the
 * outputs are device pointers; each output pointer may be null, at least one must not be; enqueued on `stream`;
 * pairs == 0 is a no-op, n == 0 writes the results of empty bags. The fused kernel exists for trained models with dim a
 * multiple of 4 and at most 512, whatever the words per wavefront. Anything else returns MEMB_HIP_UNSUPPORTED and launches
 * nothing (memb_hip_last_error says why): the caller pools the bags and calls memb_hip_dense_pair_similarity_device. A
 * null ctx, null rows (with n > 0) or offsets, three null outputs, an unknown mode, a pointer that is not aligned to 4
 * bytes or pairs > 2^35 give MEMB_HIP_ERR_INVALID with nothing launched. Nothing outside the named outputs is written, and
 * whatever the offsets hold, no entry outside [0, n) is read.
 */
int memb_hip_bag_pair_similarity_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                        size_t pairs, int mode, float* cosines, float* dots, float* norms, void* stream);

/*
 * The kernel family memb_hip_bag_pair_similarity_device launches with this context: "bag_pairs_trained", or "" where it
 * returns MEMB_HIP_UNSUPPORTED (and for a null ctx). Informational.
 */
const char* memb_hip_bag_pairs_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, rows and offsets being HOST arrays: what
 * memb_hip_pooled_algorithmic_bytes counts for the 2 * pairs bags without the 4 * dim bytes stored per bag, and per pair
 * 4 bytes for the cosine where `cosines` is not 0, 4 for the dot where `dots` is not 0 and 8 for the two norms where
 * `norms` is not 0.
 */
int memb_hip_bag_pairs_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                         size_t pairs, int cosines, int dots, int norms, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_BAG_PAIRS_H */
