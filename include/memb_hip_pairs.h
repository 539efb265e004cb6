/*
 * memb_hip_pairs.h -- the cosine similarity of pairs of rows, fused with the decode (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip.h and memb_hip_norms.h, which it includes and leaves as they are. fp32 only, one model, n
 * pairs: what similarity(w1, w2) of a word-vector library and the word-similarity benchmarks (lists of word pairs, one
 * cosine each) are made of.
 *
 * Pair i is the rows a = pairs[2i] and b = pairs[2i + 1] of an interleaved device array of 2n row ids, the ids
 * memb_hip_decode_rows_device takes; MEMB_HIP_MISSING_ROW and any id >= n_rows are an all +0.0 row.
 *
 * THE CONTRACT. x and y are the fp32 rows the plain decode writes for a and b:
 *   piece products piece k holds the columns 4k .. 4k + 3, a column >= dim counts as +0.0:
 *                      d_k = ((x0 * y0 + x1 * y1) + x2 * y2) + x3 * y3
 *                  every product and every sum ONE IEEE fp32 operation, round to nearest even: nothing is fused,
 *                  subnormals are kept
 *   lane partials  those of memb_hip_norms.h: for l = 0 .. 63: p_l = d_l + d_(l + 64) + .. in ascending k, starting from
 *                  d_l; +0.0 where l has no piece. A piece product can be -0.0 (a sum of squares cannot): a lane that has
 *                  piece l and no piece l + 64 keeps d_l's BITS, it does not add +0.0 to them
 *   butterfly      for the stride s = 1, 2, 4, 8, 16, 32 in that order: p_l = p_l + p_(l xor s), all 64 at once; dot is
 *                  the common result
 *   norms          na, nb: the norms of memb_hip_norms.h of x and y, bit for bit what memb_hip_row_norms_device gives
 *   cosine         cos = dot / (max(na, 1e-12f) * max(nb, 1e-12f)), max(n, eps) being n < eps ? eps : n: one correctly
 *                  rounded fp32 multiplication, then one correctly rounded fp32 division. NOT clamped to [-1, 1]:
 *                  cos(x, x) may be 1.0000001. A pair with a missing or an all-zero row gives +0.0, or -0.0 where dot is
 *                  -0.0: whatever IEEE gives is the contract
 * The result depends on the inputs alone: never on launch geometry, options, alignment, or which kernel ran.
 *
 * Not built: several models at once (ReadersUnion), sharded readers, bf16 / fp16 outputs, one row against many or top-k
 * search, bags against bags (n_similarity).
 */
#ifndef MEMB_HIP_PAIRS_H
#define MEMB_HIP_PAIRS_H

#include "memb_hip.h"
#include "memb_hip_norms.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cosines[i], dots[i], norms[2i] (na) and norms[2i + 1] (nb) for pair i < n, computed from the compressed rows: one
 * kernel, no row is written. pairs (2n ids) and the outputs are device pointers; each output pointer may be null, at
 * least one must not be; enqueued on `stream`; n == 0 is a no-op. The fused kernel exists for trained models with dim a
 * multiple of 4 and at most 512 whose wavefronts decode at least two words at a time (memb_hip_ctx_info::lanes_per_word
 * <= 32). Anything else returns MEMB_HIP_UNSUPPORTED and launches nothing (memb_hip_last_error says why): the caller
 * decodes the rows and calls memb_hip_dense_pair_similarity_device. A null ctx, null pairs, three null outputs, a
 * pointer that is not aligned to 4 bytes or n > 2^36 give MEMB_HIP_ERR_INVALID. Nothing outside the named outputs is
 * written.
 */
int memb_hip_pair_similarity_device(memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, float* cosines, float* dots,
                                    float* norms, void* stream);

/*
 * The same over a dense fp32 matrix of 2n rows on `device`: row r is values[r * ld_values .. + dim) (ld_values >= dim, in
 * floats), the rows 2i and 2i + 1 are pair i. One wavefront per pair, any dim and any alignment beyond that of a float;
 * no context is needed. The refusals are those above, and dim == 0, dim > 2^32 - 1, ld_values < dim or a negative
 * device.
 */
int memb_hip_dense_pair_similarity_device(int device, const float* values, size_t n, size_t dim, size_t ld_values,
                                          float* cosines, float* dots, float* norms, void* stream);

/*
 * The kernel family memb_hip_pair_similarity_device launches with this context: "pairs_trained", or "" where it returns
 * MEMB_HIP_UNSUPPORTED. A null ctx names the dense entry point's kernel, "pairs_dense". Informational.
 */
const char* memb_hip_pairs_kernel_name(const memb_hip_ctx* ctx);

/*
 * The bytes a perfect implementation moves for such a call, pairs being a HOST array of 2n ids: per entry its id and its
 * compressed bytes (what memb_hip_algorithmic_bytes counts as read), per pair 4 bytes for the cosine where `cosines` is
 * not 0, 4 for the dot where `dots` is not 0 and 8 for the two norms where `norms` is not 0.
 */
int memb_hip_pairs_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, int cosines, int dots,
                                     int norms, uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_PAIRS_H */
