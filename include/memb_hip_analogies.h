/*
 * memb_hip_analogies.h -- what an analogy query needs on top of the k-nearest selection: king - man + woman, or
 * most_similar(positive=[...], negative=[...]) (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of the selection header (the k best columns of every row of a matrix, and the k nearest candidates of every
 * query), which is left as it is and is named here by its subject only: its own test keeps its names out of every other
 * header, so the calls below are spelled ..._excluding_topk_... and this header includes memb_hip_query_matrix.h, the one
 * beneath it, for the context type. A caller includes the selection header beside this one for the workspace functions.
 * Two things:
 *   1. the selection with a PER-ROW EXCLUSION LIST: positions that are no candidates, so that an analogy
 *      drops its own input words without spending ranks of the 64 on them;
 *   2. sums of weighted rows of a dense fp32 matrix in a FIXED ORDER, so that the query built from several unit rows has
 *      the same bits on every path.
 *
 * THE CONTRACT of the selection is the selection header's with one change: the positions named in row r's exclusion list
 * are NOT CANDIDATES. Row r of the matrix with those columns removed is ordered by the same stable descending sort and
 * cut to k; positions are still the original ones. Slots from j = min(k, n - d) on are empty (position -1, value -inf),
 * d being the number of distinct excluded positions inside the candidates. With no exclusions the result is bit for bit
 * what the dense and the fused call of the selection header give. The order is total, so the result depends on the
 * inputs alone: never on the slices, the segments or the workspace.
 *
 * THE EXCLUSION LIST is a dense int64 device matrix, excluded[r * ld_excluded + e] for e < width, with
 * width <= MEMB_HIP_MAX_EXCLUDED and ld_excluded >= width. Its entries live in the space of the output `positions`:
 * base + column for the dense call, the index into `rows` for the fused one. They may come in any order and may repeat.
 * An entry that is negative or outside the candidates is ignored, so -1 is both padding and "not in the model". A fixed
 * width (rather than offsets on the device) lets the host check every size without reading device memory: the calls
 * allocate nothing and synchronise nothing and can be captured into a HIP graph. width == 0 accepts a null list.
 *
 * Not built: 3CosMul scoring, more than 64 exclusions per row, exclusions for the top-k over pooled bags, several models
 * at once (ReadersUnion), sharded readers, bf16 / fp16, k > 64, and a weighted sum fused with the decode (an analogy sums
 * three rows per query and searches millions).
 */
#ifndef MEMB_HIP_ANALOGIES_H
#define MEMB_HIP_ANALOGIES_H

#include "memb_hip_query_matrix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MEMB_HIP_MAX_EXCLUDED 64

/*
 * The selection header's dense call under the contract above: its arguments, its workspace (that header's function for
 * the dense call's workspace bytes, as it is), its limits, its refusals, its n == 0 and n_rows == 0, and `merge` -- the
 * entries the outputs hold take part as they are; the caller guarantees, as there, that they are distinct and outside
 * [base, base + n), and here also that row r's list named them when they were selected, or does not name them now. A
 * matrix fed slice after slice with the same list, in any order of the slices, ends at the bits of one call over all of
 * it.
 * Two kernels: topk_select_excluding, then the selection header's topk_merge unchanged.
 *
 * MEMB_HIP_ERR_INVALID with a message and nothing launched, besides that call's own: width > MEMB_HIP_MAX_EXCLUDED,
 * ld_excluded < width, a null `excluded` with width > 0, an `excluded` not aligned to 8 bytes.
 */
int memb_hip_dense_excluding_topk_device(int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base,
                                         uint32_t k, int merge, const int64_t* excluded, size_t width, size_t ld_excluded,
                                         float* values, int64_t* positions, size_t ld_out, void* workspace,
                                         size_t workspace_bytes, void* stream);

/*
 * The selection header's fused call under the contract above, entries of `excluded` being indices into `rows`: its
 * arguments, its workspace (that header's function for the fused call's workspace bytes, as it is), its limits, its
 * refusals, n == 0, n_queries == 0, and MEMB_HIP_UNSUPPORTED with nothing launched for the models it has no fused kernel
 * for. The same host loop over slices of the candidates with the same matrix kernel; a list may name candidates of any
 * slice. The new refusals are those of memb_hip_dense_excluding_topk_device.
 */
int memb_hip_query_excluding_topk_device(memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries,
                                         const uint32_t* rows, size_t n, uint32_t k, const int64_t* excluded, size_t width,
                                         size_t ld_excluded, float* values, int64_t* positions, size_t ld_out,
                                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * The kernel families memb_hip_query_excluding_topk_device launches with this context:
 * "query_matrix_trained+topk_select_excluding+topk_merge", or "" where it returns MEMB_HIP_UNSUPPORTED. For a null ctx:
 * "topk_select_excluding+topk_merge", what memb_hip_dense_excluding_topk_device launches. Informational.
 */
const char* memb_hip_query_excluding_topk_kernel_name(const memb_hip_ctx* ctx);

/*
 * Sums of weighted rows in a fixed order, over ANY dense fp32 device matrix, independent of a model. For sum q over the
 * entries e = offsets[q] .. offsets[q + 1], in that order, starting from out[q][c] = +0.0:
 *     out[q][c] = out[q][c] + (weights[e] * matrix[e * ld + c])          for c < dim
 * the product and the sum each rounded to float32 -- two IEEE operations, never a fused multiply-add. `offsets` are
 * n_sums + 1 uint32 on the device, non-decreasing, the caller's guarantee that they stay inside the matrix; `weights` is
 * float32 on the device, one per entry, null: all +1. A sum without entries is +0.0. out rows lie ld_out >= dim floats
 * apart and nothing outside their first dim columns is written. One kernel (weighted_rows_sum), one thread per output
 * element; enqueued on `stream`, nothing allocated, nothing synchronised.
 *
 * n_sums == 0 or dim == 0 is a no-op; a null matrix is accepted (no sum has an entry then). MEMB_HIP_ERR_INVALID with a
 * message and nothing launched: a negative device, null offsets or out, ld < dim, ld_out < dim, a pointer not aligned to
 * 4 bytes, n_sums > 2^24 or dim > 2^16.
 */
int memb_hip_weighted_rows_sum_device(int device, const float* matrix, size_t ld, const float* weights,
                                      const uint32_t* offsets, size_t n_sums, size_t dim, float* out, size_t ld_out,
                                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_ANALOGIES_H */
