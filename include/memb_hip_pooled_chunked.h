/*
 * memb_hip_pooled_chunked.h -- pooled device lookups under the CHUNKED summation order: a bag is cut into chunks of
 * MEMB_HIP_POOL_CHUNK entries, many wavefronts sum the chunks at once, and the chunks' sums are added in chunk order
 * (libmemb_hip.so, MI355X / gfx950). Long bags -- documents, paragraphs -- at speed, under an order that is fixed by the
 * inputs alone.
 *
 * An extension of memb_hip_pooled_known.h, which it includes and leaves as it is: the batch rows[0 .. n), the bags
 * offsets[0 .. bags], MEMB_HIP_POOL_SUM / MEMB_HIP_POOL_MEAN, the MEMB_HIP_OUT_* element types and what a KNOWN entry is
 * (rows[i] < n_rows) are those headers'. Their calls add a bag's rows one after the other (the SEQUENTIAL order) and stay
 * the right choice for short bags; this one defines a second order next to it.
 *
 * C = MEMB_HIP_POOL_CHUNK: a constant of the API, a power of two and a multiple of 8, independent of the model and of every
 * launch geometry. Bag b owns the entries [begin, end) with begin = min(offsets[b], n) and end = min(offsets[b + 1], n);
 * its chunk j owns the entries [begin + C j, min(end, begin + C (j + 1))).
 *   skip_missing == 0  (an entry that is not in the model is a row of +0.0 that counts)
 *     p_j   the sequential fp32 loop over chunk j: acc = v_first, then acc = acc + v_i in entry order, one IEEE fp32
 *           addition each.
 *     sum   r = p_0, then r = r + p_j for j = 1, 2, .. in chunk order: one IEEE fp32 addition each, nothing fused, nothing
 *           reassociated, subnormals kept. An empty bag is +0.0.
 *     mean  that sum, then ONE correctly rounded fp32 division by (float)(end - begin).
 *   skip_missing != 0  (an unknown entry is left out of its bag)
 *     p_j   the same loop over the KNOWN entries of chunk j, in entry order. A chunk without a known entry contributes
 *           nothing, not even +0.0.
 *     sum   r = the first such p_j, then the later ones are added in chunk order. A bag without a known entry is +0.0.
 *     mean  ONE division by the bag's total number of known entries, which is also counts[b].
 * A bf16 / fp16 result is that fp32 value rounded ONCE to the nearest even value of the type as it is stored; partial sums
 * are fp32 wherever they are kept. Consequences: a bag of at most C entries has exactly the bits of the sequential calls;
 * in general the result is, bit for bit, the sequential MEMB_HIP_POOL_SUM over the derived bags (one per chunk) followed
 * by the in-order loop over those partial sums. The result depends on the inputs alone, never on options, block sizes or
 * the stream.
 */
#ifndef MEMB_HIP_POOLED_CHUNKED_H
#define MEMB_HIP_POOLED_CHUNKED_H

#include "memb_hip_pooled_known.h"

#define MEMB_HIP_POOL_CHUNK 64

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The bytes of device memory a chunked call over n entries in `bags` bags needs as its workspace: an upper bound worked
 * out from n, bags and the model's dim alone (nothing is read from the device, nothing is launched). 0 for a null ctx.
 * It holds the chunk plan and one fp32 partial sum per chunk, for at most bags + ceil(n / C) chunks.
 */
size_t memb_hip_pool_chunked_workspace_bytes(memb_hip_ctx* ctx, size_t n, size_t bags);

/*
 * memb_hip_pool_known_rows_device_typed (skip_missing != 0) or memb_hip_pool_rows_device_typed (skip_missing == 0) under
 * the chunked order. Bag b goes to columns [col_off, col_off + dim) of out + b * ld (ld, col_off in ELEMENTS of out_type),
 * its number of known entries to counts[b] where counts is not NULL (with skip_missing only). rows, offsets, out, counts
 * and workspace are device pointers; the caller owns the workspace (16-byte aligned, at least
 * memb_hip_pool_chunked_workspace_bytes(ctx, n, bags) bytes), the context keeps none: two threads on two streams with two
 * workspaces run at once. The workspace may be reused or freed once the work enqueued on `stream` has ended.
 *
 * Enqueued on `stream`; returns before the kernels end; allocates nothing, never synchronises with the device and reads
 * nothing back. Nothing but the bags' columns, counts and the workspace is written, and no entry of `rows` outside [0, n)
 * is read whatever `offsets` holds. offsets must not decrease; where they do, the call still ends and keeps those two
 * promises, and the bags at and behind a decrease hold unspecified values. bags == 0 is a no-op.
 *
 * The refusals are those of memb_hip_pool_known_rows_device_typed, with its messages, and: a null, misaligned or
 * too-small workspace, counts without skip_missing, and a batch of 2^32 chunks or more (MEMB_HIP_ERR_INVALID,
 * memb_hip_last_error has the reason; nothing is launched).
 */
int memb_hip_pool_rows_chunked_device_typed(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                            size_t bags, void* out, int out_type, size_t ld, size_t col_off, int mode,
                                            int skip_missing, uint32_t* counts, void* workspace, size_t workspace_bytes,
                                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_POOLED_CHUNKED_H */
