/*
 * memb_hip_pooled_known.h -- pooled device lookups over the rows a model KNOWS: the sum or mean of each bag's known
 * entries, and how many there were, decoded and reduced by one kernel (libmemb_hip.so, MI355X / gfx950).
 *
 * An extension of memb_hip_pooled.h, which it includes and leaves as it is: the batch rows[0 .. n), the bags
 * offsets[0 .. bags], MEMB_HIP_POOL_SUM / MEMB_HIP_POOL_MEAN and the MEMB_HIP_OUT_* element types are that header's. There
 * an entry that is not in the model is a row of +0.0 that counts; here it is left out of the bag, as
 * torch.nn.EmbeddingBag leaves out its padding_idx: the mean of a sentence is the mean of the words the model knows.
 *
 * Entry i is KNOWN when rows[i] < n_rows: MEMB_HIP_MISSING_ROW and every id >= n_rows are unknown -- the set that
 * memb_hip_decode_rows_device writes as zeros. Bag b owns the entries [begin, end) with begin = min(offsets[b], n) and
 * end = min(offsets[b + 1], n); K is its known entries, in entry order, and v_k the fp32 row that
 * memb_hip_decode_rows_device writes for one of them:
 *   sum    K empty: +0.0 in every column. Else acc = v_K[0], then acc = acc + v_K[j] for j = 1 .. in that order, one IEEE
 *          fp32 addition each: nothing fused, nothing reassociated, subnormals kept. An unknown entry adds nothing at
 *          all, not even +0.0: a bag whose only known entry is a row of -0.0 gives -0.0.
 *   mean   that sum, then ONE correctly rounded fp32 division by (float)|K|; +0.0 when K is empty.
 *   counts |K| per bag (optional).
 * A bf16 / fp16 result is that fp32 value rounded ONCE to the nearest even value of the type as it is stored -- the bits
 * of fp32_result.to(dtype) on the CPU; no partial sum passes through a narrow `out`. The result depends on the inputs
 * alone, never on launch geometry or options. It is, bit for bit, what memb_hip_pool_rows_device_typed returns for the
 * batch with the unknown entries taken out and the offsets recomputed.
 */
#ifndef MEMB_HIP_POOLED_KNOWN_H
#define MEMB_HIP_POOLED_KNOWN_H

#include "memb_hip_pooled.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bag b goes to columns [col_off, col_off + dim) of out + b * ld (ld, col_off in ELEMENTS of out_type, out aligned to
 * its element), its number of known entries to counts[b] where counts is not NULL. rows (n entries), offsets (bags + 1
 * entries), out and counts (bags entries) are device pointers. Nothing but those columns and counts is written, nothing
 * is allocated, and no entry of `rows` outside [0, n) is read whatever `offsets` holds. Enqueued on `stream`; returns
 * before the kernel ends; safe from several threads on several streams. bags == 0 is a no-op; n == 0 writes zeros to
 * every bag and zero counts. The refusals are those of memb_hip_pool_rows_device_typed, with its messages: a null argument
 * (counts may be null), an unknown mode, an unknown out_type, ld < col_off + dim or a misaligned out give
 * MEMB_HIP_ERR_INVALID (memb_hip_last_error has the reason) and launch nothing. Trained, uniform and full storages; no
 * accumulate, no weights.
 */
int memb_hip_pool_known_rows_device_typed(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets,
                                          size_t bags, void* out, int out_type, size_t ld, size_t col_off, int mode,
                                          uint32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MEMB_HIP_POOLED_KNOWN_H */
