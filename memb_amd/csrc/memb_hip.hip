// HIP (gfx950 / CDNA4) implementation of the memb batch-lookup path behind the
// C ABI in include/memb_hip.h.
//
// Kernels
//   decode_trained : canonical-Huffman bitstream decode + k-means codebook gather
//                    (reference src/trained_compression.cpp:129-135,
//                     src/huffman_table_decoder.h:102-118, src/bit_stream_reader.h:16-31)
//   dequant_uniform: min + (max - min) * v / levels, four IEEE fp32 operations
//                    (reference src/uniform_compression.cpp:64-72)
//   gather_full    : raw fp32 row copy (reference src/full_compression.cpp:37-47)
// A row id of MEMB_HIP_MISSING_ROW yields a zero row (reference src/reader.cpp:43-46).
//
// Work decomposition of decode_trained. A Huffman bitstream is serial, so the
// parallelism is across words and across SEGMENTS of a word: when a model is
// staged, one pass over all rows records the bit position at which every
// S-th symbol of each row starts (a side index, derived data: the file is
// unchanged). A wavefront then owns a tile of 64 / G consecutive batch entries
// and G = ceil(dim / S) lanes decode one word, each its own segment of S
// symbols. Lookup table and codebook sit in LDS; the tile's bitstreams are
// first copied into LDS with wide loads (one 16-byte piece per lane), decoded
// from there, the symbols are staged in LDS one byte each, and the tile is
// written out row contiguous, 16 bytes per lane, so every store instruction
// covers whole 16-byte-aligned runs of output rows. G lanes per word divide
// the LDS needed per lane in flight by G, which is what bounds occupancy.
// One tile per wavefront at a time and short-lived blocks: the hardware's dispatch keeps the
// memory system busier than any persistent pipeline did (rounds 1-3 built three; round 4
// measured them out: planTrained, hip_decode_plan.h). The one pipeline left, decode_records_persistent,
// serves batches of two to four tiles per 16 wavefronts per CU. DESIGN.md section 5 has the
// measurements behind every choice.
//
// Files: hip_device_common.h, hip_trained_kernels.h, hip_rowwise_kernels.h -- device
// code; this file -- the shared constants, the error state, the C ABI, and the host sections it includes in
// dependency order, each a header of its own: hip_context.h -- the context, its switches, device allocation and
// teardown; hip_kernel_table.h -- the decode kernel table and the one kernel launch helper; hip_decode_plan.h -- every
// launch-geometry rule (which kernel a batch runs, with what block size and LDS), nothing that enqueues work;
// hip_decode_launch.h -- the decode launches; hip_fused_launch.h -- what the decode-fused families of the other
// units share: the models they take, the one plan (planFused) and the two launch ends, for every kernel handed over as a
// memb::KernelHandle (hip_kernel_handle.h, which also sizes their grids); hip_pooled_launch.h -- the pooled launches and
// the entry points above them; hip_host_path.h -- how rows reach host buffers (pinned ring, copy threads, centroid indices over PCIe);
// hip_staging.h -- staging of a model to HBM (context creation); hip_encoder.h, hip_words.h -- the write side and
// word -> row on the device; hip_entry_points.h -- the implementations of the other entry points;
// memb_hip_narrow.hip -- the bf16 / fp16 kernels, a translation unit of its own
// that includes the same device headers and hands its kernels over as addresses
// (hip_narrow.h), planned and launched here; memb_hip_pooled.hip -- every sequential pooled kernel (sum / mean
// of each bag of rows or of its known rows, as fp32, bf16 or fp16), handed over the same way through one selector
// (hip_pooled.h); memb_hip_pooled_chunked.hip -- the chunked order's (hip_pooled_chunked.h); memb_hip_pooled_union.hip -- the
// pooled kernels of a ReadersUnion's averaged rows and of dense rows (hip_pooled_union.h); memb_hip_norms.hip -- row norms
// and rows of unit length (hip_norms.h), launched by hip_norms_launch.h, which also holds their entry points;
// memb_hip_pairs.hip -- the cosine similarity of pairs of rows (hip_pairs.h), launched by hip_pairs_launch.h likewise;
// memb_hip_bag_pairs.hip -- that of pairs of pooled bags (hip_bag_pairs.h), launched by hip_bag_pairs_launch.h;
// memb_hip_queries.hip -- that of query vectors against groups of candidate rows (hip_queries.h), launched by
// hip_queries_launch.h; memb_hip_query_matrix.hip -- that of every query against one shared candidate list
// (hip_query_matrix.h), launched by hip_query_matrix_launch.h; memb_hip_query_topk.hip -- the k best columns of every row
// of a matrix (hip_query_topk.h), launched by hip_query_topk_launch.h, slice after slice of the query matrix;
// memb_hip_query_bags.hip -- that of every query against every pooled bag of rows (hip_query_bags.h), launched by
// hip_query_bags_launch.h, as a matrix or slice after slice in front of the same selection; memb_hip_analogies.hip -- the
// selection with a list of excluded positions per row and sums of weighted rows (hip_analogies.h), launched by
// hip_analogies_launch.h through hip_query_topk_launch.h's launches and slice loop; memb_hip_cosmul.hip -- the 3CosMul
// score of every (question, candidate) from the cosines of the question's terms (hip_cosmul.h), launched by
// hip_cosmul_launch.h alone or between the query matrix and that selection, slice after slice; memb_hip_ranks.hip -- per
// row the number of candidates that precede a mark in the selection's order (hip_ranks.h), launched by hip_ranks_launch.h
// alone or behind the query matrix, slice after slice; memb_hip_within.hip -- per row the list of those candidates
// themselves in CSR form, an ordered compaction (hip_within.h), launched by hip_within_launch.h the same two ways.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip.h"
#include "../../include/memb_hip_narrow.h"
#include "../../include/memb_hip_pooled.h"
#include "../../include/memb_hip_pooled_known.h"
#include "../../include/memb_hip_pooled_chunked.h"
#include "../../include/memb_hip_pooled_union.h"
#include "../../include/memb_hip_norms.h"
#include "../../include/memb_hip_pairs.h"
#include "../../include/memb_hip_bag_pairs.h"
#include "../../include/memb_hip_queries.h"
#include "../../include/memb_hip_query_matrix.h"
#include "../../include/memb_hip_query_topk.h"
#include "../../include/memb_hip_query_bags.h"
#include "../../include/memb_hip_analogies.h"
#include "../../include/memb_hip_cosmul.h"
#include "../../include/memb_hip_ranks.h"
#include "../../include/memb_hip_within.h"
#include "codec.h"
#include "hip_narrow.h"
#include "hip_pooled.h"
#include "hip_pooled_chunked.h"
#include "hip_pooled_union.h"
#include "hip_norms.h"
#include "hip_pairs.h"
#include "hip_bag_pairs.h"
#include "hip_queries.h"
#include "hip_query_matrix.h"
#include "hip_query_topk.h"
#include "hip_query_bags.h"
#include "hip_analogies.h"
#include "hip_cosmul.h"
#include "hip_ranks.h"
#include "hip_within.h"
#include "wire.h"
#include "worker_pool.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;
constexpr uint32_t ZERO_KEY = 255;  // codebook slot that always holds 0.0f: at most 255 centroids exist
                                    // (reference src/trained_compression.cpp:29)

thread_local std::string g_lastError;

int fail(int code, const std::string& message)
{
    g_lastError = message;
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t status_ = (expr);                                                             \
        if (status_ != hipSuccess) {                                                             \
            return fail(                                                                         \
                MEMB_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(status_));   \
        }                                                                                        \
    } while (0)

// Device code (all inside this anonymous namespace).
#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"
#include "hip_encoder_kernels.h"
#include "hip_words_kernels.h"

}  // namespace

// Implementations of the entry points; the extern "C" functions at the end of the
// file call them behind an exception barrier.
#include "hip_context.h"

namespace {

#include "hip_kernel_table.h"
#include "hip_decode_plan.h"
#include "hip_decode_launch.h"
#include "hip_fused_launch.h"
#include "hip_pooled_launch.h"
#include "hip_host_path.h"
#include "hip_staging.h"

}  // namespace

#include "hip_encoder.h"
#include "hip_words.h"

namespace {

#include "hip_entry_points.h"
#include "hip_norms_launch.h"
#include "hip_pairs_launch.h"
#include "hip_bag_pairs_launch.h"
#include "hip_queries_launch.h"
#include "hip_query_matrix_launch.h"
#include "hip_query_topk_launch.h"
#include "hip_query_bags_launch.h"
#include "hip_analogies_launch.h"
#include "hip_cosmul_launch.h"
#include "hip_ranks_launch.h"
#include "hip_within_launch.h"

// No C++ exception leaves the library: allocation failures and the like become error codes.
template <typename Call>
int guarded(Call call)
{
    try {
        return call();
    } catch (const std::bad_alloc&) {
        return fail(MEMB_HIP_ERR_DEVICE, "out of host memory");
    } catch (const std::exception& error) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("internal error: ") + error.what());
    } catch (...) {
        return fail(MEMB_HIP_ERR_DEVICE, "internal error");
    }
}

}  // namespace

extern "C" {

const char* memb_hip_last_error(void)
{
    return g_lastError.c_str();
}

void memb_hip_ctx_destroy(memb_hip_ctx* ctx)
{
    destroy(ctx);
}

int memb_hip_device_count(int* count)
{
    return guarded([&] { return device_count_checked(count); });
}

int memb_hip_ctx_create_trained(memb_hip_ctx** out, int device, const memb_hip_trained_desc* desc)
{
    return guarded([&] { return ctx_create_trained_checked(out, device, desc); });
}

int memb_hip_ctx_create_uniform(memb_hip_ctx** out, int device, const memb_hip_uniform_desc* desc)
{
    return guarded([&] { return ctx_create_uniform_checked(out, device, desc); });
}

int memb_hip_ctx_create_full(memb_hip_ctx** out, int device, const memb_hip_full_desc* desc)
{
    return guarded([&] { return ctx_create_full_checked(out, device, desc); });
}

int memb_hip_ctx_get_info(const memb_hip_ctx* ctx, memb_hip_ctx_info* info)
{
    return guarded([&] { return ctx_get_info_checked(ctx, info); });
}

int memb_hip_encoder_create(memb_hip_encoder** encoder, int device, uint32_t dim, const float* split_points, uint32_t n_split_points)
{
    return guarded([&] { return encoder_create_checked(encoder, device, dim, split_points, n_split_points); });
}

void memb_hip_encoder_destroy(memb_hip_encoder* encoder)
{
    destroyEncoder(encoder);
}

int memb_hip_encoder_add_rows(memb_hip_encoder* encoder, const float* rows, size_t n_rows)
{
    return guarded([&] { return encoder_add_rows_checked(encoder, rows, n_rows); });
}

int memb_hip_encoder_counts(memb_hip_encoder* encoder, uint64_t* counts)
{
    return guarded([&] { return encoder_counts_checked(encoder, counts); });
}

int memb_hip_encoder_rows(memb_hip_encoder* encoder, uint64_t* n_rows)
{
    return guarded([&] { return encoder_rows_checked(encoder, n_rows); });
}

int memb_hip_encoder_pack(
    memb_hip_encoder* encoder, const uint16_t* codes, const uint8_t* lengths, uint32_t* stream_bytes, uint64_t* total_bytes)
{
    return guarded([&] { return encoder_pack_checked(encoder, codes, lengths, stream_bytes, total_bytes); });
}

int memb_hip_encoder_fetch(memb_hip_encoder* encoder, uint8_t* packed, uint64_t capacity)
{
    return guarded([&] { return encoder_fetch_checked(encoder, packed, capacity); });
}

int memb_hip_abi_version(void)
{
    return MEMB_HIP_ABI_VERSION;
}

int memb_hip_ctx_set_option(memb_hip_ctx* ctx, const char* name, uint64_t value)
{
    return guarded([&] { return option_set_checked(ctx, name, value); });
}

int memb_hip_decode_rows_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, void* stream)
{
    return guarded([&] { return decode_rows_device_ex_checked(ctx, rows, n, out, ld, col_off, stream, 0, 0.f); });
}

int memb_hip_decode_rows_device_ex(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, void* stream, uint32_t flags, float divisor)
{
    return guarded([&] { return decode_rows_device_ex_checked(ctx, rows, n, out, ld, col_off, stream, flags, divisor); });
}

int memb_hip_decode_rows_device_typed(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, void* out, int out_type, size_t ld, size_t col_off, void* stream)
{
    return guarded([&] { return decode_rows_device_typed_checked(ctx, rows, n, out, out_type, ld, col_off, stream); });
}

int memb_hip_pool_rows_device(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, float* out, size_t ld,
    size_t col_off, int mode, void* stream)
{
    return guarded([&] {
        return pool_rows_device_checked(ctx, rows, n, offsets, bags, out, MEMB_HIP_OUT_F32, ld, col_off, mode, stream);
    });
}

int memb_hip_pool_rows_device_typed(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, void* out, int out_type, size_t ld,
    size_t col_off, int mode, void* stream)
{
    return guarded([&] { return pool_rows_device_checked(ctx, rows, n, offsets, bags, out, out_type, ld, col_off, mode, stream); });
}

int memb_hip_pool_known_rows_device_typed(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, void* out, int out_type, size_t ld,
    size_t col_off, int mode, uint32_t* counts, void* stream)
{
    return guarded([&] {
        return pool_rows_device_checked(ctx, rows, n, offsets, bags, out, out_type, ld, col_off, mode, stream, true, counts);
    });
}

int memb_hip_pool_rows_union_device(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, size_t count, size_t n, const uint32_t* offsets, size_t bags, void* out,
    int out_type, size_t ld, size_t col_off, int mode, void* stream)
{
    return guarded([&] { return pool_rows_union_device_checked(ctxs, rows, count, n, offsets, bags, out, out_type, ld, col_off, mode, stream); });
}

const char* memb_hip_pool_union_kernel_name(const memb_hip_ctx* first)
{
    return first ? first->pooledUnionKernel : "";
}

const char* memb_hip_pool_dense_kernel_name(int out_type)
{
    const memb::KernelHandle kernel = memb_pooled::pooledDenseKernel(out_type);
    return kernel.address ? kernel.name : "";
}

int memb_hip_pool_dense_rows_device(
    int device, const float* values, size_t n, size_t dim, size_t ld_values, const uint32_t* offsets, size_t bags, void* out,
    int out_type, size_t ld, size_t col_off, int mode, void* stream)
{
    return guarded([&] {
        return pool_dense_rows_device_checked(device, values, n, dim, ld_values, offsets, bags, out, out_type, ld, col_off, mode, stream);
    });
}

size_t memb_hip_pool_chunked_workspace_bytes(memb_hip_ctx* ctx, size_t n, size_t bags)
{
    return ctx ? memb_pooled::chunkWorkspace(n, bags, ctx->dim).bytes : 0;
}

int memb_hip_pool_rows_chunked_device_typed(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, void* out, int out_type, size_t ld,
    size_t col_off, int mode, int skip_missing, uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return pool_rows_chunked_checked(
            ctx, rows, n, offsets, bags, out, out_type, ld, col_off, mode, skip_missing != 0, counts, workspace, workspace_bytes,
            stream);
    });
}

int memb_hip_pooled_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, uint64_t* bytes)
{
    return guarded([&] { return pooled_algorithmic_bytes_checked(ctx, rows, n, offsets, bags, MEMB_HIP_OUT_F32, bytes); });
}

int memb_hip_pooled_algorithmic_bytes_typed(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, int out_type, uint64_t* bytes)
{
    return guarded([&] { return pooled_algorithmic_bytes_checked(ctx, rows, n, offsets, bags, out_type, bytes); });
}

int memb_hip_row_norms_device(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* norms, void* stream)
{
    return guarded([&] { return row_norms_device_checked(ctx, rows, n, norms, stream); });
}

int memb_hip_decode_unit_rows_device(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, float* norms_or_null, void* stream)
{
    return guarded([&] { return decode_unit_rows_device_checked(ctx, rows, n, out, ld, col_off, norms_or_null, stream); });
}

int memb_hip_dense_row_norms_device(
    int device, const float* values, size_t n, size_t dim, size_t ld_values, float* norms, void* stream)
{
    return guarded([&] { return dense_norms_device_checked(device, values, n, dim, ld_values, false, nullptr, 0, 0, norms, stream); });
}

int memb_hip_dense_unit_rows_device(
    int device, const float* values, size_t n, size_t dim, size_t ld_values, float* out, size_t ld, size_t col_off,
    float* norms_or_null, void* stream)
{
    return guarded([&] {
        return dense_norms_device_checked(device, values, n, dim, ld_values, true, out, ld, col_off, norms_or_null, stream);
    });
}

const char* memb_hip_norms_kernel_name(const memb_hip_ctx* ctx, int unit_rows, const void* out, size_t ld, size_t col_off)
{
    return norms_kernel_name(ctx, unit_rows != 0, out, ld, col_off);
}

int memb_hip_norms_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, int unit_rows, int norms, uint64_t* bytes)
{
    return guarded([&] { return norms_algorithmic_bytes_checked(ctx, rows, n, unit_rows != 0, norms != 0, bytes); });
}

int memb_hip_pair_similarity_device(
    memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, float* cosines, float* dots, float* norms, void* stream)
{
    return guarded([&] { return pair_similarity_device_checked(ctx, pairs, n, cosines, dots, norms, stream); });
}

int memb_hip_dense_pair_similarity_device(
    int device, const float* values, size_t n, size_t dim, size_t ld_values, float* cosines, float* dots, float* norms,
    void* stream)
{
    return guarded([&] { return dense_pair_similarity_device_checked(device, values, n, dim, ld_values, cosines, dots, norms, stream); });
}

const char* memb_hip_pairs_kernel_name(const memb_hip_ctx* ctx)
{
    return pairs_kernel_name(ctx);
}

int memb_hip_pairs_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, int cosines, int dots, int norms, uint64_t* bytes)
{
    return guarded([&] { return pairs_algorithmic_bytes_checked(ctx, pairs, n, cosines != 0, dots != 0, norms != 0, bytes); });
}

int memb_hip_bag_pair_similarity_device(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t pairs, int mode, float* cosines,
    float* dots, float* norms, void* stream)
{
    return guarded([&] { return bag_pair_similarity_device_checked(ctx, rows, n, offsets, pairs, mode, cosines, dots, norms, stream); });
}

const char* memb_hip_bag_pairs_kernel_name(const memb_hip_ctx* ctx)
{
    return bag_pairs_kernel_name(ctx);
}

int memb_hip_bag_pairs_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t pairs, int cosines, int dots,
    int norms, uint64_t* bytes)
{
    return guarded([&] {
        return bag_pairs_algorithmic_bytes_checked(ctx, rows, n, offsets, pairs, cosines != 0, dots != 0, norms != 0, bytes);
    });
}

int memb_hip_query_similarity_device(
    memb_hip_ctx* ctx, const float* queries, size_t groups, size_t ld_queries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, float* cosines, float* dots, float* norms, void* stream)
{
    return guarded([&] {
        return query_similarity_device_checked(ctx, queries, groups, ld_queries, rows, n, offsets, cosines, dots, norms, stream);
    });
}

const char* memb_hip_query_kernel_name(const memb_hip_ctx* ctx)
{
    return query_kernel_name(ctx);
}

int memb_hip_query_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t groups, int cosines, int dots,
    int norms, uint64_t* bytes)
{
    return guarded([&] {
        return query_algorithmic_bytes_checked(ctx, rows, n, offsets, groups, cosines != 0, dots != 0, norms != 0, bytes);
    });
}

int memb_hip_query_matrix_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n, float* cosines,
    float* dots, size_t ld_out, float* norms, void* stream)
{
    return guarded([&] {
        return query_matrix_device_checked(ctx, queries, n_queries, ld_queries, rows, n, cosines, dots, ld_out, norms, stream);
    });
}

const char* memb_hip_query_matrix_kernel_name(const memb_hip_ctx* ctx)
{
    return query_matrix_kernel_name(ctx);
}

int memb_hip_query_matrix_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t n_queries, int cosines, int dots, int norms, uint64_t* bytes)
{
    return guarded([&] {
        return query_matrix_algorithmic_bytes_checked(ctx, rows, n, n_queries, cosines != 0, dots != 0, norms != 0, bytes);
    });
}

int memb_hip_dense_topk_device(
    int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base, uint32_t k, int merge, float* values,
    int64_t* positions, size_t ld_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return dense_topk_device_checked(
            device, matrix, n_rows, n, ld, base, k, merge != 0, values, positions, ld_out, workspace, workspace_bytes, stream);
    });
}

size_t memb_hip_dense_topk_workspace_bytes(size_t n_rows, size_t n, uint32_t k)
{
    return static_cast<size_t>(denseTopkWorkspaceBytes(n_rows, n, k));
}

int memb_hip_query_topk_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n, uint32_t k,
    float* values, int64_t* positions, size_t ld_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return query_topk_device_checked(
            ctx, queries, n_queries, ld_queries, rows, n, k, values, positions, ld_out, workspace, workspace_bytes, stream);
    });
}

size_t memb_hip_query_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, uint32_t k, int minimal)
{
    return query_topk_workspace_bytes(ctx, n_queries, n, k, minimal != 0);
}

const char* memb_hip_query_topk_kernel_name(const memb_hip_ctx* ctx)
{
    return query_topk_kernel_name(ctx);
}

int memb_hip_query_topk_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t n_queries, uint32_t k, uint64_t* bytes)
{
    return guarded([&] { return query_topk_algorithmic_bytes_checked(ctx, rows, n, n_queries, k, bytes); });
}

int memb_hip_query_bags_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, size_t bags, int mode, float* cosines, float* dots, size_t ld_out, float* norms, void* stream)
{
    return guarded([&] {
        return query_bags_device_checked(
            ctx, queries, n_queries, ld_queries, rows, n, offsets, bags, mode, cosines, dots, ld_out, norms, stream);
    });
}

const char* memb_hip_query_bags_kernel_name(const memb_hip_ctx* ctx)
{
    return query_bags_kernel_name(ctx);
}

int memb_hip_query_bags_algorithmic_bytes(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, size_t n_queries, int cosines,
    int dots, int norms, uint64_t* bytes)
{
    return guarded([&] {
        return query_bags_algorithmic_bytes_checked(ctx, rows, n, offsets, bags, n_queries, cosines != 0, dots != 0, norms != 0, bytes);
    });
}

int memb_hip_query_bags_topk_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, size_t bags, int mode, uint32_t k, float* values, int64_t* positions, size_t ld_out, void* workspace,
    size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return query_bags_topk_device_checked(
            ctx, queries, n_queries, ld_queries, rows, n, offsets, bags, mode, k, values, positions, ld_out, workspace,
            workspace_bytes, stream);
    });
}

size_t memb_hip_query_bags_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t bags, uint32_t k, int minimal)
{
    return query_bags_topk_workspace_bytes(ctx, n_queries, bags, k, minimal != 0);
}

const char* memb_hip_query_bags_topk_kernel_name(const memb_hip_ctx* ctx)
{
    return query_bags_topk_kernel_name(ctx);
}

int memb_hip_dense_excluding_topk_device(
    int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base, uint32_t k, int merge,
    const int64_t* excluded, size_t width, size_t ld_excluded, float* values, int64_t* positions, size_t ld_out, void* workspace,
    size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return dense_topk_excluding_device_checked(
            device, matrix, n_rows, n, ld, base, k, merge != 0, excluded, width, ld_excluded, values, positions, ld_out, workspace,
            workspace_bytes, stream);
    });
}

int memb_hip_query_excluding_topk_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n, uint32_t k,
    const int64_t* excluded, size_t width, size_t ld_excluded, float* values, int64_t* positions, size_t ld_out, void* workspace,
    size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return query_topk_excluding_device_checked(
            ctx, queries, n_queries, ld_queries, rows, n, k, excluded, width, ld_excluded, values, positions, ld_out, workspace,
            workspace_bytes, stream);
    });
}

const char* memb_hip_query_excluding_topk_kernel_name(const memb_hip_ctx* ctx)
{
    return query_topk_excluding_kernel_name(ctx);
}

int memb_hip_weighted_rows_sum_device(
    int device, const float* matrix, size_t ld, const float* weights, const uint32_t* offsets, size_t n_sums, size_t dim,
    float* out, size_t ld_out, void* stream)
{
    return guarded([&] {
        return weighted_rows_sum_device_checked(device, matrix, ld, weights, offsets, n_sums, dim, out, ld_out, stream);
    });
}

int memb_hip_cosmul_scores_device(
    int device, const float* cosines, size_t ld, const uint32_t* offsets, const uint32_t* negatives_from, size_t n_questions,
    size_t n, float* scores, size_t ld_scores, void* stream)
{
    return guarded([&] {
        return cosmul_scores_device_checked(device, cosines, ld, offsets, negatives_from, n_questions, n, scores, ld_scores, stream);
    });
}

int memb_hip_query_cosmul_nearest_device(
    memb_hip_ctx* ctx, const float* terms, size_t n_terms, size_t ld_terms, const uint32_t* offsets, const uint32_t* negatives_from,
    size_t n_questions, const uint32_t* rows, size_t n, uint32_t k, const int64_t* excluded, size_t width, size_t ld_excluded,
    float* values, int64_t* positions, size_t ld_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return query_cosmul_nearest_device_checked(
            ctx, terms, n_terms, ld_terms, offsets, negatives_from, n_questions, rows, n, k, excluded, width, ld_excluded, values,
            positions, ld_out, workspace, workspace_bytes, stream);
    });
}

size_t memb_hip_query_cosmul_workspace_bytes(
    const memb_hip_ctx* ctx, size_t n_terms, size_t n_questions, size_t n, uint32_t k, int minimal)
{
    return query_cosmul_workspace_bytes(ctx, n_terms, n_questions, n, k, minimal != 0);
}

const char* memb_hip_query_cosmul_kernel_name(const memb_hip_ctx* ctx)
{
    return query_cosmul_kernel_name(ctx);
}

int memb_hip_dense_ranks_device(
    int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base, const float* thresholds, const int64_t* marks,
    const int64_t* excluded, size_t width, size_t ld_excluded, int accumulate, int64_t* counts, void* workspace,
    size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return dense_ranks_device_checked(
            device, matrix, n_rows, n, ld, base, thresholds, marks, excluded, width, ld_excluded, accumulate != 0, counts, workspace,
            workspace_bytes, stream);
    });
}

size_t memb_hip_dense_ranks_workspace_bytes(size_t n_rows, size_t n)
{
    return static_cast<size_t>(denseRanksWorkspaceBytes(n_rows, n));
}

int memb_hip_query_ranks_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n,
    const float* thresholds, const int64_t* marks, const int64_t* excluded, size_t width, size_t ld_excluded, int64_t* counts,
    void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        return query_ranks_device_checked(
            ctx, queries, n_queries, ld_queries, rows, n, thresholds, marks, excluded, width, ld_excluded, counts, workspace,
            workspace_bytes, stream);
    });
}

size_t memb_hip_query_ranks_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, int minimal)
{
    return query_ranks_workspace_bytes(ctx, n_queries, n, minimal != 0);
}

const char* memb_hip_query_ranks_kernel_name(const memb_hip_ctx* ctx)
{
    return query_ranks_kernel_name(ctx);
}

int memb_hip_dense_within_device(
    int device, const float* matrix, size_t n_rows, size_t n, size_t ld, int64_t base, const float* thresholds, const int64_t* marks,
    const int64_t* excluded, size_t width, size_t ld_excluded, int accumulate, const int64_t* offsets, int64_t* cursors,
    int64_t* positions, float* values, size_t capacity, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        const WithinLists lists{thresholds, marks, excluded, width, ld_excluded, offsets, cursors, positions, values, capacity};
        return dense_within_device_checked(device, matrix, n_rows, n, ld, base, lists, accumulate != 0, workspace, workspace_bytes, stream);
    });
}

size_t memb_hip_dense_within_workspace_bytes(size_t n_rows, size_t n)
{
    return static_cast<size_t>(denseWithinWorkspaceBytes(n_rows, n));
}

int memb_hip_query_within_device(
    memb_hip_ctx* ctx, const float* queries, size_t n_queries, size_t ld_queries, const uint32_t* rows, size_t n,
    const float* thresholds, const int64_t* marks, const int64_t* excluded, size_t width, size_t ld_excluded, const int64_t* offsets,
    int64_t* cursors, int64_t* positions, float* values, size_t capacity, void* workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        const WithinLists lists{thresholds, marks, excluded, width, ld_excluded, offsets, cursors, positions, values, capacity};
        return query_within_device_checked(ctx, queries, n_queries, ld_queries, rows, n, lists, workspace, workspace_bytes, stream);
    });
}

size_t memb_hip_query_within_workspace_bytes(const memb_hip_ctx* ctx, size_t n_queries, size_t n, int minimal)
{
    return query_within_workspace_bytes(ctx, n_queries, n, minimal != 0);
}

const char* memb_hip_query_within_kernel_name(const memb_hip_ctx* ctx)
{
    return query_within_kernel_name(ctx);
}

int memb_hip_decode_batches_device(memb_hip_ctx* ctx, const memb_hip_batch* batches, size_t count, void* stream)
{
    return guarded([&] { return decode_batches_device_checked(ctx, batches, count, stream); });
}

int memb_hip_decode_rows(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off)
{
    return guarded([&] { return decode_rows_checked(ctx, rows, n, out, ld, col_off); });
}

int memb_hip_decode_words(memb_hip_ctx* ctx, const memb_hip_words* batch, float* out, size_t ld, size_t col_off)
{
    return guarded([&] {
        if (!ctx || !batch) {
            return fail(MEMB_HIP_ERR_INVALID, "null argument");
        }
        return decode_rows_checked(ctx, nullptr, 0, out, ld, col_off, batch);
    });
}

int memb_hip_decode_rows_union_device(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, const size_t* col_offs, size_t count, size_t n, float* out,
    size_t ld, void* stream, uint32_t flags)
{
    return guarded([&] { return decode_rows_union_device_checked(ctxs, rows, col_offs, count, n, out, ld, stream, flags); });
}

int memb_hip_sync(memb_hip_ctx* ctx)
{
    return guarded([&] { return sync_checked(ctx); });
}

int memb_hip_ctx_stage_words(
    memb_hip_ctx* ctx, const char* packed_words, uint64_t packed_bytes, const uint32_t* word_offsets, uint64_t n_words)
{
    return guarded([&] { return stage_words_checked(ctx, packed_words, packed_bytes, word_offsets, n_words); });
}

int memb_hip_words_create(memb_hip_words** words, int device)
{
    return guarded([&] { return words_create_checked(words, device); });
}

void memb_hip_words_destroy(memb_hip_words* words)
{
    destroyWords(words);
}

int memb_hip_words_begin(memb_hip_words* batch, size_t n, size_t bytes_per_word, memb_hip_words_plan* plan)
{
    return guarded([&] { return words_begin_checked(batch, n, bytes_per_word, plan); });
}

int memb_hip_words_commit(memb_hip_words* batch)
{
    return guarded([&] { return words_commit_checked(batch); });
}

int memb_hip_words_pack(memb_hip_words* batch, const char* const* words, const uint32_t* lengths, size_t n)
{
    return guarded([&] { return words_pack_checked(batch, words, lengths, n); });
}

int memb_hip_resolve_range_device(
    memb_hip_ctx* ctx, const memb_hip_words* batch, size_t first_word, size_t n_words, uint32_t* rows_dev, void* stream)
{
    return guarded([&] { return resolve_range_device_checked(ctx, batch, first_word, n_words, rows_dev, static_cast<hipStream_t>(stream)); });
}

int memb_hip_words_count(const memb_hip_words* batch, size_t* n)
{
    return guarded([&] { return words_count_checked(batch, n); });
}

int memb_hip_resolve_rows_device(memb_hip_ctx* ctx, const memb_hip_words* batch, uint32_t* rows_dev, void* stream)
{
    return guarded([&] { return resolve_rows_device_checked(ctx, batch, rows_dev, static_cast<hipStream_t>(stream)); });
}

int memb_hip_resolve_range_union_device(
    memb_hip_ctx* const* ctxs, size_t count, const memb_hip_words* batch, size_t first_word, size_t n_words,
    uint32_t* const* rows_dev, void* stream)
{
    return guarded([&] {
        return resolve_range_union_device_checked(ctxs, count, batch, first_word, n_words, rows_dev, static_cast<hipStream_t>(stream));
    });
}

int memb_hip_resolve_packed_device(
    memb_hip_ctx* ctx, const uint8_t* bytes_dev, const uint32_t* offsets_dev, size_t n, uint32_t* rows_dev, void* stream)
{
    return guarded([&] {
        return resolve_packed_device_checked(ctx, bytes_dev, 0xFFFFFFFFull, offsets_dev, n, rows_dev, static_cast<hipStream_t>(stream));
    });
}

int memb_hip_resolve_packed_device_bounded(
    memb_hip_ctx* ctx, const uint8_t* bytes_dev, size_t bytes_len, const uint32_t* offsets_dev, size_t n, uint32_t* rows_dev,
    void* stream)
{
    return guarded([&] {
        return resolve_packed_device_checked(ctx, bytes_dev, bytes_len, offsets_dev, n, rows_dev, static_cast<hipStream_t>(stream));
    });
}

int memb_hip_algorithmic_bytes(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, uint64_t* bytes)
{
    return guarded([&] { return algorithmic_bytes_checked(ctx, rows, n, bytes); });
}

}  // extern "C"
