// The number of candidates that precede a mark, host side (include/memb_hip_ranks.h): the argument checks, how the
// workspace is cut into partial counts and cosines and the candidates into slices, the launches of rank_count and
// rank_fold, and the implementations of the entry points. The kernels are memb_hip_ranks.hip's, handed over as addresses
// (hip_ranks.h).
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after
// hip_analogies_launch.h (excludedListRefusal) and hip_query_topk_launch.h (the slices: topkRecommendedSlice, MIN_SLICE,
// MAX_SLICE). The first part needs neither a context nor the HIP runtime: tests/cpp/ranks_planning_main.cpp includes this
// file behind hip_analogies_launch.h with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host
// sanitizers.
#pragma once

// Blocks of rank_count per row over n columns; 0 where n == 0.
inline uint32_t rankBlocksPerRow(uint64_t n)
{
    return static_cast<uint32_t>((n + memb_ranks::BLOCK_RUN - 1) / memb_ranks::BLOCK_RUN);
}

// Bytes of the partial counts of nRows rows of n columns: 4 per block, rounded up to 8 so that what lies behind them is
// aligned.
inline uint64_t rankPartialBytes(uint64_t nRows, uint64_t n)
{
    return (nRows * rankBlocksPerRow(n) * 4 + 7) / 8 * 8;
}

// memb_hip_dense_ranks_workspace_bytes; 0 where nothing is needed or the sizes are refused
inline uint64_t denseRanksWorkspaceBytes(uint64_t nRows, uint64_t n)
{
    if (n > memb_ranks::MAX_COLUMNS || nRows > memb_ranks::MAX_ROWS) {
        return 0;
    }
    return rankPartialBytes(nRows, n);
}

// What both calls refuse of their marks and their output, or null.
inline const char* rankMarksRefusal(const float* thresholds, const int64_t* marks, const int64_t* counts)
{
    if (!thresholds || !marks || !counts) {
        return "null argument: thresholds, marks and counts are needed";
    }
    if (reinterpret_cast<uintptr_t>(thresholds) % 4 != 0) {
        return "thresholds must be aligned to 4 bytes";
    }
    if (reinterpret_cast<uintptr_t>(marks) % 8 != 0 || reinterpret_cast<uintptr_t>(counts) % 8 != 0) {
        return "marks and counts must be aligned to 8 bytes";
    }
    return nullptr;
}

// What memb_hip_dense_ranks_device refuses, or null.
inline const char* denseRanksArgumentsRefusal(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const float* thresholds,
    const int64_t* marks, const int64_t* excluded, size_t width, size_t ldExcluded, const int64_t* counts,
    const void* workspace, size_t workspaceBytes)
{
    if (n > memb_ranks::MAX_COLUMNS || nRows > memb_ranks::MAX_ROWS) {
        return "batch too large: at most 2^16 rows and 2^31 columns";
    }
    if (n && !matrix) {
        return "null argument: matrix is needed where n > 0";
    }
    if (ld < n) {
        return "ld must be at least n";
    }
    if (base < 0 || device < 0) {
        return "base must not be negative and device must be a HIP device";
    }
    if (reinterpret_cast<uintptr_t>(matrix) % 4 != 0) {
        return "matrix must be aligned to 4 bytes";
    }
    if (const char* refusal = rankMarksRefusal(thresholds, marks, counts)) {
        return refusal;
    }
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "workspace must be aligned to 8 bytes";
    }
    const uint64_t needed = denseRanksWorkspaceBytes(nRows, n);
    if (needed && (!workspace || workspaceBytes < needed)) {
        return "workspace too small: memb_hip_dense_ranks_workspace_bytes says how large";
    }
    return nullptr;
}

// The workspace of the fused call with slices of `slice` candidates: the partial counts of a slice, then its cosines.
inline uint64_t rankSliceBytes(uint64_t nQueries, uint64_t slice)
{
    return rankPartialBytes(nQueries, slice) + 4 * nQueries * slice;
}

// memb_hip_query_ranks_workspace_bytes without the context; 0 where nothing is needed or the sizes are refused
inline uint64_t queryRanksWorkspaceBytes(uint64_t nQueries, uint64_t n, bool minimal)
{
    if (n > (uint64_t(1) << 36) || nQueries > memb_ranks::MAX_ROWS || !n || !nQueries) {
        return 0;
    }
    return rankSliceBytes(nQueries, std::min(n, minimal ? memb_query_topk::MIN_SLICE : topkRecommendedSlice(nQueries)));
}

// The candidates of one slice under a workspace of workspaceBytes, by planTopkSlice's rule: all n where they fit,
// otherwise the largest multiple of MIN_SLICE that does, at most MAX_SLICE; 0: the workspace is too small. What a slice
// needs beside its cosines grows with the slice in steps (per BLOCK_RUN columns and query), so the largest multiple is
// found by bisection over sliceBytes(nQueries, slice), which never falls as the slice grows.
template <typename SliceBytes>
inline uint64_t planSliceByBisection(uint64_t nQueries, uint64_t n, uint64_t workspaceBytes, SliceBytes sliceBytes)
{
    if (!nQueries || !n) {
        return 0;
    }
    if (n <= memb_query_topk::MAX_SLICE && sliceBytes(nQueries, n) <= workspaceBytes) {
        return n;
    }
    uint64_t fits = 0;                                                                      // (in units of MIN_SLICE: fits)
    uint64_t beyond = std::min(n, memb_query_topk::MAX_SLICE) / memb_query_topk::MIN_SLICE + 1;   // (does not, or is not asked for)
    while (beyond - fits > 1) {
        const uint64_t middle = fits + (beyond - fits) / 2;
        if (sliceBytes(nQueries, middle * memb_query_topk::MIN_SLICE) <= workspaceBytes) {
            fits = middle;
        } else {
            beyond = middle;
        }
    }
    return fits * memb_query_topk::MIN_SLICE;
}

// planSliceByBisection for the partial counts and cosines of memb_hip_query_ranks_device
inline uint64_t planRanksSlice(uint64_t nQueries, uint64_t n, uint64_t workspaceBytes)
{
    return planSliceByBisection(nQueries, n, workspaceBytes, rankSliceBytes);
}

// What memb_hip_query_ranks_device refuses before it looks at the model, or null. dim: the model's. The matrix call's own
// limits are asked of queryMatrixArgumentsRefusal, with the thresholds standing for the matrix.
inline const char* queryRanksArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const float* thresholds,
    const int64_t* marks, const int64_t* excluded, size_t width, size_t ldExcluded, const int64_t* counts, const void* workspace,
    size_t workspaceBytes)
{
    if (const char* refusal = rankMarksRefusal(thresholds, marks, counts)) {
        return refusal;
    }
    if (const char* refusal = queryMatrixArgumentsRefusal(queries, nQueries, ldQueries, dim, rows, n, thresholds, nullptr, n, nullptr)) {
        return refusal;
    }
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "workspace must be aligned to 8 bytes";
    }
    if (n && nQueries && (!workspace || !planRanksSlice(nQueries, n, workspaceBytes))) {
        return "workspace too small: memb_hip_query_ranks_workspace_bytes(.., minimal) says how large";
    }
    return nullptr;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// rank_count over the n >= 0 columns of nRows >= 1 rows into `partials`, then rank_fold into counts. With n == 0 rank_fold
// alone, which stores zeros (and is not needed at all under accumulate). The current device is the matrix's. Arguments
// as denseRanksArgumentsRefusal lets them through.
int launchRanks(
    const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const float* thresholds, const int64_t* marks,
    const int64_t* excluded, size_t width, size_t ldExcluded, bool accumulate, int64_t* counts, void* partials, hipStream_t stream)
{
    if (n == 0 && accumulate) {
        return MEMB_HIP_OK;
    }
    memb_ranks::RankParams params{};
    params.matrix = matrix;
    params.thresholds = thresholds;
    params.marks = reinterpret_cast<const long long*>(marks);
    params.excluded = reinterpret_cast<const long long*>(excluded);
    params.partials = static_cast<uint32_t*>(partials);
    params.counts = reinterpret_cast<long long*>(counts);
    params.ld = ld;
    params.ldExcluded = ldExcluded;
    params.base = base;
    params.nRows = static_cast<uint32_t>(nRows);
    params.n = static_cast<uint32_t>(n);
    params.blocksPerRow = rankBlocksPerRow(n);
    params.width = static_cast<uint32_t>(width);
    params.accumulate = accumulate ? 1 : 0;
    void* arguments[1] = {&params};
    if (n) {
        // (blocks == 0 where they do not fit one launch: launchWithoutLds refuses)
        const int code = launchWithoutLds(
            memb_ranks::countKernel(), memb::gridBlocks(1, 1, uint64_t(nRows) * params.blocksPerRow), memb_ranks::COUNT_THREADS,
            arguments, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return launchWithoutLds(
        memb_ranks::foldKernel(), memb::gridBlocks(memb_ranks::FOLD_WAVES, 1, nRows), memb_ranks::FOLD_WAVES * WAVE, arguments, stream);
}

// memb_hip_dense_ranks_device
int dense_ranks_device_checked(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const float* thresholds, const int64_t* marks,
    const int64_t* excluded, size_t width, size_t ldExcluded, bool accumulate, int64_t* counts, void* workspace,
    size_t workspaceBytes, void* stream)
{
    if (const char* refusal = denseRanksArgumentsRefusal(
            device, matrix, nRows, n, ld, base, thresholds, marks, excluded, width, ldExcluded, counts, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nRows == 0 || (n == 0 && accumulate)) {   // (nothing to add: counts stay as they are)
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    return launchRanks(
        matrix, nRows, n, ld, base, thresholds, marks, excluded, width, ldExcluded, accumulate, counts, workspace,
        static_cast<hipStream_t>(stream));
}

// memb_hip_query_ranks_device: query_topk_device_checked's loop over the slices with a count in place of the selection
int query_ranks_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n,
    const float* thresholds, const int64_t* marks, const int64_t* excluded, size_t width, size_t ldExcluded, int64_t* counts,
    void* workspace, size_t workspaceBytes, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryRanksArgumentsRefusal(
            queries, nQueries, ldQueries, ctx->dim, rows, n, thresholds, marks, excluded, width, ldExcluded, counts, workspace,
            workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQueries == 0) {
        return MEMB_HIP_OK;
    }
    const char* reason = n ? fusedRefusal(ctx, FUSED_QUERIES) : nullptr;   // (n == 0 writes zeros for every model)
    if (reason) {
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const hipStream_t hipStream = static_cast<hipStream_t>(stream);
    if (n == 0) {
        return launchRanks(nullptr, nQueries, 0, 0, 0, thresholds, marks, excluded, width, ldExcluded, false, counts, nullptr, hipStream);
    }
    const size_t slice = planRanksSlice(nQueries, n, workspaceBytes);
    float* matrix = reinterpret_cast<float*>(static_cast<char*>(workspace) + rankPartialBytes(nQueries, slice));
    for (size_t start = 0; start < n; start += slice) {
        const size_t count = std::min(slice, n - start);
        int code = query_matrix_device_checked(ctx, queries, nQueries, ldQueries, rows + start, count, matrix, nullptr, slice, nullptr, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchRanks(
            matrix, nQueries, count, slice, static_cast<int64_t>(start), thresholds, marks, excluded, width, ldExcluded, start != 0,
            counts, workspace, hipStream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_query_ranks_workspace_bytes
size_t query_ranks_workspace_bytes(const memb_hip_ctx* ctx, size_t nQueries, size_t n, bool minimal)
{
    return ctx ? static_cast<size_t>(queryRanksWorkspaceBytes(nQueries, n, minimal)) : 0;
}

// memb_hip_query_ranks_kernel_name
const char* query_ranks_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return "rank_count+rank_fold";
    }
    return fusedRefusal(ctx, FUSED_QUERIES) ? "" : "query_matrix_trained+rank_count+rank_fold";
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
