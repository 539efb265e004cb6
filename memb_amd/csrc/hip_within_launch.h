// The list of the candidates that precede a mark, host side (include/memb_hip_within.h): the argument checks, how the
// workspace is cut into starts, totals and cosines and the candidates into slices, the launches of within_count,
// within_starts and within_write, and the implementations of the entry points. The kernels are memb_hip_within.hip's,
// handed over as addresses (hip_within.h).
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_ranks_launch.h
// (rankBlocksPerRow: the blocks are the rank unit's; planSliceByBisection) and what that one stands on
// (excludedListRefusal, the slices of hip_query_topk_launch.h). The first part needs neither a context nor the HIP
// runtime: tests/cpp/within_planning_main.cpp includes this file behind hip_ranks_launch.h with
// MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// Bytes of the blocks' int64 starts of nRows rows of n columns: the first area of the workspace.
inline uint64_t withinStartsBytes(uint64_t nRows, uint64_t n)
{
    return nRows * rankBlocksPerRow(n) * 8;
}

// Bytes of the starts and, behind them, the blocks' 32-bit totals, rounded up to 8 so that what lies behind is aligned.
inline uint64_t withinBlockBytes(uint64_t nRows, uint64_t n)
{
    return withinStartsBytes(nRows, n) + (nRows * rankBlocksPerRow(n) * 4 + 7) / 8 * 8;
}

// memb_hip_dense_within_workspace_bytes; 0 where nothing is needed or the sizes are refused
inline uint64_t denseWithinWorkspaceBytes(uint64_t nRows, uint64_t n)
{
    if (n > memb_ranks::MAX_COLUMNS || nRows > memb_ranks::MAX_ROWS) {
        return 0;
    }
    return withinBlockBytes(nRows, n);
}

// What both calls refuse of their marks and their output, or null.
inline const char* withinOutputRefusal(
    const float* thresholds, const int64_t* marks, const int64_t* offsets, const int64_t* cursors, const int64_t* positions,
    const float* values, size_t capacity)
{
    if (!thresholds || !marks || !offsets || !cursors || !positions) {
        return "null argument: thresholds, marks, offsets, cursors and positions are needed";
    }
    if (reinterpret_cast<uintptr_t>(thresholds) % 4 != 0 || reinterpret_cast<uintptr_t>(values) % 4 != 0) {
        return "thresholds and values must be aligned to 4 bytes";
    }
    if (reinterpret_cast<uintptr_t>(marks) % 8 != 0 || reinterpret_cast<uintptr_t>(offsets) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(cursors) % 8 != 0 || reinterpret_cast<uintptr_t>(positions) % 8 != 0) {
        return "marks, offsets, cursors and positions must be aligned to 8 bytes";
    }
    if (capacity > memb_within::MAX_CAPACITY) {
        return "capacity too large: at most 2^62 entries";
    }
    return nullptr;
}

// What memb_hip_dense_within_device refuses, or null.
inline const char* denseWithinArgumentsRefusal(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const float* thresholds, const int64_t* marks,
    const int64_t* excluded, size_t width, size_t ldExcluded, const int64_t* offsets, const int64_t* cursors,
    const int64_t* positions, const float* values, size_t capacity, const void* workspace, size_t workspaceBytes)
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
    if (const char* refusal = withinOutputRefusal(thresholds, marks, offsets, cursors, positions, values, capacity)) {
        return refusal;
    }
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "workspace must be aligned to 8 bytes";
    }
    const uint64_t needed = denseWithinWorkspaceBytes(nRows, n);
    if (needed && (!workspace || workspaceBytes < needed)) {
        return "workspace too small: memb_hip_dense_within_workspace_bytes says how large";
    }
    return nullptr;
}

// The workspace of the fused call with slices of `slice` candidates: the starts and totals of a slice, then its cosines.
inline uint64_t withinSliceBytes(uint64_t nQueries, uint64_t slice)
{
    return withinBlockBytes(nQueries, slice) + 4 * nQueries * slice;
}

// memb_hip_query_within_workspace_bytes without the context; 0 where nothing is needed or the sizes are refused
inline uint64_t queryWithinWorkspaceBytes(uint64_t nQueries, uint64_t n, bool minimal)
{
    if (n > (uint64_t(1) << 36) || nQueries > memb_ranks::MAX_ROWS || !n || !nQueries) {
        return 0;
    }
    return withinSliceBytes(nQueries, std::min(n, minimal ? memb_query_topk::MIN_SLICE : topkRecommendedSlice(nQueries)));
}

// The candidates of one slice under a workspace of workspaceBytes; 0: the workspace is too small.
inline uint64_t planWithinSlice(uint64_t nQueries, uint64_t n, uint64_t workspaceBytes)
{
    return planSliceByBisection(nQueries, n, workspaceBytes, withinSliceBytes);
}

// What memb_hip_query_within_device refuses before it looks at the model, or null. dim: the model's. The matrix call's own
// limits are asked of queryMatrixArgumentsRefusal, with the thresholds standing for the matrix.
inline const char* queryWithinArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const float* thresholds,
    const int64_t* marks, const int64_t* excluded, size_t width, size_t ldExcluded, const int64_t* offsets, const int64_t* cursors,
    const int64_t* positions, const float* values, size_t capacity, const void* workspace, size_t workspaceBytes)
{
    if (const char* refusal = withinOutputRefusal(thresholds, marks, offsets, cursors, positions, values, capacity)) {
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
    if (n && nQueries && (!workspace || !planWithinSlice(nQueries, n, workspaceBytes))) {
        return "workspace too small: memb_hip_query_within_workspace_bytes(.., minimal) says how large";
    }
    return nullptr;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// What a call hands on to launchWithin beside the matrix: the marks, the list of non-candidates and the output.
struct WithinLists {
    const float* thresholds;
    const int64_t* marks;
    const int64_t* excluded;
    size_t width;
    size_t ldExcluded;
    const int64_t* offsets;
    int64_t* cursors;
    int64_t* positions;
    float* values;
    size_t capacity;
};

// within_count over the n >= 0 columns of nRows >= 1 rows into the totals, within_starts into the starts and the cursors,
// within_write into the lists. With n == 0 within_starts alone, which stores zero cursors (and is not needed at all under
// accumulate). `blockArea`: withinBlockBytes(nRows, n) bytes. The current device is the matrix's. Arguments as
// denseWithinArgumentsRefusal lets them through.
int launchWithin(
    const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const WithinLists& lists, bool accumulate, void* blockArea,
    hipStream_t stream)
{
    if (n == 0 && accumulate) {
        return MEMB_HIP_OK;
    }
    memb_within::WithinParams params{};
    params.matrix = matrix;
    params.thresholds = lists.thresholds;
    params.marks = reinterpret_cast<const long long*>(lists.marks);
    params.excluded = reinterpret_cast<const long long*>(lists.excluded);
    params.offsets = reinterpret_cast<const long long*>(lists.offsets);
    params.cursors = reinterpret_cast<long long*>(lists.cursors);
    params.positions = reinterpret_cast<long long*>(lists.positions);
    params.values = lists.values;
    params.starts = static_cast<long long*>(blockArea);
    params.totals = n ? reinterpret_cast<uint32_t*>(static_cast<char*>(blockArea) + withinStartsBytes(nRows, n)) : nullptr;
    params.ld = ld;
    params.ldExcluded = lists.ldExcluded;
    params.base = base;
    params.capacity = static_cast<long long>(lists.capacity);
    params.nRows = static_cast<uint32_t>(nRows);
    params.n = static_cast<uint32_t>(n);
    params.blocksPerRow = rankBlocksPerRow(n);
    params.width = static_cast<uint32_t>(lists.width);
    params.accumulate = accumulate ? 1 : 0;
    void* arguments[1] = {&params};
    // (blocks == 0 where they do not fit one launch: launchWithoutLds refuses, before anything has run)
    const uint32_t blocks = memb::gridBlocks(1, 1, uint64_t(nRows) * params.blocksPerRow);
    if (n) {
        const int code = launchWithoutLds(memb_within::countKernel(), blocks, memb_ranks::COUNT_THREADS, arguments, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    const int code = launchWithoutLds(
        memb_within::startsKernel(), memb::gridBlocks(memb_within::STARTS_WAVES, 1, nRows), memb_within::STARTS_WAVES * WAVE, arguments,
        stream);
    if (code != MEMB_HIP_OK || n == 0) {
        return code;
    }
    return launchWithoutLds(memb_within::writeKernel(), blocks, memb_ranks::COUNT_THREADS, arguments, stream);
}

// memb_hip_dense_within_device
int dense_within_device_checked(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, const WithinLists& lists, bool accumulate,
    void* workspace, size_t workspaceBytes, void* stream)
{
    if (const char* refusal = denseWithinArgumentsRefusal(
            device, matrix, nRows, n, ld, base, lists.thresholds, lists.marks, lists.excluded, lists.width, lists.ldExcluded,
            lists.offsets, lists.cursors, lists.positions, lists.values, lists.capacity, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nRows == 0 || (n == 0 && accumulate)) {   // (nothing to add: the cursors stay as they are)
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    return launchWithin(matrix, nRows, n, ld, base, lists, accumulate, workspace, static_cast<hipStream_t>(stream));
}

// memb_hip_query_within_device: query_ranks_device_checked's loop over the slices, in ascending order, with the three
// kernels in place of the two
int query_within_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n,
    const WithinLists& lists, void* workspace, size_t workspaceBytes, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryWithinArgumentsRefusal(
            queries, nQueries, ldQueries, ctx->dim, rows, n, lists.thresholds, lists.marks, lists.excluded, lists.width,
            lists.ldExcluded, lists.offsets, lists.cursors, lists.positions, lists.values, lists.capacity, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQueries == 0) {
        return MEMB_HIP_OK;
    }
    const char* reason = n ? fusedRefusal(ctx, FUSED_QUERIES) : nullptr;   // (n == 0 writes zero cursors for every model)
    if (reason) {
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const hipStream_t hipStream = static_cast<hipStream_t>(stream);
    if (n == 0) {
        return launchWithin(nullptr, nQueries, 0, 0, 0, lists, false, nullptr, hipStream);
    }
    const size_t slice = planWithinSlice(nQueries, n, workspaceBytes);
    float* matrix = reinterpret_cast<float*>(static_cast<char*>(workspace) + withinBlockBytes(nQueries, slice));
    for (size_t start = 0; start < n; start += slice) {
        const size_t count = std::min(slice, n - start);
        int code = query_matrix_device_checked(ctx, queries, nQueries, ldQueries, rows + start, count, matrix, nullptr, slice, nullptr, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchWithin(matrix, nQueries, count, slice, static_cast<int64_t>(start), lists, start != 0, workspace, hipStream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_query_within_workspace_bytes
size_t query_within_workspace_bytes(const memb_hip_ctx* ctx, size_t nQueries, size_t n, bool minimal)
{
    return ctx ? static_cast<size_t>(queryWithinWorkspaceBytes(nQueries, n, minimal)) : 0;
}

// memb_hip_query_within_kernel_name
const char* query_within_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return "within_count+within_starts+within_write";
    }
    return fusedRefusal(ctx, FUSED_QUERIES) ? "" : "query_matrix_trained+within_count+within_starts+within_write";
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
