// The k nearest candidates of every query, host side (include/memb_hip_query_topk.h): the argument checks, how a row is
// cut into segments, how the candidates are cut into slices by the workspace, the byte count, the launches of the two
// kernels of memb_hip_query_topk.hip, which hands them over as addresses (hip_query_topk.h), and the implementations of
// the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after
// hip_query_matrix_launch.h (query_matrix_device_checked, queryMatrixArgumentsRefusal), on hip_fused_launch.h's model
// test (FUSED_QUERIES) and launchWithoutLds. The first part needs neither a
// context nor the HIP runtime: tests/cpp/query_topk_planning_main.cpp includes this file behind hip_query_matrix_launch.h
// with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// Segments a row is cut into at most: until TARGET_WAVES wavefronts exist, never more than MAX_SEGMENTS.
inline uint32_t topkMaxSegments(uint64_t nRows)
{
    const uint64_t rows = nRows ? nRows : 1;
    const uint64_t wanted = (memb_query_topk::TARGET_WAVES + rows - 1) / rows;
    return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(wanted, 1), memb_query_topk::MAX_SEGMENTS));
}

struct TopkSegments {
    uint32_t segments;        // per row; 0 where n == 0
    uint32_t segmentLength;   // a multiple of BATCH * UNROLL, at least MIN_SEGMENT
};

// How the n <= MAX_COLUMNS columns of each of nRows rows are spread over topk_select's wavefronts.
inline TopkSegments planTopkSegments(uint64_t nRows, uint64_t n)
{
    const uint64_t most = topkMaxSegments(nRows);
    const uint64_t step = memb_query_topk::BATCH * memb_query_topk::UNROLL;
    uint64_t length = std::max<uint64_t>(memb_query_topk::MIN_SEGMENT, (n + most - 1) / most);
    length = (length + step - 1) / step * step;
    return TopkSegments{static_cast<uint32_t>((n + length - 1) / length), static_cast<uint32_t>(length)};
}

// Bytes of the segment lists of `segments` segments per row: 4 for the value and 4 for the column of each of k ranks.
inline uint64_t topkListBytes(uint64_t nRows, uint64_t segments, uint64_t k)
{
    return nRows * segments * k * 8;
}

// memb_hip_dense_topk_workspace_bytes; 0 where the sizes are refused
inline uint64_t denseTopkWorkspaceBytes(uint64_t nRows, uint64_t n, uint64_t k)
{
    if (k == 0 || k > memb_query_topk::MAX_K || n > memb_query_topk::MAX_COLUMNS || nRows > memb_query_topk::MAX_ROWS) {
        return 0;
    }
    return topkListBytes(nRows, planTopkSegments(nRows, n).segments, k);
}

// What memb_hip_dense_topk_device refuses, or null.
inline const char* denseTopkArgumentsRefusal(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, const float* values,
    const int64_t* positions, size_t ldOut, const void* workspace, size_t workspaceBytes)
{
    if (k == 0 || k > memb_query_topk::MAX_K) {
        return "k must be 1 .. 64";
    }
    if (n > memb_query_topk::MAX_COLUMNS || nRows > memb_query_topk::MAX_ROWS) {
        return "batch too large";
    }
    if ((n && !matrix) || !values || !positions) {
        return "null argument: matrix, values and positions are needed";
    }
    if (ld < n) {
        return "ld must be at least n";
    }
    if (ldOut < k) {
        return "ld_out must be at least k";
    }
    if (base < 0 || device < 0) {
        return "base must not be negative and device must be a HIP device";
    }
    if (reinterpret_cast<uintptr_t>(matrix) % 4 != 0 || reinterpret_cast<uintptr_t>(values) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(positions) % 8 != 0 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "matrix and values must be aligned to 4 bytes, positions and workspace to 8";
    }
    const uint64_t needed = denseTopkWorkspaceBytes(nRows, n, k);
    if (needed && (!workspace || workspaceBytes < needed)) {
        return "workspace too small: memb_hip_dense_topk_workspace_bytes says how large";
    }
    return nullptr;
}

// The slice of the recommended workspace: a (nQueries, slice) matrix of about SLICE_MATRIX_BYTES, a multiple of MIN_SLICE.
inline uint64_t topkRecommendedSlice(uint64_t nQueries)
{
    const uint64_t fits = memb_query_topk::SLICE_MATRIX_BYTES / (4 * (nQueries ? nQueries : 1));
    return std::min(memb_query_topk::MAX_SLICE, std::max(memb_query_topk::MIN_SLICE, fits / memb_query_topk::MIN_SLICE * memb_query_topk::MIN_SLICE));
}

// The lists at the front of memb_hip_query_topk_device's workspace: room for the most segments any slice is cut into.
inline uint64_t queryTopkListBytes(uint64_t nQueries, uint64_t k)
{
    return topkListBytes(nQueries, topkMaxSegments(nQueries), k);
}

// memb_hip_query_topk_workspace_bytes without the context; 0 where nothing is needed or the sizes are refused
inline uint64_t queryTopkWorkspaceBytes(uint64_t nQueries, uint64_t n, uint64_t k, bool minimal)
{
    if (k == 0 || k > memb_query_topk::MAX_K || n > (uint64_t(1) << 36) || nQueries > memb_query_matrix::MAX_QUERIES || !n || !nQueries) {
        return 0;
    }
    const uint64_t slice = std::min(n, minimal ? memb_query_topk::MIN_SLICE : topkRecommendedSlice(nQueries));
    return queryTopkListBytes(nQueries, k) + 4 * nQueries * slice;
}

// The candidates of one slice under a workspace of workspaceBytes: all n where they fit, otherwise the largest multiple
// of MIN_SLICE that does, at most MAX_SLICE; 0: the workspace is too small.
inline uint64_t planTopkSlice(uint64_t nQueries, uint64_t n, uint64_t k, uint64_t workspaceBytes)
{
    const uint64_t lists = queryTopkListBytes(nQueries, k);
    if (!nQueries || !n || workspaceBytes < lists) {
        return 0;
    }
    const uint64_t fits = (workspaceBytes - lists) / (4 * nQueries);
    const uint64_t slice = fits >= n ? n : fits / memb_query_topk::MIN_SLICE * memb_query_topk::MIN_SLICE;
    return std::min(slice, memb_query_topk::MAX_SLICE);
}

// What memb_hip_query_topk_device refuses before it looks at the model, or null. dim: the model's. The matrix call's own
// limits are asked of queryMatrixArgumentsRefusal, with the workspace standing for the matrix.
inline const char* queryTopkArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, uint32_t k,
    const float* values, const int64_t* positions, size_t ldOut, const void* workspace, size_t workspaceBytes)
{
    if (k == 0 || k > memb_query_topk::MAX_K) {
        return "k must be 1 .. 64";
    }
    if (!values || !positions) {
        return "null argument: values and positions are needed";
    }
    if (ldOut < k) {
        return "ld_out must be at least k";
    }
    if (const char* refusal = queryMatrixArgumentsRefusal(queries, nQueries, ldQueries, dim, rows, n, values, nullptr, n, nullptr)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(positions) % 8 != 0 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "positions and workspace must be aligned to 8 bytes";
    }
    if (n && nQueries && (!workspace || !planTopkSlice(nQueries, n, k, workspaceBytes))) {
        return "workspace too small: memb_hip_query_topk_workspace_bytes(.., minimal) says how large";
    }
    return nullptr;
}

// memb_hip_query_topk_algorithmic_bytes from the matrix count without any matrix
inline uint64_t queryTopkBytes(uint64_t withoutMatrix, uint64_t nQueries, uint64_t k)
{
    return withoutMatrix + nQueries * 12 * k;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// The selection stage of launchTopk: topk_select, or a kernel of another unit that takes the same TopkParams first and one
// parameter of its own behind them (hip_analogies_launch.h: topk_select_excluding and its list).
struct TopkSelection {
    memb::KernelHandle kernel;
    void* second;   // the kernel's second parameter; null: it has none
};

TopkSelection plainTopkSelection()
{
    return TopkSelection{memb_query_topk::selectKernel(), nullptr};
}

// The selection over the n >= 0 columns of nRows >= 1 rows into `lists`, then topk_merge into the outputs. The current
// device is the matrix's. Arguments as denseTopkArgumentsRefusal let them through.
int launchTopk(
    const TopkSelection& selection, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
    float* values, int64_t* positions, size_t ldOut, void* lists, hipStream_t stream)
{
    const TopkSegments plan = planTopkSegments(nRows, n);
    memb_query_topk::TopkParams params{};
    params.matrix = matrix;
    params.listValues = static_cast<uint32_t*>(lists);
    params.listColumns = params.listValues + uint64_t(nRows) * plan.segments * k;
    params.values = values;
    params.positions = reinterpret_cast<long long*>(positions);
    params.ld = ld;
    params.ldOut = ldOut;
    params.base = base;
    params.nRows = static_cast<uint32_t>(nRows);
    params.n = static_cast<uint32_t>(n);
    params.k = k;
    params.segments = plan.segments;
    params.segmentLength = plan.segmentLength;
    params.merge = merge ? 1 : 0;
    void* arguments[2] = {&params, selection.second};   // (topk_merge and topk_select take the first alone)
    const memb::KernelHandle kernels[2] = {selection.kernel, memb_query_topk::mergeKernel()};
    const uint64_t waves[2] = {uint64_t(nRows) * plan.segments, nRows};
    for (int stage = 0; stage < 2; ++stage) {
        if (!waves[stage]) {   // (no column: topk_merge alone)
            continue;
        }
        // (at most MAX_ROWS * MAX_SEGMENTS wavefronts: they fit a launch)
        const int code = launchWithoutLds(
            kernels[stage], memb::gridBlocks(memb_query_topk::WAVES_PER_BLOCK, 1, waves[stage]),
            memb_query_topk::WAVES_PER_BLOCK * WAVE, arguments, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_dense_topk_device; with another selection: memb_hip_dense_topk_excluding_device behind its own checks
int dense_topk_device_checked(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge, float* values,
    int64_t* positions, size_t ldOut, void* workspace, size_t workspaceBytes, void* stream,
    const TopkSelection& selection = plainTopkSelection())
{
    if (const char* refusal = denseTopkArgumentsRefusal(device, matrix, nRows, n, ld, base, k, values, positions, ldOut, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nRows == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    return launchTopk(selection, matrix, nRows, n, ld, base, k, merge, values, positions, ldOut, workspace, static_cast<hipStream_t>(stream));
}

// memb_hip_query_topk_device; with another selection: memb_hip_query_topk_excluding_device behind its own checks -- the
// one loop over the slices
int query_topk_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n, uint32_t k,
    float* values, int64_t* positions, size_t ldOut, void* workspace, size_t workspaceBytes, void* stream,
    const TopkSelection& selection = plainTopkSelection())
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryTopkArgumentsRefusal(
            queries, nQueries, ldQueries, ctx->dim, rows, n, k, values, positions, ldOut, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQueries == 0) {
        return MEMB_HIP_OK;
    }
    const char* reason = n ? fusedRefusal(ctx, FUSED_QUERIES) : nullptr;   // (n == 0 fills the empty slots for every model)
    if (reason) {
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    if (n == 0) {
        return launchTopk(selection, nullptr, nQueries, 0, 0, 0, k, false, values, positions, ldOut, nullptr, static_cast<hipStream_t>(stream));
    }
    const size_t slice = planTopkSlice(nQueries, n, k, workspaceBytes);
    float* matrix = reinterpret_cast<float*>(static_cast<char*>(workspace) + queryTopkListBytes(nQueries, k));
    for (size_t start = 0; start < n; start += slice) {
        const size_t count = std::min(slice, n - start);
        int code = query_matrix_device_checked(ctx, queries, nQueries, ldQueries, rows + start, count, matrix, nullptr, slice, nullptr, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchTopk(
            selection, matrix, nQueries, count, slice, static_cast<int64_t>(start), k, start != 0, values, positions, ldOut, workspace,
            static_cast<hipStream_t>(stream));
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_query_topk_workspace_bytes
size_t query_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t nQueries, size_t n, uint32_t k, bool minimal)
{
    return ctx ? static_cast<size_t>(queryTopkWorkspaceBytes(nQueries, n, k, minimal)) : 0;
}

// memb_hip_query_topk_kernel_name
const char* query_topk_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return "topk_select+topk_merge";
    }
    return fusedRefusal(ctx, FUSED_QUERIES) ? "" : "query_matrix_trained+topk_select+topk_merge";
}

// memb_hip_query_topk_algorithmic_bytes
int query_topk_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t nQueries, uint32_t k, uint64_t* bytes)
{
    if (k == 0 || k > memb_query_topk::MAX_K) {
        return fail(MEMB_HIP_ERR_INVALID, "k must be 1 .. 64");
    }
    uint64_t withoutMatrix = 0;
    const int code = query_matrix_algorithmic_bytes_checked(ctx, rows, n, nQueries, false, false, false, &withoutMatrix);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (!bytes) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    *bytes = queryTopkBytes(withoutMatrix, nQueries, k);
    return MEMB_HIP_OK;
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
