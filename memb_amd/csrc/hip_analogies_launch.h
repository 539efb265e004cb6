// Selection with exclusion lists and sums of weighted rows, host side (include/memb_hip_analogies.h): the argument checks
// the two calls add to their siblings', the selection they hand to hip_query_topk_launch.h's launches and slice loop, the
// launch of weighted_rows_sum, and the implementations of the entry points. The kernels are memb_hip_analogies.hip's,
// handed over as addresses (hip_analogies.h).
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after
// hip_query_topk_launch.h (TopkSelection, dense_topk_device_checked, query_topk_device_checked). The first part needs
// neither a context nor the HIP runtime: tests/cpp/analogies_planning_main.cpp includes this file behind
// hip_query_topk_launch.h with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// What the two excluding calls refuse beyond their siblings, or null.
inline const char* excludedListRefusal(const int64_t* excluded, size_t width, size_t ldExcluded)
{
    if (width > memb_analogies::MAX_EXCLUDED) {
        return "width must be at most 64 excluded positions per row";
    }
    if (ldExcluded < width) {
        return "ld_excluded must be at least width";
    }
    if (width && !excluded) {
        return "null argument: excluded is needed where width > 0";
    }
    if (reinterpret_cast<uintptr_t>(excluded) % 8 != 0) {
        return "excluded must be aligned to 8 bytes";
    }
    return nullptr;
}

// What memb_hip_weighted_rows_sum_device refuses, or null.
inline const char* weightedRowsSumRefusal(
    int device, const float* matrix, size_t ld, const float* weights, const uint32_t* offsets, size_t nSums, size_t dim,
    const float* out, size_t ldOut)
{
    if (device < 0) {
        return "device must be a HIP device";
    }
    if (nSums > memb_analogies::MAX_SUMS || dim > memb_analogies::MAX_SUM_DIM) {
        return "batch too large";
    }
    if (!offsets || !out) {
        return "null argument: offsets and out are needed";
    }
    if (ld < dim || ldOut < dim) {
        return "ld and ld_out must be at least dim";
    }
    if (reinterpret_cast<uintptr_t>(matrix) % 4 != 0 || reinterpret_cast<uintptr_t>(weights) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(offsets) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0) {
        return "matrix, weights, offsets and out must be aligned to 4 bytes";
    }
    return nullptr;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// topk_select_excluding with the list as its second parameter; `list` outlives the launches (kernel parameters are copied
// when a launch is enqueued).
TopkSelection excludingTopkSelection(memb_analogies::ExcludedList* list, const int64_t* excluded, size_t width, size_t ldExcluded)
{
    list->excluded = reinterpret_cast<const long long*>(excluded);
    list->ld = ldExcluded;
    list->width = static_cast<uint32_t>(width);
    return TopkSelection{memb_analogies::selectExcludingKernel(), list};
}

// memb_hip_dense_excluding_topk_device
int dense_topk_excluding_device_checked(
    int device, const float* matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
    const int64_t* excluded, size_t width, size_t ldExcluded, float* values, int64_t* positions, size_t ldOut, void* workspace,
    size_t workspaceBytes, void* stream)
{
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    memb_analogies::ExcludedList list{};
    return dense_topk_device_checked(
        device, matrix, nRows, n, ld, base, k, merge, values, positions, ldOut, workspace, workspaceBytes, stream,
        excludingTopkSelection(&list, excluded, width, ldExcluded));
}

// memb_hip_query_excluding_topk_device
int query_topk_excluding_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n, uint32_t k,
    const int64_t* excluded, size_t width, size_t ldExcluded, float* values, int64_t* positions, size_t ldOut, void* workspace,
    size_t workspaceBytes, void* stream)
{
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    memb_analogies::ExcludedList list{};
    return query_topk_device_checked(
        ctx, queries, nQueries, ldQueries, rows, n, k, values, positions, ldOut, workspace, workspaceBytes, stream,
        excludingTopkSelection(&list, excluded, width, ldExcluded));
}

// memb_hip_query_excluding_topk_kernel_name
const char* query_topk_excluding_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return "topk_select_excluding+topk_merge";
    }
    return fusedRefusal(ctx, FUSED_QUERIES) ? "" : "query_matrix_trained+topk_select_excluding+topk_merge";
}

// memb_hip_weighted_rows_sum_device
int weighted_rows_sum_device_checked(
    int device, const float* matrix, size_t ld, const float* weights, const uint32_t* offsets, size_t nSums, size_t dim,
    float* out, size_t ldOut, void* stream)
{
    if (const char* refusal = weightedRowsSumRefusal(device, matrix, ld, weights, offsets, nSums, dim, out, ldOut)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nSums == 0 || dim == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    memb_analogies::WeightedSumParams params{};
    params.matrix = matrix;
    params.weights = weights;
    params.offsets = offsets;
    params.out = out;
    params.ld = ld;
    params.ldOut = ldOut;
    params.nSums = static_cast<uint32_t>(nSums);
    params.dim = static_cast<uint32_t>(dim);
    void* arguments[1] = {&params};
    // (blocks == 0 where the elements do not fit one launch: launchWithoutLds refuses)
    return launchWithoutLds(
        memb_analogies::weightedRowsSumKernel(), memb::gridBlocks(1, memb_analogies::SUM_THREADS, uint64_t(nSums) * dim),
        memb_analogies::SUM_THREADS, arguments, static_cast<hipStream_t>(stream));
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
