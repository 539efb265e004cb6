// Cosine similarity of many query vectors against pooled bags of rows, matrix and top-k, host side
// (include/memb_hip_query_bags.h): the argument checks, the byte counts, the bags a wavefront owns, the launch of the kernel
// of memb_hip_query_bags.hip, which hands it over as an address (hip_query_bags.h), and the implementations of the entry
// points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_query_topk_launch.h
// (planTopkSlice, queryTopkListBytes, launchTopk) and hip_pooled_launch.h (launchPooledKernel), on hip_fused_launch.h's
// model test and plan. The first part needs
// neither a context nor the HIP runtime: tests/cpp/query_bags_planning_main.cpp includes this file behind
// hip_query_topk_launch.h with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// What memb_hip_query_bags_device refuses before it looks at the model, or null. dim: the model's. The sizes are the
// siblings': the bag-pair call's bags and entries, the matrix call's queries.
inline const char* queryBagsArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const uint32_t* offsets,
    size_t bags, int mode, const float* cosines, const float* dots, size_t ldOut, const float* norms)
{
    if (nQueries && !queries) {
        return "null argument: queries";
    }
    if ((n && !rows) || (bags && !offsets)) {
        return "null argument: rows or offsets";
    }
    if (!cosines && !dots && !norms) {
        return "null argument: at least one of cosines, dots and norms is needed";
    }
    if (mode != MEMB_HIP_POOL_SUM && mode != MEMB_HIP_POOL_MEAN) {
        return "unknown pooling mode";
    }
    if (ldQueries < dim) {
        return "ld_queries must be at least dim";
    }
    if ((cosines || dots) && ldOut < bags) {
        return "ld_out must be at least bags";
    }
    const void* pointers[6] = {queries, rows, offsets, cosines, dots, norms};
    for (const void* pointer : pointers) {
        if (reinterpret_cast<uintptr_t>(pointer) % 4 != 0) {
            return "queries, rows, offsets, cosines, dots and norms must be aligned to 4 bytes";
        }
    }
    if (bags > (size_t(1) << 36) || n > (size_t(1) << 37) || nQueries > memb_query_bags::MAX_QUERIES) {
        return "batch too large";
    }
    return nullptr;
}

// memb_hip_query_bags_algorithmic_bytes from `pooled`, what memb_hip_pooled_algorithmic_bytes counts for the bags as fp32:
// without the 4 * dim it stores per bag, plus the matrix header's terms -- 4 * dim per query, 4 bytes per (query, bag) and
// matrix asked for, 4 bytes per bag for the norms.
inline uint64_t queryBagsBytes(
    uint64_t pooled, uint64_t bags, uint64_t nQueries, uint64_t dim, bool cosines, bool dots, bool norms)
{
    return pooled - bags * 4 * dim + nQueries * 4 * dim + nQueries * bags * (4ull * cosines + 4ull * dots) + bags * 4ull * norms;
}

// PoolParams::bagsPerWave of query_bags_trained over bags >= 1 bags of n entries in all. It starts from the pooled plan
// (memb_pooled::pooledBagsPerWave: whole bags, never split, about POOLED_TILES_PER_WAVE tiles, fewer while the grid would
// not fill the machine). A wavefront's work grows with nQueries, so a longer run is shared out among the queries, run /
// nQueries, as planQueryMatrixGrid shares out its tiles -- but never cut below a group of BAG_GROUP bags (a shorter group
// scores with idle registers and stores shorter segments) nor below the run the plan gave to fill the machine. The whole
// run only where ONE block of queries holds them all and one store takes them, nQueries <= min(QUERY_BLOCK, 64 /
// BAG_GROUP): then the kernel keeps the queries' norms across its groups.
inline uint32_t planQueryBagsPerWave(
    uint32_t tilesPerWaveSwitch, uint32_t wordsPerWave, uint64_t n, uint64_t bags, uint64_t nQueries, uint32_t cuCount,
    uint32_t wavesPerCu)
{
    const uint32_t owned = memb_pooled::pooledBagsPerWave(tilesPerWaveSwitch, wordsPerWave, n, bags, cuCount, wavesPerCu);
    const uint64_t perStore = 64 / memb_query_bags::BAG_GROUP;
    if (nQueries <= std::min<uint64_t>(memb_query_bags::QUERY_BLOCK, perStore)) {
        return owned;
    }
    const uint32_t group = std::min(owned, memb_query_bags::BAG_GROUP);
    return static_cast<uint32_t>(std::max<uint64_t>(group, owned / nQueries));
}

// The bags of one slice of memb_hip_query_bags_topk_device and its workspace: memb_hip_query_topk_device's, with bags for
// candidates (planTopkSlice, queryTopkWorkspaceBytes with the bag call's own limit on `bags`).
inline uint64_t queryBagsTopkWorkspaceBytes(uint64_t nQueries, uint64_t bags, uint64_t k, bool minimal)
{
    return queryTopkWorkspaceBytes(nQueries, bags, k, minimal);
}

// What memb_hip_query_bags_topk_device refuses before it looks at the model, or null. The matrix call's own limits are
// asked of queryBagsArgumentsRefusal, with the workspace standing for the matrix.
inline const char* queryBagsTopkArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const uint32_t* offsets,
    size_t bags, int mode, uint32_t k, const float* values, const int64_t* positions, size_t ldOut, const void* workspace,
    size_t workspaceBytes)
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
    if (const char* refusal = queryBagsArgumentsRefusal(
            queries, nQueries, ldQueries, dim, rows, n, offsets, bags, mode, values, nullptr, bags, nullptr)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(positions) % 8 != 0 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "positions and workspace must be aligned to 8 bytes";
    }
    if (bags && nQueries && (!workspace || !planTopkSlice(nQueries, bags, k, workspaceBytes))) {
        return "workspace too small: memb_hip_query_bags_topk_workspace_bytes(.., minimal) says how large";
    }
    return nullptr;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// query_bags_trained over bags >= 1 bags of n >= 0 entries and nQueries >= 1 queries, for a model fusedRefusal lets through
// (FUSED_QUERY_BAGS: bag_pairs_trained's models): the fused plan (planFused) and planQueryBagsPerWave's run.
int launchQueryBagsTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, memb_pooled::PoolParams pool, memb_query_matrix::QueryMatrixParams params,
    hipStream_t stream)
{
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(rows, n, nullptr, ctx->dim, 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (plan.trained.wordsPerWave < 1 || plan.trained.wordsPerWave > WAVE) {
        return inconsistentGeometry();
    }
    const memb::KernelHandle kernel = memb_query_bags::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    const uint32_t owned = planQueryBagsPerWave(
        ctx->switches.tilesPerWave, plan.trained.wordsPerWave, n, pool.bags, params.nQueries, ctx->cuCount,
        4 * memb_query_bags::TRAINED_WAVES_PER_SIMD);
    void* arguments[3] = {&plan.trained, &pool, &params};
    return launchPooledKernel(kernel, plan.waves, owned, plan.ldsBytes, &pool, arguments, stream);
}

// memb_hip_query_bags_device
int query_bags_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, size_t bags, int mode, float* cosines, float* dots, size_t ldOut, float* norms, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryBagsArgumentsRefusal(
            queries, nQueries, ldQueries, ctx->dim, rows, n, offsets, bags, mode, cosines, dots, ldOut, norms)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (bags == 0 || nQueries == 0) {   // a no-op for every model, as the header says
        return MEMB_HIP_OK;
    }
    if (const char* reason = fusedRefusal(ctx, FUSED_QUERY_BAGS)) {
        return failFused(FUSED_QUERY_BAGS, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const memb_pooled::PoolParams pool{offsets, bags, 0, mode == MEMB_HIP_POOL_MEAN ? 1u : 0u};
    memb_query_matrix::QueryMatrixParams params{};
    params.queries = queries;
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    params.ldQueries = ldQueries;
    params.ldOut = ldOut;
    params.nQueries = static_cast<uint32_t>(nQueries);
    return launchQueryBagsTrained(ctx, rows, n, pool, params, static_cast<hipStream_t>(stream));
}

// memb_hip_query_bags_kernel_name
const char* query_bags_kernel_name(const memb_hip_ctx* ctx)
{
    return !ctx || fusedRefusal(ctx, FUSED_QUERY_BAGS) ? "" : memb_query_bags::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
}

// memb_hip_query_bags_algorithmic_bytes
int query_bags_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, size_t nQueries, bool cosines,
    bool dots, bool norms, uint64_t* bytes)
{
    if (bags > (size_t(1) << 36) || nQueries > memb_query_bags::MAX_QUERIES) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    if (!ctx || !bytes) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    uint64_t pooled = 0;   // per bag: 8 bytes of offsets and 4 * dim stored; per entry: its id and its compressed bytes
    if (bags) {
        const int code = pooled_algorithmic_bytes_checked(ctx, rows, n, offsets, bags, MEMB_HIP_OUT_F32, &pooled);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    *bytes = queryBagsBytes(pooled, bags, nQueries, ctx->dim, cosines, dots, norms);
    return MEMB_HIP_OK;
}

// memb_hip_query_bags_topk_device
int query_bags_topk_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, size_t bags, int mode, uint32_t k, float* values, int64_t* positions, size_t ldOut, void* workspace,
    size_t workspaceBytes, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryBagsTopkArgumentsRefusal(
            queries, nQueries, ldQueries, ctx->dim, rows, n, offsets, bags, mode, k, values, positions, ldOut, workspace,
            workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQueries == 0) {
        return MEMB_HIP_OK;
    }
    const char* reason = bags ? fusedRefusal(ctx, FUSED_QUERY_BAGS) : nullptr;   // (bags == 0 fills the empty slots for every model)
    if (reason) {
        return failFused(FUSED_QUERY_BAGS, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    if (bags == 0) {
        return launchTopk(plainTopkSelection(), nullptr, nQueries, 0, 0, 0, k, false, values, positions, ldOut, nullptr, static_cast<hipStream_t>(stream));
    }
    const size_t slice = planTopkSlice(nQueries, bags, k, workspaceBytes);
    float* matrix = reinterpret_cast<float*>(static_cast<char*>(workspace) + queryTopkListBytes(nQueries, k));
    for (size_t start = 0; start < bags; start += slice) {
        const size_t count = std::min(slice, bags - start);
        // (the slice's bags: the offsets advance, the entries stay -- offsets index all of rows[0 .. n))
        int code = query_bags_device_checked(
            ctx, queries, nQueries, ldQueries, rows, n, offsets + start, count, mode, matrix, nullptr, slice, nullptr, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchTopk(
            plainTopkSelection(), matrix, nQueries, count, slice, static_cast<int64_t>(start), k, start != 0, values, positions, ldOut, workspace,
            static_cast<hipStream_t>(stream));
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_query_bags_topk_workspace_bytes
size_t query_bags_topk_workspace_bytes(const memb_hip_ctx* ctx, size_t nQueries, size_t bags, uint32_t k, bool minimal)
{
    return ctx ? static_cast<size_t>(queryBagsTopkWorkspaceBytes(nQueries, bags, k, minimal)) : 0;
}

// memb_hip_query_bags_topk_kernel_name
const char* query_bags_topk_kernel_name(const memb_hip_ctx* ctx)
{
    return !ctx || fusedRefusal(ctx, FUSED_QUERY_BAGS) ? "" : "query_bags_trained+topk_select+topk_merge";
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
