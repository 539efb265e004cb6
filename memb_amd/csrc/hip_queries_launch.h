// Cosine similarity of query vectors against groups of candidate rows, host side (include/memb_hip_queries.h): the
// argument checks and the grid of the kernel of memb_hip_queries.hip, which hands it over as an address (hip_queries.h),
// its launch and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_pooled_launch.h
// (the byte count of a pooled lookup), on hip_fused_launch.h's model test, plan and launch ends. The first part -- what a
// call is refused for, how its entries are spread over wavefronts and blocks (memb::gridBlocks of hip_kernel_handle.h), how
// many entries lie in a group -- needs neither a context nor the HIP runtime: tests/cpp/queries_planning_main.cpp includes
// this file with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// What memb_hip_query_similarity_device refuses before it looks at the model, or null. dim: the model's.
inline const char* queryArgumentsRefusal(
    const float* queries, size_t groups, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const uint32_t* offsets,
    const float* cosines, const float* dots, const float* norms)
{
    if (groups && (!queries || !offsets)) {
        return "null argument: queries or offsets";
    }
    if (n && !rows) {
        return "null argument: rows";
    }
    if (!cosines && !dots && !norms) {
        return "null argument: at least one of cosines, dots and norms is needed";
    }
    if (ldQueries < dim) {
        return "ld_queries must be at least dim";
    }
    const void* pointers[6] = {queries, rows, offsets, cosines, dots, norms};
    for (const void* pointer : pointers) {
        if (reinterpret_cast<uintptr_t>(pointer) % 4 != 0) {
            return "queries, rows, offsets, cosines, dots and norms must be aligned to 4 bytes";
        }
    }
    if (n > (size_t(1) << 36) || groups > 0xFFFFFFFEull) {
        return "batch too large";
    }
    return nullptr;
}

// How query_trained's n >= 1 entries are spread: a wavefront owns a run of consecutive entries sized like a run of bags
// of one entry (memb_pooled::pooledBagsPerWave, for the wavefronts the kernel's registers let a CU hold) -- launchPairsTrained's
// run without the rounding to even --, a block `waves` such runs. blocks == 0: too many for one launch.
struct QueryGrid {
    uint32_t entriesPerWave;   // 1 .. 1 << 16
    uint32_t blocks;
};

inline QueryGrid planQueryGrid(uint32_t tilesPerWaveSwitch, uint32_t wordsPerWave, uint64_t n, uint32_t cuCount, uint32_t waves)
{
    QueryGrid grid{};
    grid.entriesPerWave = memb_pooled::pooledBagsPerWave(
        tilesPerWaveSwitch, wordsPerWave, n, n, cuCount, 4 * memb_queries::TRAINED_WAVES_PER_SIMD);
    grid.blocks = memb::gridBlocks(waves, grid.entriesPerWave, n);
    return grid;
}

// The entries that lie in a group and the groups that are not empty, offsets (HOST, groups + 1 entries) clamped to n as the
// kernel clamps them.
inline void queryGroupEntries(const uint32_t* offsets, size_t groups, size_t n, uint64_t* entries, uint64_t* nonEmpty)
{
    *entries = 0;
    *nonEmpty = 0;
    for (size_t g = 0; g < groups; ++g) {
        const size_t begin = std::min<size_t>(offsets[g], n);
        const size_t end = std::min<size_t>(offsets[g + 1], n);
        if (end > begin) {
            *entries += end - begin;
            *nonEmpty += 1;
        }
    }
}

// memb_hip_query_algorithmic_bytes from the pooled count of the groups as bags (per group 8 bytes of offsets and 4 * dim,
// per entry that lies in a group its id and its compressed bytes): the 4 * dim of an EMPTY group go -- no query is read
// for it --, and every entry that lies in a group gets 4 bytes per output asked for.
inline uint64_t queryBytes(
    uint64_t pooled, uint64_t groups, uint64_t nonEmpty, uint64_t entries, uint64_t dim, bool cosines, bool dots, bool norms)
{
    return pooled - (groups - nonEmpty) * 4 * dim + entries * (4ull * cosines + 4ull * dots + 4ull * norms);
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// query_trained over n >= 1 entries of groups >= 1 groups, for a model fusedRefusal lets through (FUSED_QUERIES: one word
// per wavefront included): the fused plan (planFused) and planQueryGrid's run.
int launchQueriesTrained(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, memb_queries::QueryParams params, hipStream_t stream)
{
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(rows, n, nullptr, ctx->dim, 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (plan.trained.wordsPerWave < 1 || plan.trained.wordsPerWave > WAVE) {
        return inconsistentGeometry();
    }
    const memb::KernelHandle kernel = memb_queries::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    static_assert(4 * memb_queries::TRAINED_WAVES_PER_SIMD == ONE_TILE_WAVES_PER_CU, "planned like pairs_trained");
    params.entriesPerWave =
        planQueryGrid(ctx->switches.tilesPerWave, plan.trained.wordsPerWave, n, ctx->cuCount, plan.waves).entriesPerWave;
    void* arguments[2] = {&plan.trained, &params};
    return launchOwnedRuns(kernel, plan.waves, plan.ldsBytes, params.entriesPerWave, n, arguments, stream);
}

// memb_hip_query_similarity_device
int query_similarity_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t groups, size_t ldQueries, const uint32_t* rows, size_t n,
    const uint32_t* offsets, float* cosines, float* dots, float* norms, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryArgumentsRefusal(queries, groups, ldQueries, ctx->dim, rows, n, offsets, cosines, dots, norms)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (n == 0 || groups == 0) {   // a no-op for every model, as the header says
        return MEMB_HIP_OK;
    }
    if (const char* reason = fusedRefusal(ctx, FUSED_QUERIES)) {
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    memb_queries::QueryParams params{};
    params.queries = queries;
    params.offsets = offsets;
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    params.ldQueries = ldQueries;
    params.groups = static_cast<uint32_t>(groups);
    return launchQueriesTrained(ctx, rows, n, params, static_cast<hipStream_t>(stream));
}

// memb_hip_query_kernel_name
const char* query_kernel_name(const memb_hip_ctx* ctx)
{
    return !ctx || fusedRefusal(ctx, FUSED_QUERIES) ? "" : memb_queries::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
}

// memb_hip_query_algorithmic_bytes
int query_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t groups, bool cosines, bool dots,
    bool norms, uint64_t* bytes)
{
    if (n > (size_t(1) << 36) || groups > 0xFFFFFFFEull) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    uint64_t pooled = 0;   // per group: 8 bytes of offsets and 4 * dim, there stored, here the query read; per entry: its id and its compressed bytes
    const int code = pooled_algorithmic_bytes_checked(ctx, rows, n, offsets, groups, MEMB_HIP_OUT_F32, &pooled);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    uint64_t entries = 0;
    uint64_t nonEmpty = 0;
    queryGroupEntries(offsets, groups, n, &entries, &nonEmpty);
    *bytes = queryBytes(pooled, groups, nonEmpty, entries, ctx->dim, cosines, dots, norms);
    return MEMB_HIP_OK;
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
