// Cosine similarity of many query vectors against ONE shared list of candidate rows, host side
// (include/memb_hip_query_matrix.h): the argument checks, the byte count and the grid of the kernel of
// memb_hip_query_matrix.hip, which hands it over as an address (hip_query_matrix.h), its launch and the implementations of
// the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_queries_launch.h
// (planQueryGrid), on hip_fused_launch.h's model test (query_trained's models: FUSED_QUERIES), plan and launch ends. The
// first part -- what a call is refused for, what it counts as moved, how its
// candidates are spread over wavefronts and blocks -- needs neither a context nor the HIP runtime:
// tests/cpp/query_matrix_planning_main.cpp includes this file behind hip_queries_launch.h with
// MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host sanitizers.
#pragma once

// What memb_hip_query_matrix_device refuses before it looks at the model, or null. dim: the model's.
inline const char* queryMatrixArgumentsRefusal(
    const float* queries, size_t nQueries, size_t ldQueries, size_t dim, const uint32_t* rows, size_t n, const float* cosines,
    const float* dots, size_t ldOut, const float* norms)
{
    if (nQueries && !queries) {
        return "null argument: queries";
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
    if ((cosines || dots) && ldOut < n) {
        return "ld_out must be at least n";
    }
    const void* pointers[5] = {queries, rows, cosines, dots, norms};
    for (const void* pointer : pointers) {
        if (reinterpret_cast<uintptr_t>(pointer) % 4 != 0) {
            return "queries, rows, cosines, dots and norms must be aligned to 4 bytes";
        }
    }
    if (n > (size_t(1) << 36) || nQueries > memb_query_matrix::MAX_QUERIES) {
        return "batch too large";
    }
    return nullptr;
}

// memb_hip_query_matrix_algorithmic_bytes from `candidates`, the ids and compressed bytes of the n candidates counted once
// (what memb_hip_pooled_algorithmic_bytes counts per entry): 4 * dim per query, 4 bytes per (query, candidate) and matrix
// asked for, 4 bytes per candidate for the norms.
inline uint64_t queryMatrixBytes(
    uint64_t candidates, uint64_t n, uint64_t nQueries, uint64_t dim, bool cosines, bool dots, bool norms)
{
    return candidates + nQueries * 4 * dim + nQueries * n * (4ull * cosines + 4ull * dots) + n * 4ull * norms;
}

// How query_matrix_trained's n >= 1 candidates are spread. It starts from planQueryGrid over n, the run of ONE query. A
// wavefront's work grows with nQueries, so a run of several tiles is shared out among the queries, run / nQueries, but
// never cut below a tile (a shorter tile decodes with idle lanes and stores shorter row segments) nor below the run the
// plan gave to fill the machine. Several tiles only where ONE block of queries holds them all and one store takes them,
// nQueries <= min(QUERY_BLOCK, 64 / W): then the kernel keeps the queries' norms across its tiles, and every query's norm
// is worked out once per wavefront whatever the plan. blocks == 0: too many for one launch.
inline QueryGrid planQueryMatrixGrid(
    uint32_t tilesPerWaveSwitch, uint32_t wordsPerWave, uint64_t n, uint64_t nQueries, uint32_t cuCount, uint32_t waves)
{
    QueryGrid grid = planQueryGrid(tilesPerWaveSwitch, wordsPerWave, n, cuCount, waves);
    const uint32_t tile = std::min(wordsPerWave ? wordsPerWave : 1, grid.entriesPerWave);
    const uint64_t perStore = 64 / (wordsPerWave ? wordsPerWave : 1);
    const bool oneBlock = nQueries <= std::min<uint64_t>(memb_query_matrix::QUERY_BLOCK, perStore);
    const uint64_t shared = grid.entriesPerWave / (nQueries ? nQueries : 1);
    grid.entriesPerWave = oneBlock ? static_cast<uint32_t>(std::max<uint64_t>(tile, shared)) : tile;
    grid.blocks = memb::gridBlocks(waves, grid.entriesPerWave, n);
    return grid;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// query_matrix_trained over n >= 1 candidates and nQueries >= 1 queries, for a model fusedRefusal lets through
// (FUSED_QUERIES): the fused plan (planFused) and planQueryMatrixGrid's run.
int launchQueryMatrixTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, memb_query_matrix::QueryMatrixParams params, hipStream_t stream)
{
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(rows, n, nullptr, ctx->dim, 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (plan.trained.wordsPerWave < 1 || plan.trained.wordsPerWave > WAVE) {
        return inconsistentGeometry();
    }
    const memb::KernelHandle kernel = memb_query_matrix::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    static_assert(memb_query_matrix::TRAINED_WAVES_PER_SIMD == memb_queries::TRAINED_WAVES_PER_SIMD, "planned from planQueryGrid");
    params.entriesPerWave = planQueryMatrixGrid(
        ctx->switches.tilesPerWave, plan.trained.wordsPerWave, n, params.nQueries, ctx->cuCount, plan.waves).entriesPerWave;
    void* arguments[2] = {&plan.trained, &params};
    return launchOwnedRuns(kernel, plan.waves, plan.ldsBytes, params.entriesPerWave, n, arguments, stream);
}

// memb_hip_query_matrix_device
int query_matrix_device_checked(
    memb_hip_ctx* ctx, const float* queries, size_t nQueries, size_t ldQueries, const uint32_t* rows, size_t n, float* cosines,
    float* dots, size_t ldOut, float* norms, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = queryMatrixArgumentsRefusal(queries, nQueries, ldQueries, ctx->dim, rows, n, cosines, dots, ldOut, norms)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (n == 0 || nQueries == 0) {   // a no-op for every model, as the header says
        return MEMB_HIP_OK;
    }
    if (const char* reason = fusedRefusal(ctx, FUSED_QUERIES)) {   // (query_trained's models)
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    memb_query_matrix::QueryMatrixParams params{};
    params.queries = queries;
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    params.ldQueries = ldQueries;
    params.ldOut = ldOut;
    params.nQueries = static_cast<uint32_t>(nQueries);
    return launchQueryMatrixTrained(ctx, rows, n, params, static_cast<hipStream_t>(stream));
}

// memb_hip_query_matrix_kernel_name
const char* query_matrix_kernel_name(const memb_hip_ctx* ctx)
{
    return !ctx || fusedRefusal(ctx, FUSED_QUERIES) ? "" : memb_query_matrix::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
}

// memb_hip_query_matrix_algorithmic_bytes
int query_matrix_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, size_t nQueries, bool cosines, bool dots, bool norms, uint64_t* bytes)
{
    if (n > (size_t(1) << 36) || nQueries > memb_query_matrix::MAX_QUERIES) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    if (!ctx || !bytes || (n && !rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    // the candidates as bags of the pooled count, at most 2^31 entries each (its offsets are 32 bits wide), without what it
    // counts per bag: 8 bytes of offsets and the 4 * dim stored
    uint64_t candidates = 0;
    const size_t slice = size_t(1) << 31;
    for (size_t start = 0; start < n; start += slice) {
        const uint32_t cut[2] = {0, static_cast<uint32_t>(std::min(slice, n - start))};
        uint64_t pooled = 0;
        const int code = pooled_algorithmic_bytes_checked(ctx, rows + start, cut[1], cut, 1, MEMB_HIP_OUT_F32, &pooled);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        candidates += pooled - (8 + 4ull * ctx->dim);
    }
    *bytes = queryMatrixBytes(candidates, n, nQueries, ctx->dim, cosines, dots, norms);
    return MEMB_HIP_OK;
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
