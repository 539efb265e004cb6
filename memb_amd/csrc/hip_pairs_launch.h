// Cosine similarity of row pairs, host side (include/memb_hip_pairs.h): the launches of the kernels of memb_hip_pairs.hip,
// which hands them over as addresses (hip_pairs.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_norms_launch.h
// (floatAligned and the byte count of the plain decode are used here), on hip_fused_launch.h's model test, plan and launch
// ends. pairs_trained takes the models of FUSED_PAIRS: those whose wavefronts hold at least one pair.
#pragma once

// pairs_trained over the 2 * n entries of n pairs, n >= 1, for a model fusedRefusal lets through: the fused plan
// (planFused) of a decode of 2 n rows, and a wavefront owns a run of consecutive entries sized like a run of bags of one
// entry (memb_pooled::pooledBagsPerWave), rounded up to an even count: a pair is never split.
int launchPairsTrained(memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, float* cosines, float* dots, float* norms, hipStream_t stream)
{
    const size_t entries = 2 * n;
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(pairs, entries, nullptr, ctx->dim, 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (plan.trained.wordsPerWave < 2) {
        return inconsistentGeometry();
    }
    const memb::KernelHandle kernel = memb_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    memb_pairs::PairParams params{};
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    const uint32_t owned = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, plan.trained.wordsPerWave, entries, entries, ctx->cuCount, ONE_TILE_WAVES_PER_CU);
    params.entriesPerWave = owned + (owned & 1u);   // (at most (1 << 16) + 1 before, even after)
    void* arguments[2] = {&plan.trained, &params};
    return launchOwnedRuns(kernel, plan.waves, plan.ldsBytes, params.entriesPerWave, entries, arguments, stream);
}

// what both entry points refuse before they look at the model or the matrix
int pairArgumentsRefusal(const void* rows, size_t n, const float* cosines, const float* dots, const float* norms, const char* rowsName)
{
    if (n && !rows) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("null argument: ") + rowsName);
    }
    if (n && !cosines && !dots && !norms) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: at least one of cosines, dots and norms is needed");
    }
    if (!floatAligned(rows) || !floatAligned(cosines) || !floatAligned(dots) || !floatAligned(norms)) {
        return fail(MEMB_HIP_ERR_INVALID, std::string(rowsName) + ", cosines, dots and norms must be aligned to 4 bytes");
    }
    if (n > (size_t(1) << 36)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    return MEMB_HIP_OK;
}

// memb_hip_pair_similarity_device
int pair_similarity_device_checked(
    memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, float* cosines, float* dots, float* norms, void* stream)
{
    const int refused = pairArgumentsRefusal(pairs, n, cosines, dots, norms, "pairs");
    if (refused != MEMB_HIP_OK) {
        return refused;
    }
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* reason = fusedRefusal(ctx, FUSED_PAIRS)) {
        return failFused(FUSED_PAIRS, reason);
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    return launchPairsTrained(ctx, pairs, n, cosines, dots, norms, static_cast<hipStream_t>(stream));
}

// memb_hip_dense_pair_similarity_device
int dense_pair_similarity_device_checked(
    int device, const float* values, size_t n, size_t dim, size_t ldValues, float* cosines, float* dots, float* norms, void* stream)
{
    const int refused = pairArgumentsRefusal(values, n, cosines, dots, norms, "values");
    if (refused != MEMB_HIP_OK) {
        return refused;
    }
    if (dim == 0 || dim > 0xFFFFFFFFull || ldValues < dim || device < 0) {
        return fail(MEMB_HIP_ERR_INVALID, "dim must be 1 .. 2^32 - 1, ld_values at least dim and device a HIP device");
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    memb_pairs::DensePairParams params{};
    params.values = values;
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    params.pairs = n;
    params.ldValues = ldValues;
    params.dim = static_cast<uint32_t>(dim);
    void* arguments[1] = {&params};
    return launchWithoutLds(
        memb_pairs::denseKernel(), memb::gridBlocks(memb_pairs::DENSE_WAVES, 1, n), memb_pairs::DENSE_WAVES * WAVE, arguments,
        static_cast<hipStream_t>(stream));
}

// memb_hip_pairs_kernel_name
const char* pairs_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return memb_pairs::denseKernel().name;
    }
    return fusedRefusal(ctx, FUSED_PAIRS) ? "" : memb_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
}

// memb_hip_pairs_algorithmic_bytes
int pairs_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, bool cosines, bool dots, bool norms, uint64_t* bytes)
{
    if (n > (size_t(1) << 36)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    uint64_t decoded = 0;
    const int code = algorithmic_bytes_checked(ctx, pairs, 2 * n, &decoded);   // per entry: its id, its compressed bytes, 4 * dim
    if (code != MEMB_HIP_OK) {
        return code;
    }
    *bytes = decoded - 2 * n * 4ull * ctx->dim + n * (4ull * cosines + 4ull * dots + 8ull * norms);
    return MEMB_HIP_OK;
}
