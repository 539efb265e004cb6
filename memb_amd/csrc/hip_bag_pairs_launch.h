// Cosine similarity of pairs of bags, host side (include/memb_hip_bag_pairs.h): the launch of the kernel of
// memb_hip_bag_pairs.hip, which hands it over as an address (hip_bag_pairs.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_pooled_launch.h
// (launchPooledKernel, the byte count of a pooled lookup) and hip_norms_launch.h (floatAligned), on hip_fused_launch.h's
// model test and plan. bag_pairs_trained takes the models of FUSED_BAG_PAIRS: no two words per tile are needed.
#pragma once

// bag_pairs_trained over the 2 * pairs bags of pairs >= 1 pairs and n >= 0 entries, for a model fusedRefusal lets through:
// the fused plan (planFused), and a wavefront owns a run of consecutive whole bags (memb_pooled::pooledBagsPerWave, for the
// wavefronts the kernel's registers let a CU hold) rounded up to an even count: a pair is never split.
int launchBagPairsTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, memb_pooled::PoolParams pool, memb_bag_pairs::BagPairParams params,
    hipStream_t stream)
{
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(rows, n, nullptr, ctx->dim, 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const memb::KernelHandle kernel = memb_bag_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    static_assert(4 * memb_bag_pairs::TRAINED_WAVES_PER_SIMD == ONE_TILE_WAVES_PER_CU, "planned like pool_trained");
    const uint32_t owned = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, plan.trained.wordsPerWave, n, pool.bags, ctx->cuCount,
        4 * memb_bag_pairs::TRAINED_WAVES_PER_SIMD);
    void* arguments[3] = {&plan.trained, &pool, &params};
    // (at most (1 << 16) + 1 before, even after)
    return launchPooledKernel(kernel, plan.waves, owned + (owned & 1u), plan.ldsBytes, &pool, arguments, stream);
}

// memb_hip_bag_pair_similarity_device
int bag_pair_similarity_device_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t pairs, int mode, float* cosines,
    float* dots, float* norms, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if ((n && !rows) || (pairs && !offsets)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: rows or offsets");
    }
    if (pairs && !cosines && !dots && !norms) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: at least one of cosines, dots and norms is needed");
    }
    if (mode != MEMB_HIP_POOL_SUM && mode != MEMB_HIP_POOL_MEAN) {
        return fail(MEMB_HIP_ERR_INVALID, "unknown pooling mode " + std::to_string(mode));
    }
    if (!floatAligned(rows) || !floatAligned(offsets) || !floatAligned(cosines) || !floatAligned(dots) || !floatAligned(norms)) {
        return fail(MEMB_HIP_ERR_INVALID, "rows, offsets, cosines, dots and norms must be aligned to 4 bytes");
    }
    if (pairs > (size_t(1) << 35) || n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    if (const char* reason = fusedRefusal(ctx, FUSED_BAG_PAIRS)) {
        return failFused(FUSED_BAG_PAIRS, reason);
    }
    if (pairs == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const memb_pooled::PoolParams pool{offsets, 2ull * pairs, 0, mode == MEMB_HIP_POOL_MEAN ? 1u : 0u};
    return launchBagPairsTrained(
        ctx, rows, n, pool, memb_bag_pairs::BagPairParams{cosines, dots, norms}, static_cast<hipStream_t>(stream));
}

// memb_hip_bag_pairs_kernel_name
const char* bag_pairs_kernel_name(const memb_hip_ctx* ctx)
{
    return !ctx || fusedRefusal(ctx, FUSED_BAG_PAIRS) ? "" : memb_bag_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
}

// memb_hip_bag_pairs_algorithmic_bytes
int bag_pairs_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t pairs, bool cosines, bool dots,
    bool norms, uint64_t* bytes)
{
    if (pairs > (size_t(1) << 35)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    uint64_t pooled = 0;   // per bag: 8 bytes of offsets and 4 * dim stored; per entry: its id and its compressed bytes
    const int code = pooled_algorithmic_bytes_checked(ctx, rows, n, offsets, 2 * pairs, MEMB_HIP_OUT_F32, &pooled);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    *bytes = pooled - 2 * pairs * 4ull * ctx->dim + pairs * (4ull * cosines + 4ull * dots + 8ull * norms);
    return MEMB_HIP_OK;
}
