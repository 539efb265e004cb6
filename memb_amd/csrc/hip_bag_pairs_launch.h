// Cosine similarity of pairs of bags, host side (include/memb_hip_bag_pairs.h): the launch of the kernel of
// memb_hip_bag_pairs.hip, which hands it over as an address (hip_bag_pairs.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_pooled_launch.h
// (the byte count of a pooled lookup) and hip_norms_launch.h (floatAligned).
#pragma once

// Whether bag_pairs_trained takes this model at all: pool_trained's register form, which needs no two words per tile.
const char* fusedBagPairsRefusal(const memb_hip_ctx* ctx)
{
    if (ctx->storage != memb::wire::Storage_Trained) {
        return "fused bag-pair kernel: trained storage only (pool the bags and use the dense pair entry point)";
    }
    if (ctx->dim % 4 != 0 || ctx->dim > memb_bag_pairs::TRAINED_MAX_DIM) {
        return "fused bag-pair kernel: dim must be a multiple of 4 and at most 512 (pool the bags and use the dense pair entry point)";
    }
    return nullptr;
}

// bag_pairs_trained over the 2 * pairs bags of pairs >= 1 pairs, for a model fusedBagPairsRefusal lets through. Planned
// like launchPooled plans pool_trained -- a decode of n rows by the one-tile kernel, whose LDS and block size the kernel
// shares --, and a wavefront owns a run of consecutive whole bags (memb_pooled::pooledBagsPerWave, for the wavefronts the
// kernel's registers let a CU hold) rounded up to an even count: a pair is never split.
int launchBagPairsTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, memb_pooled::PoolParams pool, memb_bag_pairs::BagPairParams params,
    hipStream_t stream)
{
    Lookup planned = floatRows(rows, std::max<size_t>(n, 1), nullptr, ctx->dim, 0);
    TrainedPlan plan;
    const int code = planTrained(ctx, planned, 0, false, rowsUnordered(ctx, false), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const TrainedGeometry geometry = plan.geometry;
    if (!geometry.waves) {
        return fail(MEMB_HIP_ERR_INVALID, "decode tables and bitstream slots do not fit into LDS");
    }
    TrainedParams trained = lookupParams(ctx);
    trained.rows = rows;
    trained.out = nullptr;
    trained.n = n;
    trained.ld = planned.ld;
    trained.colOff = planned.colOff;
    if (!lookupParamsConsistent(ctx, trained, geometry)) {
        return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
    }
    const memb_bag_pairs::BagPairKernel kernel = memb_bag_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    static_assert(4 * memb_bag_pairs::TRAINED_WAVES_PER_SIMD == ONE_TILE_WAVES_PER_CU, "planned like pool_trained");
    const uint32_t owned = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, trained.wordsPerWave, n, pool.bags, ctx->cuCount, 4 * memb_bag_pairs::TRAINED_WAVES_PER_SIMD);
    void* arguments[3] = {&trained, &pool, &params};
    // (at most (1 << 16) + 1 before, even after)
    return launchPooledKernel(
        memb_pooled::PoolKernel{kernel.address, kernel.name}, geometry.waves, owned + (owned & 1u), geometry.ldsBytes, &pool,
        arguments, stream);
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
    if (const char* refusal = fusedBagPairsRefusal(ctx)) {
        return fail(MEMB_HIP_UNSUPPORTED, refusal);
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
    return !ctx || fusedBagPairsRefusal(ctx) ? "" : memb_bag_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
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
