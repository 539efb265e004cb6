// Cosine similarity of row pairs, host side (include/memb_hip_pairs.h): the launches of the kernels of memb_hip_pairs.hip,
// which hands them over as addresses (hip_pairs.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after hip_norms_launch.h
// (fusedNormsRefusal's conditions, floatAligned and the byte count of the plain decode are used here).
#pragma once

// Whether pairs_trained takes this model at all: norms_trained's models whose wavefronts hold at least one pair.
const char* fusedPairsRefusal(const memb_hip_ctx* ctx)
{
    if (ctx->storage != memb::wire::Storage_Trained) {
        return "fused pair kernel: trained storage only (decode the rows and use the dense entry point)";
    }
    if (ctx->dim % 4 != 0 || ctx->dim > memb_pairs::TRAINED_MAX_DIM) {
        return "fused pair kernel: dim must be a multiple of 4 and at most 512 (decode the rows and use the dense entry point)";
    }
    if (WAVE / ctx->lanesPerWord < 2) {
        return "fused pair kernel: a wavefront of this geometry holds fewer than two words (decode the rows and use the dense entry point)";
    }
    return nullptr;
}

// pairs_trained over the 2 * n entries of n pairs, n >= 1, for a model fusedPairsRefusal lets through. Planned like
// launchNormsTrained -- a decode of 2 n rows by the one-tile kernel, whose LDS and block size the kernel shares --, and a
// wavefront owns a run of consecutive entries sized like a run of bags of one entry (memb_pooled::pooledBagsPerWave),
// rounded up to an even count: a pair is never split.
int launchPairsTrained(memb_hip_ctx* ctx, const uint32_t* pairs, size_t n, float* cosines, float* dots, float* norms, hipStream_t stream)
{
    const size_t entries = 2 * n;
    Lookup planned = floatRows(pairs, entries, nullptr, ctx->dim, 0);
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
    trained.rows = pairs;
    trained.out = nullptr;
    trained.n = entries;
    trained.ld = planned.ld;
    trained.colOff = planned.colOff;
    if (!lookupParamsConsistent(ctx, trained, geometry) || trained.wordsPerWave < 2) {
        return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
    }
    const memb_pairs::PairKernel kernel = memb_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    memb_pairs::PairParams params{};
    params.cosines = cosines;
    params.dots = dots;
    params.norms = norms;
    const uint32_t owned = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, trained.wordsPerWave, entries, entries, ctx->cuCount, ONE_TILE_WAVES_PER_CU);
    params.entriesPerWave = owned + (owned & 1u);   // (at most (1 << 16) + 1 before, even after)
    const uint64_t perBlock = uint64_t(geometry.waves) * params.entriesPerWave;
    const uint64_t blocks = (entries + perBlock - 1) / perBlock;
    if (blocks >= 0x7FFFFFFFull) {
        return fail(MEMB_HIP_ERR_INVALID, "batches too large for one launch");
    }
    void* arguments[2] = {&trained, &params};
    const hipError_t status = launchKernelAddress(
        kernel.address, dim3(static_cast<uint32_t>(blocks)), dim3(geometry.waves * WAVE), geometry.ldsBytes, stream, arguments);
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(kernel.name) + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
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
    if (const char* refusal = fusedPairsRefusal(ctx)) {
        return fail(MEMB_HIP_UNSUPPORTED, refusal);
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
    const memb_pairs::PairKernel kernel = memb_pairs::denseKernel();
    const uint64_t blocks = (uint64_t(n) + memb_pairs::DENSE_WAVES - 1) / memb_pairs::DENSE_WAVES;
    if (blocks >= 0x7FFFFFFFull) {
        return fail(MEMB_HIP_ERR_INVALID, "batches too large for one launch");
    }
    void* arguments[1] = {&params};
    // (no dynamic LDS: launched as it is, like norms_dense)
    hipError_t status = hipLaunchKernel(
        kernel.address, dim3(static_cast<uint32_t>(blocks)), dim3(memb_pairs::DENSE_WAVES * WAVE), arguments, 0,
        static_cast<hipStream_t>(stream));
    status = status != hipSuccess ? status : hipGetLastError();
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(kernel.name) + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// memb_hip_pairs_kernel_name
const char* pairs_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return memb_pairs::denseKernel().name;
    }
    return fusedPairsRefusal(ctx) ? "" : memb_pairs::trainedKernel(lookupHasSub(ctx), ctx->fast).name;
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
