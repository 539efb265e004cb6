// Row norms and unit rows, host side (include/memb_hip_norms.h): the launches of the kernels of memb_hip_norms.hip, which
// hands them over as addresses (hip_norms.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the other entry points
// (hip_entry_points.h: the plain decode and its byte count are used here); see that file for the overview.
#pragma once

// Whether the fused kernels take this model at all: norms_trained's condition, and unit_trained's before alignment.
const char* fusedNormsRefusal(const memb_hip_ctx* ctx)
{
    if (ctx->storage != memb::wire::Storage_Trained) {
        return "fused norm kernels: trained storage only (decode the rows and use the dense entry points)";
    }
    if (ctx->dim % 4 != 0 || ctx->dim > memb_norms::TRAINED_MAX_DIM) {
        return "fused norm kernels: dim must be a multiple of 4 and at most 512 (decode the rows and use the dense entry points)";
    }
    return nullptr;
}

// unit_trained stores 16-byte pieces: the aligned output of the decode's piece form.
bool unitRowsFused(const memb_hip_ctx* ctx, const void* out, size_t ld, size_t colOff)
{
    return !fusedNormsRefusal(ctx) && outputMode(ctx->dim, ld, colOff, out, 4, WAVE / ctx->lanesPerWord) != OUT_SCALAR;
}

// norms_trained (out null) or unit_trained over rows[0 .. n), n >= 1, for a model fusedNormsRefusal lets through. Planned
// like launchPooled -- a decode of n rows by the one-tile kernel (planTrained, force = 0, usual index), whose LDS and block
// size these kernels share -- and a wavefront owns a run of consecutive rows sized like a run of bags of one entry
// (memb_pooled::pooledBagsPerWave).
int launchNormsTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t colOff, float* norms, hipStream_t stream)
{
    const bool unit = out != nullptr;
    Lookup planned = floatRows(rows, n, out, unit ? ld : ctx->dim, unit ? colOff : 0);
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
    trained.out = out;
    trained.n = n;
    trained.ld = planned.ld;
    trained.colOff = planned.colOff;
    if (!lookupParamsConsistent(ctx, trained, geometry) || planned.ld < planned.colOff + trained.dim) {
        return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
    }
    const memb_norms::NormKernel kernel = memb_norms::trainedKernel(lookupHasSub(ctx), ctx->fast, unit);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    memb_norms::NormParams params{};
    params.norms = norms;
    params.rowsPerWave = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, trained.wordsPerWave, n, n, ctx->cuCount, ONE_TILE_WAVES_PER_CU);
    const uint64_t perBlock = uint64_t(geometry.waves) * params.rowsPerWave;
    const uint64_t blocks = (n + perBlock - 1) / perBlock;
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

// norms_dense (params.out null) or unit_dense: one wavefront per row, params.n >= 1.
int launchNormsDense(const memb_norms::DenseNormParams& dense, hipStream_t stream)
{
    memb_norms::DenseNormParams params = dense;
    const memb_norms::NormKernel kernel = memb_norms::denseKernel(params.out != nullptr);
    const uint64_t blocks = (params.n + memb_norms::DENSE_WAVES - 1) / memb_norms::DENSE_WAVES;
    if (blocks >= 0x7FFFFFFFull) {
        return fail(MEMB_HIP_ERR_INVALID, "batches too large for one launch");
    }
    void* arguments[1] = {&params};
    // (no dynamic LDS: launched as it is, like the chunk kernels of hip_pooled_launch.h)
    hipError_t status = hipLaunchKernel(
        kernel.address, dim3(static_cast<uint32_t>(blocks)), dim3(memb_norms::DENSE_WAVES * WAVE), arguments, 0, stream);
    status = status != hipSuccess ? status : hipGetLastError();
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(kernel.name) + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

bool floatAligned(const void* pointer)
{
    return reinterpret_cast<uintptr_t>(pointer) % 4 == 0;
}

// memb_hip_row_norms_device
int row_norms_device_checked(memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* norms, void* stream)
{
    if (!ctx || (n && (!rows || !norms))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    if (!floatAligned(norms) || !floatAligned(rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "rows and norms must be aligned to 4 bytes");
    }
    if (const char* refusal = fusedNormsRefusal(ctx)) {
        return fail(MEMB_HIP_UNSUPPORTED, refusal);
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    if (n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    return launchNormsTrained(ctx, rows, n, nullptr, 0, 0, norms, static_cast<hipStream_t>(stream));
}

// memb_hip_decode_unit_rows_device
int decode_unit_rows_device_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, float* norms, void* stream)
{
    if (!ctx || (n && (!rows || !out))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    if (!floatAligned(out) || !floatAligned(norms) || !floatAligned(rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "rows, out and norms must be aligned to 4 bytes");
    }
    if (col_off > ld || ld - col_off < ctx->dim) {
        return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    if (n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const hipStream_t queue = static_cast<hipStream_t>(stream);
    if (unitRowsFused(ctx, out, ld, col_off)) {
        return launchNormsTrained(ctx, rows, n, out, ld, col_off, norms, queue);
    }
    // the plain decode into the caller's columns, then unit_dense in place on them
    const int decoded = launch(ctx, floatRows(rows, n, out, ld, col_off), queue);
    if (decoded != MEMB_HIP_OK) {
        return decoded;
    }
    memb_norms::DenseNormParams params{};
    params.values = out + col_off;
    params.out = out;
    params.norms = norms;
    params.n = n;
    params.ld = ld;
    params.colOff = col_off;
    params.ldValues = ld;
    params.dim = ctx->dim;
    return launchNormsDense(params, queue);
}

// memb_hip_dense_row_norms_device (out null) and memb_hip_dense_unit_rows_device
int dense_norms_device_checked(
    int device, const float* values, size_t n, size_t dim, size_t ldValues, bool unit, float* out, size_t ld, size_t col_off,
    float* norms, void* stream)
{
    if (n && (!values || (unit ? !out : !norms))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    if (dim == 0 || dim > 0xFFFFFFFFull || ldValues < dim || device < 0) {
        return fail(MEMB_HIP_ERR_INVALID, "dim must be 1 .. 2^32 - 1, ld_values at least dim and device a HIP device");
    }
    if (!floatAligned(values) || !floatAligned(out) || !floatAligned(norms)) {
        return fail(MEMB_HIP_ERR_INVALID, "values, out and norms must be aligned to 4 bytes");
    }
    if (unit && (col_off > ld || ld - col_off < dim)) {
        return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    if (n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    memb_norms::DenseNormParams params{};
    params.values = values;
    params.out = unit ? out : nullptr;
    params.norms = norms;
    params.n = n;
    params.ld = ld;
    params.colOff = col_off;
    params.ldValues = ldValues;
    params.dim = static_cast<uint32_t>(dim);
    return launchNormsDense(params, static_cast<hipStream_t>(stream));
}

// memb_hip_norms_kernel_name
const char* norms_kernel_name(const memb_hip_ctx* ctx, bool unit, const void* out, size_t ld, size_t colOff)
{
    if (!ctx) {
        return memb_norms::denseKernel(unit).name;
    }
    if (!unit) {
        return fusedNormsRefusal(ctx) ? "" : memb_norms::trainedKernel(lookupHasSub(ctx), ctx->fast, false).name;
    }
    return unitRowsFused(ctx, out, ld, colOff) ? memb_norms::trainedKernel(lookupHasSub(ctx), ctx->fast, true).name
                                              : memb_norms::denseKernel(true).name;
}

// memb_hip_norms_algorithmic_bytes
int norms_algorithmic_bytes_checked(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, bool unit, bool norms, uint64_t* bytes)
{
    uint64_t decoded = 0;
    const int code = algorithmic_bytes_checked(ctx, rows, n, &decoded);   // per row: its id, its compressed bytes, 4 * dim
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const uint64_t rowBytes = 4ull * ctx->dim;
    *bytes = decoded - (unit ? 0 : n * rowBytes) + (norms ? 4ull * n : 0);
    return MEMB_HIP_OK;
}
