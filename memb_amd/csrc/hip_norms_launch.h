// Row norms and unit rows, host side (include/memb_hip_norms.h): the launches of the kernels of memb_hip_norms.hip, which
// hands them over as addresses (hip_norms.h), and the implementations of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the other entry points
// (hip_entry_points.h: the plain decode and its byte count are used here), on hip_fused_launch.h's model test, plan and
// launch ends; see memb_hip.hip for the overview.
#pragma once

// unit_trained stores 16-byte pieces: a model the fused kernels take (fusedRefusal: norms_trained's only condition) and
// the aligned output of the decode's piece form.
bool unitRowsFused(const memb_hip_ctx* ctx, const void* out, size_t ld, size_t colOff)
{
    return !fusedRefusal(ctx, FUSED_NORMS) && outputMode(ctx->dim, ld, colOff, out, 4, WAVE / ctx->lanesPerWord) != OUT_SCALAR;
}

// norms_trained (out null) or unit_trained over rows[0 .. n), n >= 1, for a model fusedRefusal lets through: the fused
// plan (planFused), and a wavefront owns a run of consecutive rows sized like a run of bags of one entry
// (memb_pooled::pooledBagsPerWave).
int launchNormsTrained(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t colOff, float* norms, hipStream_t stream)
{
    const bool unit = out != nullptr;
    FusedPlan plan;
    const int code = planFused(ctx, floatRows(rows, n, out, unit ? ld : ctx->dim, unit ? colOff : 0), &plan);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const memb::KernelHandle kernel = memb_norms::trainedKernel(lookupHasSub(ctx), ctx->fast, unit);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this model");
    }
    memb_norms::NormParams params{};
    params.norms = norms;
    params.rowsPerWave = memb_pooled::pooledBagsPerWave(
        ctx->switches.tilesPerWave, plan.trained.wordsPerWave, n, n, ctx->cuCount, ONE_TILE_WAVES_PER_CU);
    void* arguments[2] = {&plan.trained, &params};
    return launchOwnedRuns(kernel, plan.waves, plan.ldsBytes, params.rowsPerWave, n, arguments, stream);
}

// norms_dense (params.out null) or unit_dense: one wavefront per row, params.n >= 1.
int launchNormsDense(const memb_norms::DenseNormParams& dense, hipStream_t stream)
{
    memb_norms::DenseNormParams params = dense;
    void* arguments[1] = {&params};
    return launchWithoutLds(
        memb_norms::denseKernel(params.out != nullptr), memb::gridBlocks(memb_norms::DENSE_WAVES, 1, params.n),
        memb_norms::DENSE_WAVES * WAVE, arguments, stream);
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
    if (const char* reason = fusedRefusal(ctx, FUSED_NORMS)) {
        return failFused(FUSED_NORMS, reason);
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
        return fusedRefusal(ctx, FUSED_NORMS) ? "" : memb_norms::trainedKernel(lookupHasSub(ctx), ctx->fast, false).name;
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
