// Pooled lookups, host side: the launches of the pooled kernels (the other translation units hand them over as
// addresses: hip_pooled.h, hip_pooled_chunked.h, hip_pooled_union.h) and the implementations of the pooled
// entry points with the argument check they share.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the plans
// (hip_decode_plan.h) and the fused launches' shared part (hip_fused_launch.h); see that file for the overview.
#pragma once

// The end of every sequential pooled launch (launchOwnedRuns): a wavefront owns bagsPerWave bags, which the kernel reads
// from `pool`, its second argument.
int launchPooledKernel(
    const memb::KernelHandle& kernel, uint32_t waves, uint32_t bagsPerWave, uint32_t ldsBytes, memb_pooled::PoolParams* pool,
    void** arguments, hipStream_t stream)
{
    pool->bagsPerWave = bagsPerWave;
    return launchOwnedRuns(kernel, waves, ldsBytes, bagsPerWave, pool->bags, arguments, stream);
}

// A pooled lookup (include/memb_hip_pooled.h): `lookup` describes the ENTRIES (rows, n) and the bags' rows (out, ld, colOff),
// `pool` the bags, both checked by the caller (PooledCall::check: at least one bag, neither count beyond a launch). One kernel of
// memb_hip_pooled.hip, whatever the storage, the element and `known` (memb_pooled::pooledKernel of hip_pooled.h).
// Trained: the fused plan (planFused) -- pool_trained is the one-tile decode up to the symbol tile -- and a wavefront owns
// a run of consecutive whole bags (memb_pooled::pooledBagsPerWave). Bags' rows of a narrow outType run the bf16 / fp16
// kernels on the same plan, and only the choice of the piece form follows the element.
// Uniform, full: one wavefront per bag, blocks of ROWWISE_WAVES.
// known (include/memb_hip_pooled_known.h): the pool_known_* kernels, which leave a bag's unknown entries out and take the
// counts as a third parameter -- the same plan, the same geometry.
int launchPooled(
    memb_hip_ctx* ctx, const Lookup& lookup, memb_pooled::PoolParams pool, hipStream_t stream,
    const memb_pooled::KnownParams* known = nullptr)
{
    memb_pooled::PoolStorage storage;
    bool vec4 = false;
    memb_pooled::KnownParams counted = known ? *known : memb_pooled::KnownParams{};
    void* arguments[3] = {nullptr, &pool, &counted};   // (the third: the pool_known_* kernels only)
    FusedPlan fused;
    UniformParams uniform;
    FullParams full;
    uint32_t waves = memb_pooled::ROWWISE_WAVES;
    uint32_t ldsBytes = 0;
    uint32_t bagsPerWave = 1;
    switch (ctx->storage) {
        case memb::wire::Storage_Trained: {
            storage = memb_pooled::PoolStorage::Trained;
            const int code = planFused(ctx, lookup, &fused);
            if (code != MEMB_HIP_OK) {
                return code;
            }
            const uint32_t wordsPerWave = fused.trained.wordsPerWave;
            const bool pieces =
                outputMode(ctx->dim, lookup.ld, lookup.colOff, lookup.out, lookup.elementBytes(), wordsPerWave) != OUT_SCALAR;
            vec4 = pieces && ctx->dim <= memb_pooled::TRAINED_VEC4_MAX_DIM;
            waves = fused.waves;
            ldsBytes = fused.ldsBytes;
            bagsPerWave = memb_pooled::pooledBagsPerWave(
                ctx->switches.tilesPerWave, wordsPerWave, lookup.n, pool.bags, ctx->cuCount, ONE_TILE_WAVES_PER_CU);
            arguments[0] = &fused.trained;
            break;
        }
        case memb::wire::Storage_Uniform:
            storage = memb_pooled::PoolStorage::Uniform;
            uniform = rowwiseParams<UniformParams>(ctx, lookup);
            uniform.records = ctx->uniformRecords;
            uniform.regionPieces = ctx->regionPieces;
            uniform.levels = ctx->levels;
            arguments[0] = &uniform;
            break;
        case memb::wire::Storage_Full:
            storage = memb_pooled::PoolStorage::Full;
            full = rowwiseParams<FullParams>(ctx, lookup);
            full.values = ctx->fullValues;
            arguments[0] = &full;
            break;
        default:
            return fail(MEMB_HIP_ERR_INVALID, "context has no storage");
    }
    const memb::KernelHandle kernel =
        memb_pooled::pooledKernel(storage, lookupHasSub(ctx), ctx->fast, vec4, lookup.outType, known != nullptr);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this output");
    }
    return launchPooledKernel(kernel, waves, bagsPerWave, ldsBytes, &pool, arguments, stream);
}

// A pooled lookup of a union's AVERAGED rows (include/memb_hip_pooled_union.h), checked by the caller like launchPooled's:
// pool_trained_union of memb_hip_pooled_union.hip (memb_pooled::pooledUnionKernel of hip_pooled_union.h), for the unions
// launchTrainedUnion takes (planUnion) whose dim fits pool_trained's register form; MEMB_HIP_UNSUPPORTED with the reason
// otherwise, nothing launched. LDS per wavefront and the shared image are decode_trained_union's, the block size the one
// with the most resident wavefronts (chooseUnionWaves), the bags of a wavefront launchPooled's.
int launchPooledUnion(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, size_t count, size_t n, memb_pooled::PoolParams pool, void* out,
    int outType, size_t ld, size_t colOff, hipStream_t stream)
{
    size_t colOffs[UNION_MAX_MODELS];
    for (size_t m = 0; m < UNION_MAX_MODELS; ++m) {
        colOffs[m] = colOff;
    }
    UnionPlan plan;
    const int planned = planUnion(ctxs, rows, colOffs, count, n, out, outType == MEMB_HIP_OUT_F32 ? 4 : 2, ld, &plan);
    if (planned != MEMB_HIP_OK) {
        return planned;
    }
    memb_hip_ctx* first = ctxs[0];
    if (first->dim > memb_pooled::TRAINED_VEC4_MAX_DIM) {
        return fail(MEMB_HIP_UNSUPPORTED, "pooled union kernel: dim beyond the register form (" + std::to_string(memb_pooled::TRAINED_VEC4_MAX_DIM) + ")");
    }
    UnionParams& params = plan.params;
    params.rowPieces = first->dim / 4;
    params.rowMagic = magicFor(params.rowPieces, uint64_t(plan.wordsPerWave) * params.rowPieces);
    layOutUnionWave(ctxs, count, plan.wordsPerWave, &params);
    const memb::KernelHandle kernel =
        memb_pooled::pooledUnionKernel(plan.hasSub && !plan.allFast, plan.allFast, static_cast<int>(count), outType);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this output");
    }
    uint32_t waves = 0;
    uint32_t ldsBytes = 0;
    const hipError_t status = chooseUnionWaves(first, kernel.address, params.sharedDwords, params.perWaveDwords, &waves, &ldsBytes);
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(status));
    }
    if (!waves) {
        return fail(MEMB_HIP_UNSUPPORTED, "pooled union kernel: tables and bitstream slots of the models do not fit into LDS together");
    }
    const uint32_t bagsPerWave = memb_pooled::pooledBagsPerWave(
        first->switches.tilesPerWave, plan.wordsPerWave, n, pool.bags, first->cuCount, ONE_TILE_WAVES_PER_CU);
    void* arguments[2] = {&params, &pool};
    const int code = launchPooledKernel(kernel, waves, bagsPerWave, ldsBytes, &pool, arguments, stream);
    if (code == MEMB_HIP_OK) {
        first->pooledUnionKernel = kernel.name;
    }
    return code;
}

// memb_hip_pool_dense_rows_device, checked by the caller like launchPooled's: pool_dense of memb_hip_pooled_union.hip
// (memb_pooled::pooledDenseKernel), one wavefront per bag.
int launchPooledDense(memb_pooled::DenseParams params, memb_pooled::PoolParams pool, int outType, hipStream_t stream)
{
    const memb::KernelHandle kernel = memb_pooled::pooledDenseKernel(outType);
    if (!kernel.address) {
        return fail(MEMB_HIP_ERR_INVALID, std::string("internal error: no ") + kernel.name + " kernel for this output");
    }
    void* arguments[2] = {&params, &pool};
    return launchPooledKernel(kernel, memb_pooled::ROWWISE_WAVES, 1, 0, &pool, arguments, stream);
}

bool knownOutType(int outType)
{
    return outType == MEMB_HIP_OUT_F32 || outType == MEMB_HIP_OUT_BF16 || outType == MEMB_HIP_OUT_F16;
}

// The arguments every pooled entry point takes, and the check they share. The entry point's own go in beside them:
// sourceMissing, its test of what the entries come from (a context and rows, a union's contexts and their rows, dense
// values), and ownRefusal, what it refuses beyond the shared checks (null: nothing).
struct PooledCall {
    bool sourceMissing;
    size_t n;
    const uint32_t* offsets;
    size_t bags;
    void* out;
    int outType;
    size_t ld;
    size_t colOff;
    int mode;
    const char* ownRefusal = nullptr;   // chunked: counts without skip_missing; dense: its dim, ld_values and device
    bool dense = false;                 // ownRefusal comes before the alignment, which is that of `values` too
    const void* values = nullptr;

    struct Checked {
        int code;
        bool launch;                    // false with MEMB_HIP_OK: bags == 0, nothing to do
        memb_pooled::PoolParams pool;   // offsets, bags, mean
    };
    // ONE order: out_type, mode, null arguments, [dense's own,] alignment, ld, [chunked's own,] no bags, a batch beyond one
    // launch. dim() is called once the null check has passed, never before: what it reads need not exist until then.
    template <typename Dim>
    Checked check(Dim dim) const
    {
        const auto refuse = [](const std::string& message) { return Checked{fail(MEMB_HIP_ERR_INVALID, message), false, {}}; };
        if (!knownOutType(outType)) {
            return refuse("unknown out_type " + std::to_string(outType));
        }
        if (mode != MEMB_HIP_POOL_SUM && mode != MEMB_HIP_POOL_MEAN) {
            return refuse("unknown pooling mode " + std::to_string(mode));
        }
        if (sourceMissing || (bags && (!offsets || !out))) {
            return refuse("null argument");
        }
        if (dense && ownRefusal) {
            return refuse(ownRefusal);
        }
        const size_t elementBytes = outType == MEMB_HIP_OUT_F32 ? 4 : 2;
        if (reinterpret_cast<uintptr_t>(out) % elementBytes != 0 || reinterpret_cast<uintptr_t>(values) % 4 != 0) {
            return refuse(
                dense ? "values and out must be aligned to their elements"
                      : "out must be aligned to its element (" + std::to_string(elementBytes) + " bytes)");
        }
        if (colOff > ld || ld - colOff < dim()) {
            return refuse("ld must be at least col_off + dim");
        }
        if (ownRefusal) {
            return refuse(ownRefusal);
        }
        if (bags == 0) {
            return Checked{MEMB_HIP_OK, false, {}};
        }
        if (n > (size_t(1) << 37) || bags >= (1ull << 37)) {
            return refuse("batch too large");
        }
        return Checked{MEMB_HIP_OK, true, {offsets, bags, 0, mode == MEMB_HIP_POOL_MEAN ? 1u : 0u}};
    }
};

// known: memb_hip_pool_known_rows_device_typed -- the same checks, the kernels that skip unknown entries, counts or null
int pool_rows_device_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, void* out, int outType, size_t ld,
    size_t col_off, int mode, void* stream, bool known = false, uint32_t* counts = nullptr)
{
    const PooledCall::Checked checked = PooledCall{!ctx || (n && !rows), n, offsets, bags, out, outType, ld, col_off, mode}.check(
        [&] { return size_t(ctx->dim); });
    if (!checked.launch) {
        return checked.code;
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const memb_pooled::KnownParams counted{counts};
    return launchPooled(
        ctx, Lookup{rows, n, out, outType, ld, col_off}, checked.pool, static_cast<hipStream_t>(stream), known ? &counted : nullptr);
}

// memb_hip_pool_rows_union_device (include/memb_hip_pooled_union.h)
int pool_rows_union_device_checked(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, size_t count, size_t n, const uint32_t* offsets, size_t bags, void* out,
    int outType, size_t ld, size_t col_off, int mode, void* stream)
{
    bool sourceMissing = !ctxs || !rows || count == 0;
    for (size_t m = 0; !sourceMissing && m < count; ++m) {
        sourceMissing = !ctxs[m] || (n && !rows[m]);
    }
    const PooledCall::Checked checked = PooledCall{sourceMissing, n, offsets, bags, out, outType, ld, col_off, mode}.check(
        [&] { return size_t(ctxs[0]->dim); });
    if (!checked.launch) {
        return checked.code;
    }
    DeviceScope deviceScope(ctxs[0]->device);
    HIP_TRY(deviceScope.status());
    return launchPooledUnion(ctxs, rows, count, n, checked.pool, out, outType, ld, col_off, static_cast<hipStream_t>(stream));
}

// memb_hip_pool_dense_rows_device (include/memb_hip_pooled_union.h)
int pool_dense_rows_device_checked(
    int device, const float* values, size_t n, size_t dim, size_t ldValues, const uint32_t* offsets, size_t bags, void* out,
    int outType, size_t ld, size_t col_off, int mode, void* stream)
{
    PooledCall call{n && !values, n, offsets, bags, out, outType, ld, col_off, mode};
    if (dim == 0 || dim > 0xFFFFFFFFull || ldValues < dim || device < 0) {
        call.ownRefusal = "dim must be 1 .. 2^32 - 1, ld_values at least dim and device a HIP device";
    }
    call.dense = true;
    call.values = values;
    const PooledCall::Checked checked = call.check([&] { return dim; });
    if (!checked.launch) {
        return checked.code;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    memb_pooled::DenseParams params{};
    params.values = values;
    params.out = static_cast<float*>(out);
    params.n = n;
    params.ld = ld;
    params.colOff = col_off;
    params.ldValues = ldValues;
    params.dim = static_cast<uint32_t>(dim);
    return launchPooledDense(params, checked.pool, outType, static_cast<hipStream_t>(stream));
}

// memb_hip_pool_rows_chunked_device_typed (include/memb_hip_pooled_chunked.h): the chunk plan, the partial sums of the
// chunks -- launchPooled with MEMB_HIP_POOL_SUM over the derived offsets, into the caller's workspace -- and the bags' sums
// of those, all enqueued on `stream`. The host knows no chunk count: every launch is sized by the workspace's bound.
int pool_rows_chunked_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, void* out, int outType, size_t ld,
    size_t col_off, int mode, bool skip, uint32_t* counts, void* workspace, size_t workspaceBytes, void* stream)
{
    PooledCall call{!ctx || (n && !rows), n, offsets, bags, out, outType, ld, col_off, mode};
    if (counts && !skip) {
        call.ownRefusal = "counts need skip_missing: they are of the entries the model knows";
    }
    const PooledCall::Checked checked = call.check([&] { return size_t(ctx->dim); });
    if (!checked.launch) {
        return checked.code;
    }
    const memb_pooled::ChunkWorkspace layout = memb_pooled::chunkWorkspace(n, bags, ctx->dim);
    if (layout.maxChunks >= 0xFFFFFFFFull) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        return fail(MEMB_HIP_ERR_INVALID, "workspace must be a device pointer aligned to 16 bytes");
    }
    if (workspaceBytes < layout.bytes) {
        return fail(
            MEMB_HIP_ERR_INVALID,
            "workspace of " + std::to_string(workspaceBytes) + " bytes, " + std::to_string(layout.bytes) + " needed");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    const hipStream_t queue = static_cast<hipStream_t>(stream);
    char* const base = static_cast<char*>(workspace);
    uint32_t* const derived = reinterpret_cast<uint32_t*>(base + layout.derived);
    uint32_t* const chunkCounts = reinterpret_cast<uint32_t*>(base + layout.chunkCounts);
    float* const partials = reinterpret_cast<float*>(base + layout.partials);

    memb_pooled::ChunkPlanParams plan{};
    plan.offsets = offsets;
    plan.bags = bags;
    plan.n = n;
    plan.maxChunks = layout.maxChunks;
    plan.planBlocks = layout.planBlocks;
    plan.blockSums = reinterpret_cast<unsigned long long*>(base + layout.blockSums);
    plan.bagStart = reinterpret_cast<uint32_t*>(base + layout.bagStart);
    plan.derived = derived;
    void* planArguments[] = {&plan};
    // (no dynamic LDS, and the scan kernels have static LDS of their own: launchWithoutLds. Every count here is at least 1
    // and, by maxChunks' bound above, fits a launch.)
    const auto enqueue = [&](const char* name, const void* kernel, uint64_t blocks, void** arguments) {
        return launchWithoutLds(
            memb::KernelHandle{kernel, name}, static_cast<uint32_t>(blocks), memb_pooled::PLAN_THREADS, arguments, queue);
    };
    int code = MEMB_HIP_OK;
    if (layout.planBlocks > 1) {   // (one block: its bags' starts need no other block's sum)
        code = enqueue("chunk_block_sums", memb_pooled::chunkBlockSumsKernel(), layout.planBlocks, planArguments);
        if (code == MEMB_HIP_OK) {
            code = enqueue("chunk_scan_sums", memb_pooled::chunkScanSumsKernel(), 1, planArguments);
        }
    }
    if (code == MEMB_HIP_OK) {
        code = enqueue("chunk_bag_starts", memb_pooled::chunkBagStartsKernel(), layout.planBlocks, planArguments);
    }
    if (code == MEMB_HIP_OK) {
        code = enqueue(
            "chunk_offsets", memb_pooled::chunkOffsetsKernel(), layout.maxChunks / memb_pooled::PLAN_THREADS + 1, planArguments);
    }
    if (code != MEMB_HIP_OK) {
        return code;
    }

    memb_pooled::PoolParams chunks{};
    chunks.offsets = derived;
    chunks.bags = layout.maxChunks;
    chunks.mean = 0;
    const memb_pooled::KnownParams counted{chunkCounts};
    code = launchPooled(
        ctx, Lookup{rows, n, partials, MEMB_HIP_OUT_F32, ctx->dim, 0}, chunks, queue, skip ? &counted : nullptr);
    if (code != MEMB_HIP_OK) {
        return code;
    }

    memb_pooled::ChunkSumParams sums{};
    sums.offsets = offsets;
    sums.bagStart = plan.bagStart;
    sums.partials = partials;
    sums.chunkCounts = skip ? chunkCounts : nullptr;
    sums.out = out;
    sums.counts = counts;
    sums.bags = bags;
    sums.n = n;
    sums.ld = ld;
    sums.colOff = col_off;
    sums.dim = ctx->dim;
    sums.mean = checked.pool.mean;
    const uint64_t waves = uint64_t(bags) * ((ctx->dim + WAVE - 1) / WAVE);
    void* sumArguments[] = {&sums};
    return enqueue(
        "pool_chunks", memb_pooled::poolChunksKernel(outType), memb::gridBlocks(memb_pooled::PLAN_THREADS / WAVE, 1, waves),
        sumArguments);
}

int pooled_algorithmic_bytes_checked(
    const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, const uint32_t* offsets, size_t bags, int outType, uint64_t* bytes)
{
    if (!knownOutType(outType)) {
        return fail(MEMB_HIP_ERR_INVALID, "unknown out_type " + std::to_string(outType));
    }
    if (!ctx || !bytes || (n && !rows) || (bags && !offsets)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    const uint64_t elementBytes = outType == MEMB_HIP_OUT_F32 ? 4 : 2;
    uint64_t total = 0;
    for (size_t bag = 0; bag < bags; ++bag) {
        total += 8 + elementBytes * ctx->dim;
        const size_t begin = std::min<size_t>(offsets[bag], n);
        const size_t end = std::min<size_t>(offsets[bag + 1], n);
        for (size_t i = begin; i < end; ++i) {
            total += 4;
            if (rows[i] >= ctx->nRows) {
                continue;
            }
            switch (ctx->storage) {
                case memb::wire::Storage_Trained:
                    total += 4 + ctx->streamBytes[rows[i]];
                    break;
                case memb::wire::Storage_Uniform:
                    total += 12 + ctx->dim;
                    break;
                case memb::wire::Storage_Full:
                    total += 4 + 4ull * ctx->dim;
                    break;
                default:
                    break;
            }
        }
    }
    *bytes = total;
    return MEMB_HIP_OK;
}
