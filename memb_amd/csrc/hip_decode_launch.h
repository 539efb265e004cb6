// The decode launches: one function per storage and kernel family, and launch(), where every decode of rows
// into device memory starts.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the plans
// (hip_decode_plan.h); see that file for the overview.
#pragma once

// Enqueues one kernel on `stream` and returns. A narrow lookup (bf16 / fp16) runs decode_trained_narrow, planned like
// decode_trained with half the codebook in LDS. Its instances keep decode_trained's registers -- seven wavefronts per
// SIMD, ONE_TILE_WAVES_PER_CU (tests/test_narrow_isa.py) -- and it runs at every batch size: no narrow
// decode_records_persistent (force = 0). The batch-order word is read for the block size, never
// written: a bf16 batch does not change what the next fp32 one picks.
int launchTrained(memb_hip_ctx* ctx, const Lookup& lookup, hipStream_t stream)
{
    const bool narrow = lookup.outType != MEMB_HIP_OUT_F32;
    TrainedPlan plan;
    int planned = planTrained(ctx, lookup, narrow ? 0 : -1, true, rowsUnordered(ctx, lookup.randomOrder), &plan);
    if (planned != MEMB_HIP_OK) {
        return planned;
    }
    const TrainedGeometry geometry = plan.geometry;
    if (!geometry.waves) {
        return fail(MEMB_HIP_ERR_INVALID, "decode tables and bitstream slots do not fit into LDS");
    }
    TrainedParams params = lookupParams(ctx, plan.fine);
    if (narrow) {
        params.codebookDwords = codebookDwords(ctx) / 2;
    }
    params.rows = lookup.rows;
    params.out = static_cast<float*>(lookup.out);   // (2-byte elements for a narrow type: outputTileNarrow)
    params.n = lookup.n;
    params.ld = lookup.ld;
    params.colOff = lookup.colOff;
    params.accumulate = lookup.accumulate;
    params.divisor = lookup.divisor;
    if (!lookupParamsConsistent(ctx, params, geometry) || lookup.ld < lookup.colOff + params.dim) {
        return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
    }
    const size_t tiles = (lookup.n + params.wordsPerWave - 1) / params.wordsPerWave;
    const uint32_t threads = geometry.waves * WAVE;
    hipError_t status;
    if (plan.persistent) {
        // as many blocks as are resident at once; each wavefront strides over the tiles. (Round 5, batch 11: a grid cut down so
        // that every wavefront gets the SAME number of tiles -- 12 500 tiles as 4 167 wavefronts x 3 instead of 5 120 wavefronts
        // of which 44 % run a third round -- is slower: 100 000 uncached rows +10 % (4-bit), +15 % (6-bit, 2-bit). More wavefronts
        // in flight beat an even last round.)
        const uint32_t tileBlocks = static_cast<uint32_t>((tiles + geometry.waves - 1) / geometry.waves);
        KernelFacts facts;
        status = kernelFacts(plan.kernel->fn, &facts, threads, geometry.ldsBytes);
        if (status == hipSuccess) {
            const uint32_t resident = static_cast<uint32_t>(facts.blocksPerCu) * ctx->cuCount;
            status = launchKernel(plan.kernel->fn, dim3(std::min(tileBlocks, resident)), dim3(threads), geometry.ldsBytes, stream, params);
        }
    } else {
        uint32_t blocks = 0;
        const int code = oneTileBlocks(ctx, tiles, geometry.waves, &params, &blocks);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        // very large batches leave word of their order for the next one (device-resident row ids only: the host-buffer
        // entry points stage slices of the caller's batch)
        const uint64_t R = uint64_t(ctx->cuCount) * PIPELINE_WAVES_PER_CU;
        if (tiles > 16 * R && !narrow && !lookup.keysOut && lookup.rows && ctx->orderSeenDevice) {
            params.orderOut = ctx->orderSeenDevice;
        }
        const uint32_t ldsBytes = std::min<uint32_t>(geometry.ldsBytes + ctx->switches.ldsPad, 160 * 1024);   // (ldsPad: measurement builds)
        if (narrow) {
            void* arguments[] = {&params};
            status = launchKernelAddress(
                memb_narrow::trainedKernel(lookupHasSub(ctx), geometry.mode, ctx->fast, lookup.outType), dim3(blocks), dim3(threads),
                ldsBytes, stream, arguments);
        } else {
            status = launchKernel(plan.kernel->fn, dim3(blocks), dim3(threads), ldsBytes, stream, params);
        }
    }
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(narrow ? "decode_trained_narrow" : "decode_trained") + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// memb_hip_decode_batches_device for a trained storage: the tiles of up to MAX_BATCHES batches numbered through in one
// decode_trained_batches grid (the same body as decode_trained: one tile per wavefront at a time), launch geometry by
// the rule of a single batch with as many words as all of them together.
int launchTrainedBatches(memb_hip_ctx* ctx, const memb_hip_batch* batches, size_t count, hipStream_t stream)
{
    size_t words = 0;
    int mode = OUT_FLAT;
    for (size_t k = 0; k < count; ++k) {
        const memb_hip_batch& batch = batches[k];
        words += batch.n;
        // one output mode for the launch: the most general one any batch needs (OUT_SCALAR < OUT_VEC4 < OUT_FLAT)
        mode = std::min(mode, outputMode(ctx->dim, batch.ld, batch.col_off, batch.out, 4, 0));
    }
    // (the finer index as for one batch of as many words: a serving loop's handful of small lookups is a small batch)
    TrainedPlan plan;
    const int planned = planTrained(ctx, floatRows(nullptr, words, nullptr, ctx->dim, 0), 0, true, false, &plan);
    if (planned != MEMB_HIP_OK) {
        return planned;
    }
    const uint32_t wordsPerWave = WAVE / (plan.fine ? ctx->fineLanes : ctx->lanesPerWord);
    BatchList list{};
    uint64_t tiles = 0;
    for (size_t k = 0; k < count; ++k) {
        const memb_hip_batch& batch = batches[k];
        list.firstTile[list.count] = tiles;
        list.rows[list.count] = batch.rows;
        list.out[list.count] = batch.out;
        list.n[list.count] = batch.n;
        list.ld[list.count] = batch.ld;
        list.colOff[list.count] = batch.col_off;
        ++list.count;
        tiles += (batch.n + wordsPerWave - 1) / wordsPerWave;
    }
    list.firstTile[list.count] = tiles;
    TrainedGeometry geometry = plan.geometry;
    geometry.mode = mode;
    if (!geometry.waves) {
        return fail(MEMB_HIP_ERR_INVALID, "decode tables and bitstream slots do not fit into LDS");
    }
    TrainedParams params = lookupParams(ctx, plan.fine);
    if (!lookupParamsConsistent(ctx, params, geometry)) {
        return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
    }
    uint32_t blocks = 0;
    const int code = oneTileBlocks(ctx, tiles, geometry.waves, &params, &blocks);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const hipError_t status = launchKernel(
        kernelTable().batches[lookupHasSub(ctx)][mode][ctx->fast].fn, dim3(blocks), dim3(geometry.waves * WAVE), geometry.ldsBytes,
        stream, params, list);
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("decode_trained_batches launch: ") + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// See memb_hip_decode_rows_union_device. MEMB_HIP_UNSUPPORTED when the models cannot share the kernel.
int launchTrainedUnion(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, const size_t* colOffs, size_t count, size_t n, float* out,
    size_t ld, hipStream_t stream, bool average)
{
    UnionPlan plan;
    const int planned = planUnion(ctxs, rows, colOffs, count, n, out, sizeof(float), ld, &plan);
    if (planned != MEMB_HIP_OK) {
        return planned;
    }
    const memb_hip_ctx* first = ctxs[0];
    UnionParams& params = plan.params;
    const bool hasSub = plan.hasSub;
    const bool allFast = plan.allFast;
    const uint32_t wordsPerWave = plan.wordsPerWave;
    const uint32_t sharedDwords = params.sharedDwords;
    const size_t tiles = (n + wordsPerWave - 1) / wordsPerWave;
    params.rowPieces = (average ? 1u : static_cast<uint32_t>(count)) * (first->dim / 4);
    params.rowMagic = magicFor(params.rowPieces, uint64_t(wordsPerWave) * params.rowPieces);
    auto layOut = [&] { layOutUnionWave(ctxs, count, wordsPerWave, &params); };
    auto chooseWaves = [&](const KernelInstance<UnionParams>& kernel, uint32_t sharedDwords, uint32_t perWaveDwords,
                           uint32_t* waves, uint32_t* ldsBytes) -> hipError_t {
        return chooseUnionWaves(first, reinterpret_cast<const void*>(kernel.fn), sharedDwords, perWaveDwords, waves, ldsBytes);
    };
    uint32_t waves = 0;
    uint32_t ldsBytes = 0;

    // decode_union_split: two models staged as row records -- the wavefront's word slots are divided
    // between the models, a tile is half as many words, LDS per wavefront as in the single-model kernel.
    // Against decode_trained_union (nibble keys, round 3 batch 32): 10 k words -20 %, 30 k -14 %, 100 k -10 %, 500 k -9 %.
    bool split = count == 2 && first->switches.unionSplit != 0 && wordsPerWave % 2 == 0 &&
        ((wordsPerWave / 2) * params.model[0].keyRowBytes) % 4 == 0;
    // the slots take the geometry of the model with the larger row regions; the other model's loads then run up to as
    // many pieces into the rows behind its own (its array ends with a guard of more than one region)
    const size_t larger = count == 2 && ctxs[1]->slotDwords > ctxs[0]->slotDwords ? 1 : 0;
    for (size_t m = 0; m < count && split; ++m) {
        split = ctxs[m]->recordPieces && ctxs[m]->recordPieces <= ctxs[larger]->recordPieces &&
            ctxs[larger]->recordPieces <= 2 * ctxs[m]->recordPieces &&
            wordsPerWave * (ctxs[larger]->slotDwords / 4) <= RECORD_ROUNDS * WAVE;
    }
    if (split) {
        UnionParams sp = params;
        uint32_t shared = sharedDwords;
        const bool packedSub = !allFast && hasSub;
        // nibble keys through the 4-byte tables (round 5: -2.5 % at 500 000 and 1 M words): half the table bytes in the block's LDS image
        const bool compact = allFast && ctxs[0]->table32 && ctxs[1]->table32 &&
            !ctxs[0]->byteTable.hasSubTables && !ctxs[1]->byteTable.hasSubTables;
        if (compact) {
            shared = 0;
            for (size_t m = 0; m < 2; ++m) {
                sp.model[m].table = ctxs[m]->table32;
                sp.model[m].tableDwords = packedTableDwords(ctxs[m]);
                sp.model[m].rootBits = ctxs[m]->byteTable.rootBits;
                sp.tableOffsetDwords[m] = shared;
                shared += sp.model[m].tableDwords;
            }
            sp.codebookOffsetDwords = shared;
            shared += 2 * 512;
            sp.sharedDwords = shared;
        }
        const uint32_t half = wordsPerWave / 2;
        sp.model[2] = sp.model[larger];
        sp.model[2].nRows = 0xFFFFFFFFu;   // (rows reach the decoder checked against their own model, or MISSING)
        sp.slotOffsetDwords[0] = 0;
        sp.keyTileOffsetDwords[0] = roundUp4(wordsPerWave * ctxs[larger]->slotDwords);
        sp.keyTileOffsetDwords[1] = sp.keyTileOffsetDwords[0] + half * sp.model[0].keyRowBytes / 4;
        sp.perWaveDwords = sp.keyTileOffsetDwords[0] + roundUp4(sp.model[0].keyTileDwords);
        const KernelInstance<UnionParams>& kernel = kernelTable().split[packedSub][allFast][average][compact];
        hipError_t status = chooseWaves(kernel, shared, sp.perWaveDwords, &waves, &ldsBytes);
        if (status != hipSuccess) {
            return fail(MEMB_HIP_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(status));
        }
        if (waves && (n + half - 1) / half / waves >= 0x7FFFFFFFull) {
            waves = 0;   // (more blocks than a grid holds: the forms below have tiles twice as large)
        }
        if (waves) {
            const size_t splitTiles = (n + half - 1) / half;
            sp.model[2].tilesPerWave = oneTileSteps(first, splitTiles, 4u * shared, true);
            const size_t perBlock = size_t(waves) * sp.model[2].tilesPerWave;
            status = launchKernel(
                kernel.fn, dim3(static_cast<uint32_t>((splitTiles + perBlock - 1) / perBlock)), dim3(waves * WAVE), ldsBytes, stream, sp);
            if (status != hipSuccess) {
                return fail(MEMB_HIP_ERR_DEVICE, std::string("decode_union_split launch: ") + hipGetErrorString(status));
            }
            ctxs[0]->unionKernel = kernel.name.c_str();
            return MEMB_HIP_OK;
        }
        // (does not fit: the forms below lay their areas out afresh)
    }
    // decode_trained_union, one tile per wavefront: three or four models, pairs without row records.
    // Its outputUnionTile keeps the words a nibble-key model lacks as one bit per (word, model) of a tile in ONE 64-bit mask:
    // a tile of more than 64 such pairs -- one lane per word (dim < 8), or three and four models at two or three lanes per
    // word -- does not fit (decode_union_split above has tiles of half as many words of two models: at most 64 pairs)
    if (allFast && uint64_t(wordsPerWave) * count > WAVE) {
        return fail(MEMB_HIP_UNSUPPORTED, "union kernel: nibble keys and more than 64 (word, model) pairs in a tile");
    }
    layOut();
    const KernelInstance<UnionParams>& kernel = kernelTable().unions[hasSub && !allFast][allFast][count][average];
    hipError_t status = chooseWaves(kernel, sharedDwords, params.perWaveDwords, &waves, &ldsBytes);
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(status));
    }
    if (!waves) {
        return fail(MEMB_HIP_UNSUPPORTED, "union kernel: tables and bitstream slots of the models do not fit into LDS together");
    }
    status = launchKernel(kernel.fn, dim3(static_cast<uint32_t>((tiles + waves - 1) / waves)), dim3(waves * WAVE), ldsBytes, stream, params);
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("decode_trained_union launch: ") + hipGetErrorString(status));
    }
    ctxs[0]->unionKernel = kernel.name.c_str();
    return MEMB_HIP_OK;
}

// The row-wise block kernels (dequant_uniform, gather_full and their narrow forms): `kernel` over n words, its one argument
// *params. No dynamic LDS, so nothing to configure: a plain launch. vec: the form of four values per thread and store.
template <typename Params>
int launchRowwise(const char* name, const void* kernel, size_t n, bool vec, uint32_t dim, Params* params, hipStream_t stream)
{
    if (vec) {
        params->pieceMagic = magicFor(dim / 4, uint64_t(params->wordsPerBlock) * (dim / 4));
    }
    const uint32_t blocks = static_cast<uint32_t>((n + params->wordsPerBlock - 1) / params->wordsPerBlock);
    void* arguments[] = {params};
    hipError_t status = kernel ? hipLaunchKernel(kernel, dim3(blocks), dim3(ROWWISE_THREADS), arguments, 0, stream)
                               : hipErrorInvalidDeviceFunction;
    if (status == hipSuccess) {
        status = hipGetLastError();
    }
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(name) + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

int launchUniform(memb_hip_ctx* ctx, const Lookup& lookup, hipStream_t stream)
{
    UniformParams params = rowwiseParams<UniformParams>(ctx, lookup);
    params.records = ctx->uniformRecords;
    params.regionPieces = ctx->regionPieces;
    params.levels = ctx->levels;
    const UniformTilePlan tilePlan = planUniform(ctx, lookup);
    if (tilePlan.tiled) {
        const uint32_t tileWords = tilePlan.tileWords, waves = tilePlan.waves;
        params.wordsPerWave = tileWords;
        params.regionMagic = magicFor(ctx->regionPieces, uint64_t(tileWords) * ctx->regionPieces + WAVE);
        params.pieceMagic = magicFor(ctx->dim / 4, uint64_t(tileWords) * (ctx->dim / 4));
        const uint32_t ldsBytes = waves * tileWords * ctx->regionPieces * 16;
        const uint64_t tiles = (lookup.n + tileWords - 1) / tileWords;
        const bool flat = lookup.ld == ctx->dim && lookup.colOff == 0;
        const hipError_t status = launchKernel(
            flat ? &dequant_uniform_tile<true> : &dequant_uniform_tile<false>, dim3(static_cast<uint32_t>((tiles + waves - 1) / waves)),
            dim3(waves * WAVE), ldsBytes, stream, params);
        if (status != hipSuccess) {
            return fail(MEMB_HIP_ERR_DEVICE, std::string("dequant_uniform_tile launch: ") + hipGetErrorString(status));
        }
        return MEMB_HIP_OK;
    }
    const bool vec = outputMode(ctx->dim, lookup.ld, lookup.colOff, lookup.out, lookup.elementBytes(), 0) != OUT_SCALAR;
    void (*const fp32Kernel)(UniformParams) = vec ? &dequant_uniform<true> : &dequant_uniform<false>;
    const bool narrow = lookup.outType != MEMB_HIP_OUT_F32;
    return launchRowwise(
        narrow ? "dequant_uniform_narrow" : "dequant_uniform",
        narrow ? memb_narrow::uniformKernel(vec, lookup.outType) : reinterpret_cast<const void*>(fp32Kernel), lookup.n, vec, ctx->dim,
        &params, stream);
}

int launchFull(memb_hip_ctx* ctx, const Lookup& lookup, hipStream_t stream)
{
    FullParams params = rowwiseParams<FullParams>(ctx, lookup);
    params.values = ctx->fullValues;
    const bool vec = outputMode(ctx->dim, lookup.ld, lookup.colOff, lookup.out, lookup.elementBytes(), 0) != OUT_SCALAR;
    void (*const fp32Kernel)(FullParams) = vec ? &gather_full<true> : &gather_full<false>;
    const bool narrow = lookup.outType != MEMB_HIP_OUT_F32;
    return launchRowwise(
        narrow ? "gather_full_narrow" : "gather_full",
        narrow ? memb_narrow::fullKernel(vec, lookup.outType) : reinterpret_cast<const void*>(fp32Kernel), lookup.n, vec, ctx->dim,
        &params, stream);
}

// Every decode of rows into device memory, whatever the storage and the element type, starts here.
int launch(memb_hip_ctx* ctx, const Lookup& lookup, hipStream_t stream)
{
    if (lookup.n == 0) {
        return MEMB_HIP_OK;
    }
    if (lookup.n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_ERR_INVALID, "batch too large");
    }
    switch (ctx->storage) {
        case memb::wire::Storage_Trained:
            return launchTrained(ctx, lookup, stream);
        case memb::wire::Storage_Uniform:
            return launchUniform(ctx, lookup, stream);
        case memb::wire::Storage_Full:
            return launchFull(ctx, lookup, stream);
        default:
            return fail(MEMB_HIP_ERR_INVALID, "context has no storage");
    }
}
