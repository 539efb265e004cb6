// Implementations of the entry points that are neither context creation (hip_staging.h), pooled lookups
// (hip_pooled_launch.h), the write side (hip_encoder.h) nor word lookups (hip_words.h): info and options, the
// decodes into device and host memory, sync, byte counts.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after every other
// host section (hip_host_path.h and hip_words.h among them); see that file for the overview.
#pragma once

int device_count_checked(int* count)
{
    if (!count) {
        return fail(MEMB_HIP_ERR_INVALID, "count is null");
    }
    *count = 0;
    hipError_t status = hipGetDeviceCount(count);
    if (status != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return fail(MEMB_HIP_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

int fillInfo(const memb_hip_ctx* ctx, memb_hip_ctx_info* info, uint64_t batchWords)
{
    std::memset(info, 0, sizeof(*info));
    info->device = ctx->device;
    info->storage = ctx->storage;
    info->dim = ctx->dim;
    info->n_rows = ctx->nRows;
    info->device_bytes = ctx->deviceBytes;
    info->word_index_bytes = ctx->wordIndexBytes;
    info->word_index_slots = ctx->wordSlots ? static_cast<uint32_t>(std::min<uint64_t>(uint64_t(ctx->wordSlotMask) + 1, 0xFFFFFFFFull)) : 0;   // (saturates: a table of 2^32 slots)
    info->word_index_keys = ctx->wordIndexKeys;
    if (ctx->storage == memb::wire::Storage_Trained) {
        const memb::DecodeTable& table = ctx->fast ? ctx->hostTable : ctx->byteTable;   // the lookup kernels' table
        info->root_bits = table.rootBits;
        info->max_code_bits = table.maxCodeBits;
        info->table_entries = static_cast<uint32_t>(table.entries.size());
        info->max_stream_bytes = ctx->maxStreamBytes;
        // the plan of a dense device-resident batch
        TrainedPlan plan;
        {
            DeviceScope deviceScope(ctx->device);
            HIP_TRY(deviceScope.status());
            const int planned = planTrained(
                ctx, floatRows(nullptr, batchWords ? size_t(batchWords) : size_t(1) << 30, nullptr, ctx->dim, 0), -1, true,
                rowsUnordered(ctx, false), &plan);
            if (planned != MEMB_HIP_OK) {
                return planned;
            }
        }
        const TrainedGeometry geometry = plan.geometry;
        info->waves_per_block = geometry.waves;
        std::snprintf(info->union_kernel, sizeof(info->union_kernel), "%s", ctx->unionKernel);
        info->kernel_registers = static_cast<uint32_t>(plan.numRegs);
        info->register_waves_per_cu = plan.persistent ? plan.registerWavesPerCu : 0;
        info->lanes_per_word = plan.fine ? ctx->fineLanes : ctx->lanesPerWord;
        info->segment_symbols = plan.fine ? ctx->fineSymbols : ctx->segmentSymbols;
        info->lds_bytes_per_block = geometry.ldsBytes;
        info->row_layout = ctx->recordPieces ? 2u : (ctx->rowMeta ? 1u : 0u);
        info->row_bytes = ctx->recordPieces * 16;
        // (the instance of dense fp32 rows, output mode 2)
        std::snprintf(info->kernel, sizeof(info->kernel), "%s", lookupKernel(ctx, plan.persistent, OUT_FLAT).name.c_str());
        if (!plan.persistent) {
            const uint32_t wordsPerWave = WAVE / info->lanes_per_word;
            const uint64_t words = batchWords ? batchWords : uint64_t(1) << 30;
            info->tiles_per_wavefront = oneTileSteps(
                ctx, (words + wordsPerWave - 1) / wordsPerWave,
                4u * ((ctx->fast ? ctx->tableDwords : packedTableDwords(ctx)) + codebookDwords(ctx)), false);
        }
    } else {
        // (a dense, aligned device-resident batch: what bench.py and the tests report for)
        const UniformTilePlan tilePlan = ctx->storage == memb::wire::Storage_Uniform ? planUniform(ctx, floatRows(nullptr, 0, nullptr, ctx->dim, 0)) : UniformTilePlan();
        const bool tiled = tilePlan.tiled;
        info->waves_per_block = tiled ? tilePlan.waves : ROWWISE_THREADS / WAVE;
        info->lds_bytes_per_block = tiled ? tilePlan.waves * tilePlan.tileWords * ctx->regionPieces * 16 : 0;
        std::snprintf(
            info->kernel, sizeof(info->kernel), "%s<true>",
            tiled ? "dequant_uniform_tile" : ctx->storage == memb::wire::Storage_Uniform ? "dequant_uniform" : "gather_full");
    }
    return MEMB_HIP_OK;
}

int ctx_get_info_checked(const memb_hip_ctx* ctx, memb_hip_ctx_info* info)
{
    if (!ctx || !info) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    // the caller's declaration of the struct may be shorter (or longer) than this library's
    const uint32_t callerSize = info->struct_size;
    if (callerSize < sizeof(uint32_t) || callerSize > 4096) {
        return fail(MEMB_HIP_ERR_INVALID, "memb_hip_ctx_info.struct_size must be set to sizeof(memb_hip_ctx_info)");
    }
    // ABI 4 declared union_kernel 8 bytes lower than ABI 3 and ABI 5 do (two dwords fewer in front of it): a client
    // built against that header would read the kernel name out of step. Its size gives it away.
    if (callerSize == offsetof(memb_hip_ctx_info, word_index_bytes) - 8) {
        return fail(MEMB_HIP_ERR_INVALID, "memb_hip_ctx_info: this is the ABI-4 layout; rebuild against include/memb_hip.h of ABI 5");
    }
    memb_hip_ctx_info filled;
    uint64_t batchWords = 0;
    if (callerSize >= offsetof(memb_hip_ctx_info, batch_words) + sizeof(uint64_t)) {
        batchWords = info->batch_words;
    }
    const int code = fillInfo(ctx, &filled, batchWords);
    filled.batch_words = batchWords;
    if (code != MEMB_HIP_OK) {
        return code;
    }
    const uint32_t bytes = std::min<uint32_t>(callerSize, sizeof(filled));
    filled.struct_size = bytes;
    std::memcpy(info, &filled, bytes);
    return MEMB_HIP_OK;
}

int option_set_checked(memb_hip_ctx* ctx, const char* name, uint64_t value)
{
    if (!ctx || !name) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    const std::string key(name);
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (key == "waves_per_block" && value <= 16) {
        ctx->switches.waves = static_cast<uint32_t>(value);
    } else if (key == "tiles_per_wave" && value <= 64) {
        ctx->switches.tilesPerWave = static_cast<uint32_t>(value);
    } else if (key == "fine_lanes" && value <= 2) {
        ctx->switches.fineLanes = static_cast<uint32_t>(value);
    } else if (key == "union_fused" && value <= 1) {
        ctx->switches.unionFused = static_cast<uint32_t>(value);
    } else if (key == "union_split" && value <= 1) {
        ctx->switches.unionSplit = static_cast<uint32_t>(value);
    } else if (key == "persistent" && value <= 2) {
        ctx->switches.persistent = static_cast<uint32_t>(value);
    } else if (key == "host_expand" && value <= 1) {
        ctx->switches.hostExpand = value != 0;
#ifdef MEMB_HIP_MEASURE
    } else if (key == "debug" && value <= 0xFFFFFFFFull) {
        ctx->switches.debugFlags = static_cast<uint32_t>(value);
    } else if (key == "lds_pad" && value <= 128 * 1024) {
        ctx->switches.ldsPad = static_cast<uint32_t>(value);
#endif
    } else {
        return fail(MEMB_HIP_ERR_INVALID, "unknown option or value out of range: " + key);
    }
    return MEMB_HIP_OK;
}

// (memb_hip_decode_rows_device: no flags, no divisor)
int decode_rows_device_ex_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, void* stream,
    uint32_t flags, float divisor)
{
    if (!ctx || (n && (!rows || !out))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    if (ld < col_off + ctx->dim) {
        return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
    }
    if ((flags & ~uint32_t(MEMB_HIP_ACCUMULATE | MEMB_HIP_ROWS_IN_RANDOM_ORDER)) || !(divisor == divisor)) {
        return fail(MEMB_HIP_ERR_INVALID, "unknown flags or NaN divisor");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    Lookup lookup = floatRows(rows, n, out, ld, col_off);
    lookup.accumulate = (flags & MEMB_HIP_ACCUMULATE) ? 1u : 0u;
    lookup.divisor = divisor;
    lookup.randomOrder = (flags & MEMB_HIP_ROWS_IN_RANDOM_ORDER) != 0;
    return launch(ctx, lookup, static_cast<hipStream_t>(stream));
}

int decode_rows_device_typed_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, void* out, int outType, size_t ld, size_t col_off, void* stream)
{
    if (outType != MEMB_HIP_OUT_F32 && outType != MEMB_HIP_OUT_BF16 && outType != MEMB_HIP_OUT_F16) {
        return fail(MEMB_HIP_ERR_INVALID, "unknown out_type " + std::to_string(outType));
    }
    if (!ctx || (n && (!rows || !out))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    const size_t elementBytes = outType == MEMB_HIP_OUT_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(out) % elementBytes != 0) {
        return fail(MEMB_HIP_ERR_INVALID, "out must be aligned to its element (" + std::to_string(elementBytes) + " bytes)");
    }
    if (col_off > ld || ld - col_off < ctx->dim) {
        return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    return launch(ctx, Lookup{rows, n, out, outType, ld, col_off}, static_cast<hipStream_t>(stream));
}

int decode_batches_device_checked(memb_hip_ctx* ctx, const memb_hip_batch* batches, size_t count, void* stream)
{
    if (!ctx || (count && !batches)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    std::vector<memb_hip_batch> live;   // (empty batches take no part)
    for (size_t k = 0; k < count; ++k) {
        const memb_hip_batch& batch = batches[k];
        if (batch.n && (!batch.rows || !batch.out)) {
            return fail(MEMB_HIP_ERR_INVALID, "null argument");
        }
        if (batch.ld < batch.col_off + ctx->dim) {
            return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
        }
        if (batch.n > (size_t(1) << 37)) {
            return fail(MEMB_HIP_ERR_INVALID, "batch too large");
        }
        if (batch.n) {
            live.push_back(batch);
        }
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    if (ctx->storage != memb::wire::Storage_Trained || live.size() == 1) {
        // uniform / full: their kernels have no shared prologue worth one launch; a single batch: the plain call
        for (const memb_hip_batch& batch : live) {
            const int code = launch(ctx, floatRows(batch.rows, batch.n, batch.out, batch.ld, batch.col_off), static_cast<hipStream_t>(stream));
            if (code != MEMB_HIP_OK) {
                return code;
            }
        }
        return MEMB_HIP_OK;
    }
    for (size_t first = 0; first < live.size(); first += MAX_BATCHES) {
        const int code = launchTrainedBatches(
            ctx, live.data() + first, std::min<size_t>(MAX_BATCHES, live.size() - first), static_cast<hipStream_t>(stream));
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_decode_rows (host row ids in `rows`) and memb_hip_decode_words (`batch`: the row ids are looked up on the
// device and fetched into pinned memory for the host threads that zero the rows of unknown words).
int decode_rows_checked(
    memb_hip_ctx* ctx, const uint32_t* rows, size_t n, float* out, size_t ld, size_t col_off, const memb_hip_words* batch = nullptr)
{
    if (batch) {
        n = wordBatchCount(batch);
    }
    if (!ctx || (n && ((!rows && !batch) || !out))) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    if (ld < col_off + ctx->dim) {
        return fail(MEMB_HIP_ERR_INVALID, "ld must be at least col_off + dim");
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->mutex);
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());

    // Small batches (single words above all): two tiny copies cost more than the
    // decode. Row ids and results go through one pinned, device-mapped host
    // buffer instead: the kernel reads the ids from it and writes the rows into it
    // over PCIe, the host then copies them to the caller's (possibly strided) rows.
    constexpr size_t SMALL_WORDS = 512;
    const size_t rowBytes = size_t(ctx->dim) * sizeof(float);
    // (at most 2 MiB of rows that way: very wide rows leave the small path after fewer words)
    const size_t smallWords = std::min<size_t>(SMALL_WORDS, (size_t(2) << 20) / rowBytes);
    if (n <= smallWords && !ctx->smallUnavailable && !batch) {
        // row ids first, rows from the next 256-byte boundary
        constexpr size_t outOffset = (SMALL_WORDS * sizeof(uint32_t) + 255) / 256 * 256;
        if (!ctx->smallHost) {
            void* host = nullptr;
            void* device = nullptr;
            if (hipHostMalloc(&host, outOffset + smallWords * rowBytes, hipHostMallocMapped) == hipSuccess &&
                hipHostGetDevicePointer(&device, host, 0) == hipSuccess) {
                ctx->smallHost = host;
                ctx->smallDevice = device;
            } else {
                (void)hipGetLastError();
                if (host) {
                    (void)hipHostFree(host);
                }
                ctx->smallUnavailable = true;
            }
        }
        if (ctx->smallHost) {
            std::memcpy(ctx->smallHost, rows, n * sizeof(uint32_t));
            float* deviceOut = reinterpret_cast<float*>(static_cast<char*>(ctx->smallDevice) + outOffset);
            int code = launch(ctx, floatRows(static_cast<const uint32_t*>(ctx->smallDevice), n, deviceOut, ctx->dim, 0), ctx->stream);
            if (code != MEMB_HIP_OK) {
                return code;
            }
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            const char* hostOut = static_cast<const char*>(ctx->smallHost) + outOffset;
            for (size_t i = 0; i < n; ++i) {
                std::memcpy(out + i * ld + col_off, hostOut + i * rowBytes, rowBytes);
            }
            return MEMB_HIP_OK;
        }
    }

    // Device staging holds one row per word -- fp32, or centroid indices for trained
    // storages (decodeRowsAsKeys) -- ; batches larger than the staging area (4 GiB of
    // fp32 rows) are processed in slices.
    const size_t dim = ctx->dim;
    const bool asKeys = ctx->storage == memb::wire::Storage_Trained && !ctx->hostCodebook.empty() &&
        keyRowBytes(ctx) <= RING_CHUNK_BYTES && ctx->switches.hostExpand && ensureRing(ctx);
    const size_t stagedRowBytes = asKeys ? keyRowBytes(ctx) : dim * sizeof(float);
    const size_t sliceLimit = std::min<size_t>((size_t(4) << 30) / (dim * sizeof(float)), ctx->switches.sliceWords);
    const size_t sliceWords = std::max<size_t>(1, std::min<size_t>(n, sliceLimit));
    if (batch && sliceWords < n) {
        return fail(MEMB_HIP_UNSUPPORTED, "a word batch of this size is decoded in slices: look the words up first and pass row ids");
    }
    if (batch && ctx->hostRowsCapacity < n) {
        if (ctx->hostRowsPinned) {
            (void)hipHostFree(ctx->hostRowsPinned);
            ctx->hostRowsPinned = nullptr;
            ctx->hostRowsCapacity = 0;
        }
        void* pinned = nullptr;
        HIP_TRY(hipHostMalloc(&pinned, (n + n / 4) * sizeof(uint32_t), hipHostMallocDefault));
        ctx->hostRowsPinned = static_cast<uint32_t*>(pinned);
        ctx->hostRowsCapacity = n + n / 4;
    }
    if (ctx->stagedCapacity < sliceWords || ctx->stagedRowBytes < stagedRowBytes) {
        if (ctx->stagedRows) {
            (void)hipFree(ctx->stagedRows);
            ctx->stagedRows = nullptr;
        }
        if (ctx->stagedOut) {
            (void)hipFree(ctx->stagedOut);
            ctx->stagedOut = nullptr;
        }
        ctx->stagedCapacity = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->stagedRows), sliceWords * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->stagedOut), sliceWords * stagedRowBytes + 16));
        ctx->stagedCapacity = sliceWords;
        ctx->stagedRowBytes = stagedRowBytes;
    }
    const bool verbose = ctx->switches.verbose;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    int result = MEMB_HIP_OK;
    for (size_t start = 0; start < n && result == MEMB_HIP_OK; start += sliceWords) {
        const size_t words = std::min(sliceWords, n - start);
        hipError_t status;
        if (batch) {
            // word -> row on the device, straight into the staging array; the ids also go to pinned host memory, for the
            // threads that expand the result (an unknown word's row is zeroed there). Every copy of result chunks is
            // enqueued behind this one, so the ids have landed when the first chunk's event fires.
            result = resolveBatchOnContextStream(ctx, batch, ctx->stagedRows);
            if (result != MEMB_HIP_OK) {
                break;
            }
            status = hipMemcpyAsync(ctx->hostRowsPinned, ctx->stagedRows, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
            rows = ctx->hostRowsPinned;
        } else {
            status = hipMemcpyAsync(ctx->stagedRows, rows + start, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        }
        if (status != hipSuccess) {
            result = fail(MEMB_HIP_ERR_DEVICE, std::string("row id copy: ") + hipGetErrorString(status));
            break;
        }
        float* destination = out + start * ld + col_off;
        if (asKeys) {
            result = decodeRowsAsKeys(
                ctx, ctx->stagedRows, rows + start, words, reinterpret_cast<uint8_t*>(ctx->stagedOut), destination, ld);
        } else {
            result = launch(ctx, floatRows(ctx->stagedRows, words, ctx->stagedOut, dim, 0), ctx->stream);
            if (result == MEMB_HIP_OK) {
                result = copyRowsToHost(ctx, ctx->stagedOut, words, destination, ld);
            }
        }
    }
    if (result != MEMB_HIP_OK) {
        (void)hipStreamSynchronize(ctx->stream);   // nothing of this call may still be running when the caller's buffers go away
    }
    // a full-vocabulary dump should not keep gigabytes of HBM for the next small batch
    if (ctx->stagedCapacity * ctx->stagedRowBytes > (size_t(1) << 30)) {
        (void)hipFree(ctx->stagedRows);
        (void)hipFree(ctx->stagedOut);
        ctx->stagedRows = nullptr;
        ctx->stagedOut = nullptr;
        ctx->stagedCapacity = 0;
        ctx->stagedRowBytes = 0;
    }
    if (verbose) {
        std::fprintf(stderr, "memb_hip: decode_rows n=%zu (%s over PCIe) rows + kernel + copy %.4fs\n",
                     n, asKeys ? "centroid indices" : "fp32 rows", now() - t0);
    }
    return result;
}

int decode_rows_union_device_checked(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, const size_t* col_offs, size_t count, size_t n, float* out,
    size_t ld, void* stream, uint32_t flags)
{
    if (flags & ~uint32_t(MEMB_HIP_UNION_AVERAGE)) {
        return fail(MEMB_HIP_ERR_INVALID, "unknown flags");
    }
    if (!ctxs || !rows || !col_offs || count == 0 || (n && !out)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    for (size_t m = 0; m < count; ++m) {
        if (!ctxs[m] || (n && !rows[m])) {
            return fail(MEMB_HIP_ERR_INVALID, "null argument");
        }
    }
    if (n == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(ctxs[0]->device);
    HIP_TRY(deviceScope.status());
    return launchTrainedUnion(
        ctxs, rows, col_offs, count, n, out, ld, static_cast<hipStream_t>(stream), (flags & MEMB_HIP_UNION_AVERAGE) != 0);
}

int sync_checked(memb_hip_ctx* ctx)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEMB_HIP_OK;
}

int algorithmic_bytes_checked(const memb_hip_ctx* ctx, const uint32_t* rows, size_t n, uint64_t* bytes)
{
    if (!ctx || !bytes || (n && !rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    uint64_t total = 0;
    const uint64_t rowBytes = 4ull * ctx->dim;
    for (size_t i = 0; i < n; ++i) {
        total += 4 + rowBytes;
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
                total += 4 + rowBytes;
                break;
            default:
                break;
        }
    }
    *bytes = total;
    return MEMB_HIP_OK;
}
