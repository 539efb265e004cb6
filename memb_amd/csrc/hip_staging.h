// Staging of a model to HBM: the steps of a trained storage (tables, stream lengths, re-packed bitstreams,
// lanes per word, segment index) and the three context constructors.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the plans
// (hip_decode_plan.h), which size the tables; see that file for the overview.
#pragma once

// One pass over every row with one lane per word: records the bit position at
// which each segment of each row starts (segmentIndex), so that lanesPerWord
// lanes can later decode a row side by side.
// (lanes, symbols, target: the index to build -- the context's own, or the finer one of small batches)
int buildSegmentIndex(memb_hip_ctx* ctx, uint32_t lanes, uint32_t symbols, uint16_t* target)
{
    if (lanes <= 1 || ctx->nRows == 0) {
        return MEMB_HIP_OK;
    }
    TrainedParams params = baseTrainedParams(ctx);
    params.segmentIndex = nullptr;
    params.segmentIndexOut = target;
    params.rows = nullptr;
    params.n = ctx->nRows;
    params.lanesPerWord = 1;
    params.laneMagic = 0;
    params.segmentSymbols = (ctx->dim + 7) / 8 * 8;
    params.keyRowBytes = 0;
    params.keyTileDwords = 0;
    params.indexLanes = lanes;
    params.indexSegmentSymbols = symbols;

    // one lane per word, normally 64 words per wavefront; fewer (the other lanes idle) when
    // 64 bitstream slots are more than LDS holds
    uint32_t wordsPerWave = WAVE;
    while (wordsPerWave > 1 && trainedLdsBytes(ctx, 1, wordsPerWave, false) > ctx->ldsLimit) {
        wordsPerWave /= 2;
    }
    uint32_t waves = 4;
    while (waves > 1 && trainedLdsBytes(ctx, waves, wordsPerWave, false) > ctx->ldsLimit) {
        waves /= 2;
    }
    const uint32_t ldsBytes = trainedLdsBytes(ctx, waves, wordsPerWave, false);
    if (ldsBytes > ctx->ldsLimit) {
        return fail(MEMB_HIP_ERR_INVALID, "a row's bitstream does not fit into LDS");
    }
    params.wordsPerWave = wordsPerWave;
    const size_t tiles = (ctx->nRows + wordsPerWave - 1) / wordsPerWave;
    const uint32_t blocks = static_cast<uint32_t>((tiles + waves - 1) / waves);
    // (the index pass reads the 8-byte table)
    const KernelInstance<TrainedParams>& kernel = kernelTable().trained[ctx->hostTable.hasSubTables && !ctx->fast][OUT_INDEX][ctx->fast];
    hipError_t status = launchKernel(kernel.fn, dim3(blocks), dim3(waves * WAVE), ldsBytes, ctx->stream, params);
    if (status == hipSuccess) {
        status = hipStreamSynchronize(ctx->stream);
    }
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("segment index build: ") + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// ---- staging of a trained storage, step by step (memb_hip_ctx_create_trained) ----

// Code lengths -> two-level lookup table (host form).
int buildHostTable(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    try {
        auto lengths = memb::codeLengthsFromSizeOffsets(
            desc->keys, desc->n_keys, desc->size_offsets, desc->n_size_offsets);
        for (const auto& info : lengths) {
            if (info.key >= desc->n_centroids) {
                throw std::runtime_error("Huffman symbol without a centroid");
            }
        }
        // First-level width: a hint (results never depend on it). With long codes a narrow first
        // level makes the second-level tables large -- 2^(longest code - width) entries each --
        // so the width is raised until the whole table takes at most 64 KiB of the 160 KiB of LDS,
        // which leaves room for the bitstream slots of at least a few wavefronts.
        uint32_t limit = desc->max_direct_bits ? desc->max_direct_bits : envUint("MEMB_HIP_ROOT_BITS", 11);
        limit = std::max<uint32_t>(1, std::min<uint32_t>(limit, 12));
        for (;;) {
            ctx->hostTable = memb::buildDecodeTable(lengths, limit);
            if (ctx->hostTable.entries.size() * 8 <= 64 * 1024 || limit >= 12) {
                break;
            }
            ++limit;
        }
        // The byte-key kernels' table. What costs there is the second-level lookup, not the size of
        // the first level: a branch and a second dependent LDS round trip per symbol as soon as one
        // lane of the wavefront needs it (6-bit GloVe-shaped model, codes up to 10 bits: 0.71 ms with
        // an 8-bit first level, 0.61 ms with a 10-bit one; 8-bit model, codes up to 13 bits: 0.74 /
        // 0.72 / 0.68 ms with 11 / 12 / 13 bits). So the first level covers the longest code
        // whenever 32 KiB of 4-byte entries hold it (13 bits); a given max_direct_bits is still
        // honoured (tests force the two-level path with it), raised only while the tables would not fit.
        ctx->codeLengths = lengths;
        uint32_t byteLimit = desc->max_direct_bits ? desc->max_direct_bits : 13u;
        byteLimit = std::max<uint32_t>(1, std::min<uint32_t>(byteLimit, 13));
        for (;;) {
            ctx->byteTable = memb::buildDecodeTable(lengths, byteLimit);
            if (ctx->byteTable.entries.size() * 4 <= 48 * 1024 || byteLimit >= 13) {
                break;
            }
            ++byteLimit;
        }
    } catch (const std::exception& error) {
        return fail(MEMB_HIP_ERR_INVALID, error.what());
    }

    return MEMB_HIP_OK;
}

// Per-row stream length: streams are laid out back to back, so a stream ends where the
// next one (in storage order) begins. Sets ctx->streamBytes and ctx->maxStreamBytes.
int measureStreams(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    // Every start is marked in a bitmap over the byte positions; each row then scans forward
    // to the next mark. Both passes run on a few host threads.
    {
        for (uint64_t r = 0; r < desc->n_rows; ++r) {
            if (desc->value_offsets[r] > desc->packed_values_bytes) {
                        return fail(MEMB_HIP_ERR_INVALID, "value offset beyond packed values");
            }
        }
        const uint64_t totalBytes = desc->packed_values_bytes;
        const size_t bitmapWords = static_cast<size_t>(totalBytes / 64 + 2);
        std::vector<std::atomic<uint64_t>> marks(bitmapWords);
        for (auto& word : marks) {
            word.store(0, std::memory_order_relaxed);
        }
        marks[totalBytes / 64].fetch_or(uint64_t(1) << (totalBytes % 64), std::memory_order_relaxed);   // end sentinel
        const uint64_t bound =
            (static_cast<uint64_t>(desc->dim) * std::max<uint32_t>(ctx->hostTable.maxCodeBits, 1) + 7) / 8;
        ctx->streamBytes.assign(desc->n_rows, 0);
        const size_t threads = std::max<size_t>(1, std::min<size_t>({std::thread::hardware_concurrency(), size_t(16), size_t(desc->n_rows / 65536 + 1)}));
        const uint64_t perThread = (desc->n_rows + threads - 1) / threads;
        auto parallel = [&](auto body) {
            std::vector<std::thread> pool;
            for (size_t t = 1; t < threads; ++t) {
                pool.emplace_back(body, t * perThread, std::min<uint64_t>(desc->n_rows, (t + 1) * perThread));
            }
            body(uint64_t(0), std::min<uint64_t>(desc->n_rows, perThread));
            for (auto& thread : pool) {
                thread.join();
            }
        };
        parallel([&](uint64_t first, uint64_t last) {
            for (uint64_t r = first; r < last; ++r) {
                const uint64_t offset = desc->value_offsets[r];
                marks[offset / 64].fetch_or(uint64_t(1) << (offset % 64), std::memory_order_relaxed);
            }
        });
        std::vector<uint32_t> threadMax(threads, 0);
        parallel([&](uint64_t first, uint64_t last) {
            uint32_t longest = 0;
            for (uint64_t r = first; r < last; ++r) {
                const uint64_t offset = desc->value_offsets[r];
                uint64_t bytes = 0;
                if (offset < totalBytes) {
                    // next mark strictly after `offset` (a stream never holds more than dim codes of the longest length)
                    uint64_t position = offset + 1;
                    size_t word = position / 64;
                    uint64_t bits = marks[word].load(std::memory_order_relaxed) & (~uint64_t(0) << (position % 64));
                    while (!bits && (word + 1) * 64 <= offset + bound + 64) {
                        bits = marks[++word].load(std::memory_order_relaxed);
                    }
                    const uint64_t next = bits ? word * 64 + static_cast<uint64_t>(__builtin_ctzll(bits)) : offset + bound;
                    bytes = std::min(next - offset, bound);
                }
                ctx->streamBytes[r] = static_cast<uint32_t>(bytes);
                longest = std::max(longest, ctx->streamBytes[r]);
            }
            threadMax[first / std::max<uint64_t>(perThread, 1)] = longest;
        });
        ctx->maxStreamBytes = *std::max_element(threadMax.begin(), threadMax.end());
    }
    return MEMB_HIP_OK;
}

// Re-packed layout on the device: streamStarts, then the bitstreams themselves (repack_streams).
int stageStreams(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    // Row records (TrainedParams::recordPieces) where the model allows: at most 8 lanes per word and
    // streams below 1 KiB (the record's 13-bit offsets), and rows of similar length (the regions may take
    // 35 % more than the compact layout; the 2-bit model, rows of 1..3 bits per weight, needs 33 % and
    // still gains 1 % on the key-order dump and 3 % on shuffled rows) -- every row then
    // owns 16 + the longest stream bytes, rounded up to 32 so that a row never touches a third line.
    // Otherwise (or with MEMB_HIP_ROW_RECORDS=0) the compact layout: row r's stream occupies
    // ceil(bytes / 16) pieces from streamStarts[r], offsets in rowMeta or the two arrays.
    std::vector<uint32_t> streamStarts(desc->n_rows + 1, 0);
    uint64_t compactPieces = 0;
    for (uint64_t r = 0; r < desc->n_rows; ++r) {
        compactPieces += (ctx->streamBytes[r] + 15) / 16;
    }
    const uint32_t recordPieces = ((16 + ctx->maxStreamBytes + 31) / 32) * 2;
    ctx->recordPieces = 0;
    if (desc->n_rows && ctx->lanesPerWord > 1 && ctx->lanesPerWord <= ROW_META_MAX_LANES &&
        uint64_t(ctx->maxStreamBytes) * 8 + 64 < (1u << ROW_META_BITS) && envUint("MEMB_HIP_ROW_RECORDS", 1) &&
        envUint("MEMB_HIP_ROW_META", 1) && ctx->slotDwords >= 4 * recordPieces + 3 &&
        uint64_t(recordPieces) * desc->n_rows * 100 <=
            (compactPieces + desc->n_rows) * (100 + 35) &&   // at most 35 % padding
        uint64_t(recordPieces) * (desc->n_rows + 2) < (1ull << 32)) {
        ctx->recordPieces = recordPieces;
    } else {
        // compact layout: the slot holds the stream and the decoder's last window only (no record, no
        // rounding to 32), so lookups copy two pieces per word less and the wavefronts need less LDS
        ctx->slotDwords = compactSlotDwords(ctx->maxStreamBytes);
    }
    {
        uint64_t next = 0;
        for (uint64_t r = 0; r < desc->n_rows; ++r) {
            if (ctx->recordPieces) {
                streamStarts[r] = static_cast<uint32_t>(r * ctx->recordPieces + 1);   // the stream follows the record
                continue;
            }
            streamStarts[r] = static_cast<uint32_t>(next);
            next += (ctx->streamBytes[r] + 15) / 16;
        }
        if (ctx->recordPieces) {
            next = uint64_t(ctx->recordPieces) * desc->n_rows;
        }
        if (next + ctx->slotDwords / 4 + 1 >= (1ull << 32)) {
                return fail(MEMB_HIP_ERR_INVALID, "bitstreams too large");
        }
        streamStarts[desc->n_rows] = static_cast<uint32_t>(next);
    }
    const size_t streamPieces = size_t(streamStarts[desc->n_rows]) + ctx->slotDwords / 4 + 1;   // + guard of one slot

    // (Where the array lies does not matter: round 3 placed it at 1 GiB and 2 MiB alignments with 64 MiB / 4 KiB / 256 B
    // offsets, all within 0.25 % -- profiles/r03_aa_control.txt; the switches for that experiment are gone.)
    int code = deviceAlloc(ctx, &ctx->streams, streamPieces * 16);
    if (ctx->switches.verbose) {
        std::fprintf(stderr, "memb_hip: stream array at %p, %zu bytes\n", static_cast<void*>(ctx->streams), streamPieces * 16);
    }
    uint8_t* filePacked = nullptr;      // temporary device copies of the file's arrays
    uint32_t* fileOffsets = nullptr;
    if (code == MEMB_HIP_OK) {
        hipError_t status = hipMemset(ctx->streams, 0, streamPieces * 16);
        if (status != hipSuccess) {
            code = fail(MEMB_HIP_ERR_DEVICE, std::string("hipMemset: ") + hipGetErrorString(status));
        }
    }
    if (code == MEMB_HIP_OK) {
        code = deviceAlloc(ctx, &ctx->streamStarts, streamStarts.size() * 4);
    }
    if (code == MEMB_HIP_OK) {
        code = copyToDevice(ctx->streamStarts, streamStarts.data(), streamStarts.size() * 4);
    }
    if (code == MEMB_HIP_OK && desc->n_rows) {
        hipError_t status = hipMalloc(reinterpret_cast<void**>(&filePacked), std::max<size_t>(desc->packed_values_bytes, 16));
        if (status == hipSuccess) {
            status = hipMalloc(reinterpret_cast<void**>(&fileOffsets), desc->n_rows * 4);
        }
        if (status != hipSuccess) {
            code = fail(MEMB_HIP_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(status));
        }
        if (code == MEMB_HIP_OK) {
            code = copyToDevice(filePacked, desc->packed_values, desc->packed_values_bytes);
        }
        if (code == MEMB_HIP_OK) {
            code = copyToDevice(fileOffsets, desc->value_offsets, desc->n_rows * 4);
        }
        if (code == MEMB_HIP_OK) {
            const uint32_t threads = 256;
            const uint64_t blocks = (desc->n_rows * WAVE + threads - 1) / threads;
            hipLaunchKernelGGL(
                repack_streams, dim3(static_cast<uint32_t>(blocks)), dim3(threads), 0, ctx->stream, filePacked,
                desc->packed_values_bytes, fileOffsets, ctx->streamStarts, desc->n_rows, ctx->streams, ctx->recordPieces);
            hipError_t launched = hipGetLastError();
            if (launched == hipSuccess) {
                launched = hipStreamSynchronize(ctx->stream);
            }
            if (launched != hipSuccess) {
                code = fail(MEMB_HIP_ERR_DEVICE, std::string("repack_streams: ") + hipGetErrorString(launched));
            }
        }
        if (filePacked) {
            (void)hipFree(filePacked);
        }
        if (fileOffsets) {
            (void)hipFree(fileOffsets);
        }
    }
    return code;
}

// Lanes per word (G), symbols per lane (S) and the width of the segment index.
void chooseLanes(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    // MEMB_HIP_LANES (default 8, the measured
    // optimum for 300-dimensional rows) or, for rows so long that a wavefront's 64 / G
    // bitstream slots and symbol rows would not fit into LDS, the next power of two that does;
    // rows of fewer than 8 weights are not split.
    uint32_t lanes = std::max<uint32_t>(1, std::min<uint32_t>(envUint("MEMB_HIP_LANES", 8), WAVE));
    if (desc->dim < 8) {
        lanes = 1;
    }
    const uint32_t group = ctx->fast ? 8 : 4;
    // (byte keys: a first level wider than 11 bits is a luxury -- it goes first when LDS is short)
    auto narrowTable = [ctx] {
        if (ctx->fast || ctx->byteTable.rootBits <= 11) {
            return false;
        }
        ctx->byteTable = memb::buildDecodeTable(ctx->codeLengths, ctx->byteTable.rootBits - 1);
        return true;
    };
    for (;;) {
        ctx->segmentSymbols = std::max<uint32_t>(group, ((desc->dim + lanes - 1) / lanes + group - 1) / group * group);
        ctx->lanesPerWord = (desc->dim + ctx->segmentSymbols - 1) / ctx->segmentSymbols;
        if (lanes >= WAVE || trainedLdsBytes(ctx, 1, WAVE / ctx->lanesPerWord, true) <= ctx->ldsLimit) {
            break;
        }
        if (narrowTable()) {
            continue;
        }
        lanes = std::min<uint32_t>(WAVE, lanes < 8 ? 8 : 2 * lanes);
    }
    // a forced block size (MEMB_HIP_WAVES, tests) may still need the room
    while (!chooseGeometry(ctx, WAVE / ctx->lanesPerWord, 4).waves && narrowTable()) {
    }
    ctx->indexWide = uint64_t(ctx->maxStreamBytes) * 8 + 64 >= 65536;
}

// Lookup table and codebook in their device forms.
int stageTables(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    int code = MEMB_HIP_OK;
    if (code == MEMB_HIP_OK) {
        code = deviceAlloc(ctx, &ctx->table, size_t(ctx->tableDwords) * 4);
    }
    if (code == MEMB_HIP_OK) {
        // device form of the table: {length or pointer, symbol replicated per byte / nibble}
        std::vector<uint32_t> expanded(ctx->tableDwords, 0);
        for (size_t i = 0; i < ctx->hostTable.entries.size(); ++i) {
            const uint32_t entry = ctx->hostTable.entries[i];
            if (entry & memb::TABLE_POINTER_FLAG) {
                expanded[2 * i] = entry;
            } else {
                const uint32_t key = (entry >> 8) & 0xff;
                expanded[2 * i] = entry & 0xff;
                expanded[2 * i + 1] = ctx->fast ? key * 0x11111111u : key * 0x01010101u;
            }
        }
        code = copyToDevice(ctx->table, expanded.data(), expanded.size() * 4);
    }
    if (code == MEMB_HIP_OK) {
        // (setUpLds copies whole 16-byte pieces: the device copy is padded to packedTableDwords like the LDS image;
        // nibble-key models have it too: decode_union_split decodes them through it beside a byte-key partner)
        std::vector<uint32_t> padded(ctx->byteTable.entries);
        padded.resize(packedTableDwords(ctx), 0);
        code = deviceAlloc(ctx, &ctx->table32, padded.size() * 4);
        if (code == MEMB_HIP_OK) {
            code = copyToDevice(ctx->table32, padded.data(), padded.size() * 4);
        }
    }
    if (code == MEMB_HIP_OK) {
        code = deviceAlloc(ctx, &ctx->codebook, 512 * 4);
    }
    if (code == MEMB_HIP_OK) {
        std::vector<float> centroids(256, 0.f);
        std::copy(desc->centroids, desc->centroids + desc->n_centroids, centroids.begin());
        centroids[ZERO_KEY] = 0.f;
        std::vector<float> codebook(512, 0.f);
        if (ctx->fast) {
            // pair b = {centroid[low nibble], centroid[high nibble]}: two symbols per LDS read
            for (uint32_t b = 0; b < 256; ++b) {
                codebook[2 * b] = centroids[b & 15];
                codebook[2 * b + 1] = centroids[b >> 4];
            }
        } else {
            std::copy(centroids.begin(), centroids.end(), codebook.begin());
        }
        code = copyToDevice(ctx->codebook, codebook.data(), 512 * 4);
        ctx->hostCodebook = codebook;
        if (code == MEMB_HIP_OK && ctx->fast) {
            // the byte-key form of the codebook (see memb_hip_ctx::codebookBytes): 1 KiB
            code = deviceAlloc(ctx, &ctx->codebookBytes, 256 * 4);
            if (code == MEMB_HIP_OK) {
                code = copyToDevice(ctx->codebookBytes, centroids.data(), 256 * 4);
            }
        }
    }
    return code;
}

// Segment index (one decode pass over every row) and the rowMeta records packed from it.
int stageIndex(memb_hip_ctx* ctx, const memb_hip_trained_desc* desc)
{
    int code = MEMB_HIP_OK;
    if (code == MEMB_HIP_OK) {
        TrainedGeometry geometry = chooseGeometry(ctx, WAVE / ctx->lanesPerWord, 4);
        if (!geometry.waves) {
            code = fail(MEMB_HIP_ERR_INVALID, "decode tables and bitstream slots do not fit into LDS");
        }
    }
    if (code == MEMB_HIP_OK && ctx->lanesPerWord > 1) {
        code = deviceAlloc(
            ctx, &ctx->segmentIndex,
            size_t(desc->n_rows) * (ctx->lanesPerWord - 1) * (ctx->indexWide ? sizeof(uint32_t) : sizeof(uint16_t)));
    }
    if (code == MEMB_HIP_OK) {
        code = buildSegmentIndex(ctx, ctx->lanesPerWord, ctx->segmentSymbols, ctx->segmentIndex);
    }
    // Lookups read a row's stream start and segment offsets as one 16-byte record with one load
    // per lane: one request per word of a random batch (the two arrays cost two or three), one
    // per tile of a key-order dump. With row records the same record sits in front of the row's
    // stream instead and costs no request of its own.
    const bool records = ctx->recordPieces != 0;
    if (code == MEMB_HIP_OK && desc->n_rows && ctx->lanesPerWord > 1 && ctx->lanesPerWord <= ROW_META_MAX_LANES &&
        uint64_t(ctx->maxStreamBytes) * 8 + 64 < (1u << ROW_META_BITS) && (records || envUint("MEMB_HIP_ROW_META", 1))) {
        uint32_t* lengths = nullptr;   // per-row stream bytes, staging only
        if (records) {
            hipError_t status = hipMalloc(reinterpret_cast<void**>(&lengths), desc->n_rows * 4);
            if (status != hipSuccess) {
                code = fail(MEMB_HIP_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(status));
            } else {
                code = copyToDevice(lengths, ctx->streamBytes.data(), desc->n_rows * 4);
            }
        } else {
            code = deviceAlloc(ctx, &ctx->rowMeta, size_t(desc->n_rows) * 16 + 16);
        }
        if (code == MEMB_HIP_OK) {
            const uint32_t threads = 256;
            hipLaunchKernelGGL(
                pack_row_meta, dim3(static_cast<uint32_t>((desc->n_rows + threads - 1) / threads)), dim3(threads), 0,
                ctx->stream, ctx->streamStarts, ctx->segmentIndex, ctx->lanesPerWord, desc->n_rows,
                records ? reinterpret_cast<uint32_t*>(ctx->streams) : ctx->rowMeta, ctx->recordPieces, lengths);
            hipError_t status = hipGetLastError();
            if (status == hipSuccess) {
                status = hipStreamSynchronize(ctx->stream);
            }
            if (status != hipSuccess) {
                code = fail(MEMB_HIP_ERR_DEVICE, std::string("pack_row_meta: ") + hipGetErrorString(status));
            }
        }
        if (lengths) {
            (void)hipFree(lengths);
        }
    }
    // The finer index of small batches (memb_hip_ctx::fineIndex): about sixteen lanes per word for models staged as row
    // records -- a second pass of the index kernel, 2 bytes per offset (53 MB for the 2.2 M-word model of dim 300: a
    // seventh of its footprint on a 288 GB part).
    if (code == MEMB_HIP_OK && records && desc->n_rows && !ctx->indexWide) {
        const uint32_t group = ctx->fast ? 8 : 4;
        const uint32_t wanted = 16;
        const uint32_t symbols = std::max<uint32_t>(group, ((desc->dim + wanted - 1) / wanted + group - 1) / group * group);
        const uint32_t lanes = (desc->dim + symbols - 1) / symbols;
        if (lanes > ctx->lanesPerWord && lanes <= WAVE) {
            // (an optimisation of small batches: a model that cannot have it -- no memory left, a failed pass -- is staged without)
            const size_t fineBytes = size_t(desc->n_rows) * (lanes - 1) * sizeof(uint16_t) + 16;
            int fine = deviceAlloc(ctx, &ctx->fineIndex, fineBytes);
            if (fine == MEMB_HIP_OK) {
                fine = buildSegmentIndex(ctx, lanes, symbols, ctx->fineIndex);
            }
            if (fine == MEMB_HIP_OK) {
                ctx->fineLanes = lanes;
                ctx->fineSymbols = symbols;
            } else {
                (void)hipGetLastError();
                deviceRelease(ctx, &ctx->fineIndex, fineBytes);
            }
        }
    }
    return code;
}

int ctx_create_trained_checked(memb_hip_ctx** out, int device, const memb_hip_trained_desc* desc)
{
    if (!out || !desc) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if (desc->dim == 0 || desc->n_keys == 0 || desc->n_keys > 256 || desc->n_centroids > 255 ||
        (desc->n_rows && !desc->value_offsets) || (desc->packed_values_bytes && !desc->packed_values)) {
        return fail(MEMB_HIP_ERR_INVALID, "inconsistent trained storage description");
    }

    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tStart = now();
    DeviceRestore restore;
    memb_hip_ctx* ctx = new memb_hip_ctx();
    ContextGuard guard(ctx);   // destroys the context unless it is handed to the caller
    ctx->switches = readSwitches();
    ctx->storage = memb::wire::Storage_Trained;
    ctx->dim = desc->dim;
    ctx->nRows = desc->n_rows;

    // host side: tables and stream lengths (everything that can refuse a description does so
    // before a device is opened)
    int code = buildHostTable(ctx, desc);
    if (code == MEMB_HIP_OK) {
        code = measureStreams(ctx, desc);
    }
    if (code != MEMB_HIP_OK) {
        return code;
    }
    // (sized for row records first: stageStreams shrinks it when the model stays on the compact layout)
    ctx->slotDwords = recordSlotDwords(ctx->maxStreamBytes);
    ctx->fast = desc->n_centroids <= 16 && ctx->hostTable.maxCodeBits <= 8 && !ctx->hostTable.hasSubTables &&
        !envUint("MEMB_HIP_NO_FAST", 0);
    ctx->tableDwords = static_cast<uint32_t>((2 * ctx->hostTable.entries.size() + 3) / 4 * 4);
    const double tSorted = now();

    code = openDevice(ctx, device);
    if (code == MEMB_HIP_OK) {
        chooseLanes(ctx, desc);   // before the streams: the layout depends on the lanes per word
        code = stageStreams(ctx, desc);
    }
    const double tRepacked = now();
    if (code == MEMB_HIP_OK) {
        code = stageTables(ctx, desc);
    }
    if (code == MEMB_HIP_OK) {
        code = stageIndex(ctx, desc);
    }
    if (ctx->switches.verbose) {
        std::fprintf(stderr, "memb_hip: stage trained rows=%llu: host lengths %.3fs, device open + copy + repack %.3fs, tables + index %.3fs\n",
                     static_cast<unsigned long long>(desc->n_rows), tSorted - tStart, tRepacked - tSorted, now() - tRepacked);
    }
    if (code != MEMB_HIP_OK) {
        return code;
    }
    *out = guard.release();
    return MEMB_HIP_OK;
}

int ctx_create_uniform_checked(memb_hip_ctx** out, int device, const memb_hip_uniform_desc* desc)
{
    if (!out || !desc) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if (desc->dim == 0 || (desc->n_rows && !desc->rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "inconsistent uniform storage description");
    }
    DeviceRestore restore;
    memb_hip_ctx* ctx = new memb_hip_ctx();
    ContextGuard guard(ctx);   // destroys the context unless it is handed to the caller
    ctx->switches = readSwitches();
    ctx->storage = memb::wire::Storage_Uniform;
    ctx->dim = desc->dim;
    ctx->nRows = desc->n_rows;
    ctx->levels = static_cast<float>(desc->quantization_levels);

    // HBM layout: ROW RECORDS (UniformParams::records) -- every row owns 16 bytes of {min, max} and its
    // weights, one byte each, zero padded to whole 16-byte pieces. The file scatters each row in its own
    // table; rows shorter than dim are zero padded (the reference writes only values->size() outputs there).
    ctx->regionPieces = 1 + (desc->dim + 15) / 16;
    const size_t regionBytes = size_t(ctx->regionPieces) * 16;
    std::vector<uint8_t> records((size_t(desc->n_rows) + 1) * regionBytes, 0);   // + one region of guard
    for (uint64_t r = 0; r < desc->n_rows; ++r) {
        const memb_hip_uniform_row& row = desc->rows[r];
        uint8_t* region = records.data() + r * regionBytes;
        const float header[2] = {row.min_value, row.max_value};
        std::memcpy(region, header, sizeof(header));
        size_t count = std::min<size_t>(row.n_values, desc->dim);
        if (count) {
            std::memcpy(region + 16, row.values, count);
        }
    }

    int code = openDevice(ctx, device);
    if (code == MEMB_HIP_OK) {
        code = deviceAlloc(ctx, &ctx->uniformRecords, records.size());
    }
    if (code == MEMB_HIP_OK) {
        code = copyToDevice(ctx->uniformRecords, records.data(), records.size());
    }
    if (code != MEMB_HIP_OK) {
        return code;
    }
    *out = guard.release();
    return MEMB_HIP_OK;
}

int ctx_create_full_checked(memb_hip_ctx** out, int device, const memb_hip_full_desc* desc)
{
    if (!out || !desc) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if (desc->dim == 0 || (desc->n_rows && !desc->rows)) {
        return fail(MEMB_HIP_ERR_INVALID, "inconsistent full storage description");
    }
    DeviceRestore restore;
    memb_hip_ctx* ctx = new memb_hip_ctx();
    ContextGuard guard(ctx);   // destroys the context unless it is handed to the caller
    ctx->switches = readSwitches();
    ctx->storage = memb::wire::Storage_Full;
    ctx->dim = desc->dim;
    ctx->nRows = desc->n_rows;

    std::vector<float> values(size_t(desc->n_rows) * desc->dim, 0.f);
    for (uint64_t r = 0; r < desc->n_rows; ++r) {
        const memb_hip_full_row& row = desc->rows[r];
        size_t count = std::min<size_t>(row.n_values, desc->dim);
        if (count) {
            std::memcpy(values.data() + r * desc->dim, row.values, count * sizeof(float));
        }
    }
    int code = openDevice(ctx, device);
    if (code == MEMB_HIP_OK) {
        code = deviceAlloc(ctx, &ctx->fullValues, values.size() * sizeof(float) + 16);
    }
    if (code == MEMB_HIP_OK) {
        code = copyToDevice(ctx->fullValues, values.data(), values.size() * sizeof(float));
    }
    if (code != MEMB_HIP_OK) {
        return code;
    }
    *out = guard.release();
    return MEMB_HIP_OK;
}
