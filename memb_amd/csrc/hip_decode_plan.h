// Launch geometry of the decode kernels: how a batch picks its kernel, its block size, its LDS and its
// parameters. Rules only: nothing here enqueues work.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the context
// (hip_context.h) and the kernel table (hip_kernel_table.h); see that file for the overview.
#pragma once

struct TrainedGeometry {
    uint32_t waves;      // wavefronts per block
    uint32_t ldsBytes;   // dynamic LDS per block
    int mode;
    uint32_t resident;   // wavefronts a CU holds at this block size (LDS and registers)
};

// Wavefronts per CU the registers of the one-tile kernels (decode_trained, decode_trained_batches, decode_union_split)
// admit: 57-61 vector registers would allow 8 per SIMD, but the hardware hands out scalar registers too -- 800 per SIMD
// in steps of 16 plus 16 (MI355X_MICROARCH.md, "Residency and cooperative launch") -- and the compiler, which does not
// count that, took 106: SIX per SIMD, 24 per CU, in rounds 1-4 (seen in round 5 as a step in the time of small batches at
// exactly 24 x CUs tiles). hip_trained_kernels.h now holds these kernels to a budget (MEMB_HIP_SGPRS = 96: .sgpr_count 94,
// no vector register more, 12 lane spills in the headline kernel's 2 000 instructions; 88 gives the same seven with 20): SEVEN per SIMD. A budget of 80 (8 per SIMD) costs two vector registers of spills, 3-5 % on the
// chain of a small batch, and in blocks of eight +5 % on a key-order dump (round 5, batches 16-18, profiles/r05_experiments.txt);
// tests/test_isa.py pins the seven.
constexpr uint32_t ONE_TILE_WAVES_PER_CU = 28;

// ceil(2^32 / d) for fastDivide: exact for every q <= maxQ when maxQ * d < 2^32.
// Returns 0 (plain division) for d == 1, where the magic does not fit 32 bits,
// and when the range is too large.
uint32_t magicFor(uint32_t d, uint64_t maxQ)
{
    if (d <= 1 || maxQ * d >= (1ull << 32)) {
        return 0;
    }
    return static_cast<uint32_t>(((1ull << 32) + d - 1) / d);
}

uint32_t roundUp4(uint32_t v)
{
    return (v + 3) / 4 * 4;
}

// LDS dwords of one word's bitstream slot: the stream plus the 12-byte window the decoder reads
// at its last position, whole 16-byte pieces, an odd number of them so that equal positions in
// consecutive slots fall into different LDS banks.
uint32_t compactSlotDwords(uint32_t maxStreamBytes)
{
    return (((maxStreamBytes + 12 + 15) / 16) | 1u) * 4;
}

// Same with a row record in front (16 bytes of record + the longest stream, rounded up to 32:
// stageStreams), which must fit in front of that window as well.
uint32_t recordSlotDwords(uint32_t maxStreamBytes)
{
    return (((((16 + maxStreamBytes + 31) / 32) * 32 + 12 + 15) / 16) | 1u) * 4;
}

// symbol tile of one wave: rows of dim bytes (dword aligned) or dim / 2 bytes (FAST)
uint32_t keyRowBytes(const memb_hip_ctx* ctx)
{
    return ctx->fast ? ((ctx->dim + 1) / 2 + 1) / 2 * 2 : roundUp4(ctx->dim);
}

uint32_t keyTileDwords(const memb_hip_ctx* ctx, uint32_t wordsPerWave)
{
    return wordsPerWave ? (wordsPerWave * keyRowBytes(ctx) + 3) / 4 + 1 : 0;
}

uint32_t codebookDwords(const memb_hip_ctx* ctx)
{
    return ctx->fast ? 512u : 256u;
}

// LDS dwords of the PACKED kernels' table (4-byte entries, padded to 16 bytes)
uint32_t packedTableDwords(const memb_hip_ctx* ctx)
{
    return roundUp4(static_cast<uint32_t>(ctx->byteTable.entries.size()));
}

// withKeys: a lookup kernel (symbol tiles; byte-key models then use the PACKED layout); without: the index pass.
// outBytes: bytes of an output element, whose codebook the lookup kernel holds in LDS (2: decode_trained_narrow)
uint32_t trainedLdsBytes(const memb_hip_ctx* ctx, uint32_t waves, uint32_t wordsPerWave, bool withKeys, uint32_t outBytes = 4)
{
    uint32_t perWave = wordsPerWave * ctx->slotDwords + (withKeys ? keyTileDwords(ctx, wordsPerWave) : 0);
    const uint32_t codebook = codebookDwords(ctx) * outBytes / 4;
    if (withKeys && !ctx->fast) {
        return 4u * (packedTableDwords(ctx) + codebook + waves * perWave);
    }
    return 4u * (ctx->tableDwords + codebook + waves * perWave);
}

// How a kernel writes rows of dim elements of elementBytes (4: fp32, 2: bf16 / fp16) to out + row * ld + colOff (ld and
// colOff in elements). The two rules side by side:
//   OUT_VEC4  pieces of four elements, row by row (16- / 8-byte stores): dim, ld and colOff multiples of four and `out`
//             aligned to a piece; else OUT_SCALAR, one element per store
//   OUT_FLAT  one dense run of 16-byte pieces where the rows lie back to back (ld == dim, colOff == 0). 4-byte elements:
//             nothing more to ask. 2-byte elements: 16 bytes are eight values, so `out` must be 16-byte aligned and every
//             tile of wordsPerWave rows must start on such a boundary -- dim a multiple of 8, or an even number of words
//             per tile. (The row-wise kernels only ask whether the answer is OUT_SCALAR: wordsPerWave 0.)
int outputMode(uint32_t dim, size_t ld, size_t colOff, const void* out, uint32_t elementBytes, uint32_t wordsPerWave)
{
    const uintptr_t address = reinterpret_cast<uintptr_t>(out);
    if (dim % 4 != 0 || ld % 4 != 0 || colOff % 4 != 0 || address % (4 * elementBytes) != 0) {
        return OUT_SCALAR;
    }
    bool dense = ld == dim && colOff == 0;
    if (elementBytes == 2) {
        dense = dense && address % 16 == 0 && (dim % 8 == 0 || wordsPerWave % 2 == 0);
    }
    return dense ? OUT_FLAT : OUT_VEC4;
}

// What a caller asks of a decode launch: rows[0 .. n) as rows of outType elements (MEMB_HIP_OUT_*) at out + i * ld + colOff
// (ld, colOff in elements); fp32 rows may pass through the epilogue of a union (hip_device_common.h: accumulate, divide).
struct Lookup {
    const uint32_t* rows = nullptr;
    size_t n = 0;
    void* out = nullptr;
    int outType = MEMB_HIP_OUT_F32;
    size_t ld = 0;
    size_t colOff = 0;
    uint32_t accumulate = 0;
    float divisor = 0.f;
    bool randomOrder = false;   // the caller's hint MEMB_HIP_ROWS_IN_RANDOM_ORDER (launch geometry only)
    bool keysOut = false;       // trained: `out` receives rows of centroid indices (OUT_KEYS) instead; ld = dim, colOff = 0

    uint32_t elementBytes() const { return outType == MEMB_HIP_OUT_F32 ? 4u : 2u; }
};

Lookup floatRows(const uint32_t* rows, size_t n, float* out, size_t ld, size_t colOff)
{
    return Lookup{rows, n, out, MEMB_HIP_OUT_F32, ld, colOff};
}

// Wavefronts a CU holds in blocks of `waves` with ldsBytes of LDS each (0: the block does not fit). LDS is handed out in
// 1 KiB steps of a 160 KiB pool; at most 32 waves per CU, fewer when the kernel's registers say so (registerWaves: 512
// per lane and SIMD, MI355X_MICROARCH.md "Register files").
uint32_t residentWaves(uint32_t ldsLimit, uint32_t waves, uint32_t ldsBytes, uint32_t registerWaves)
{
    if (ldsBytes > ldsLimit) {
        return 0;
    }
    const uint32_t blocksPerCu = std::min<uint32_t>(
        ldsLimit / ((ldsBytes + 1023) / 1024 * 1024), std::max<uint32_t>(1, std::min<uint32_t>(32, registerWaves) / waves));
    return blocksPerCu * waves;
}

// Wavefronts per block: the PREFERRED size (planTrained: eight for batches of more than 16 R tiles, else four), unless
// another size lets a CU hold at least a quarter more resident wavefronts (LDS is handed out per block: the 8-bit model's
// 33 KiB of tables leave 12 wavefronts per CU in blocks of four and 16 in blocks of eight, which is worth 10-17 %; the
// 6-bit model's 28 against 32 is not worth leaving the preference: round 5, batch 7). Where the preferred size does not
// fit: the size with the most resident wavefronts, in the order 4, 8, 2, 1. MEMB_HIP_WAVES / option waves_per_block forces a
// size. registerWavesPerCu: how many wavefronts of the kernel about to be launched its registers let a CU hold (32 when
// unknown): a block size whose LDS would allow more resident wavefronts than the registers do gains nothing by it.
// outBytes: of the output element, whose codebook the kernel holds in LDS. (`mode` is not set here: planTrained.)
TrainedGeometry chooseGeometry(
    const memb_hip_ctx* ctx, uint32_t wordsPerWave, uint32_t outBytes, uint32_t preferred = 4,
    uint32_t registerWavesPerCu = ONE_TILE_WAVES_PER_CU)
{
    TrainedGeometry best{};
    const uint32_t forcedWaves = ctx->switches.waves;   // (1 .. 16; anything but 1, 2, 4, 8: measurements)
    auto residentWith = [&](uint32_t waves, uint32_t* ldsBytes) -> uint32_t {
        *ldsBytes = trainedLdsBytes(ctx, waves, wordsPerWave, true, outBytes);
        return residentWaves(ctx->ldsLimit, waves, *ldsBytes, registerWavesPerCu);
    };
    uint32_t preferredLds = 0;
    const uint32_t wanted = forcedWaves ? forcedWaves : preferred;
    const uint32_t preferredResident = residentWith(wanted, &preferredLds);
    uint32_t bestResident = 0;
    for (uint32_t waves : {4u, 8u, 2u, 1u}) {
        if (forcedWaves) {
            break;
        }
        uint32_t ldsBytes = 0;
        const uint32_t resident = residentWith(waves, &ldsBytes);
        if (resident > bestResident) {
            bestResident = resident;
            best.waves = waves;
            best.ldsBytes = ldsBytes;
        }
    }
    best.resident = bestResident;
    if (preferredResident && (forcedWaves || 4 * bestResident < 5 * preferredResident)) {
        best.waves = wanted;
        best.ldsBytes = preferredLds;
        best.resident = preferredResident;
    }
    return best;
}

TrainedParams baseTrainedParams(const memb_hip_ctx* ctx)
{
    TrainedParams params{};
    params.streams = ctx->streams;
    params.streamStarts = ctx->streamStarts;
    params.segmentIndex = ctx->segmentIndex;
    params.indexWide = ctx->indexWide ? 1u : 0u;
    params.rowMeta = ctx->rowMeta;
    params.recordPieces = ctx->recordPieces;
    params.loadPieces = ctx->recordPieces ? ctx->recordPieces : ctx->slotDwords / 4;
    params.table = ctx->table;
    params.codebook = ctx->codebook;
    params.nRows = ctx->nRows;
    params.tableDwords = ctx->tableDwords;
    params.codebookDwords = codebookDwords(ctx);
    params.rootBits = ctx->hostTable.rootBits;
    params.dim = ctx->dim;
    params.slotDwords = ctx->slotDwords;
    params.slotMagic = magicFor(params.loadPieces, 64ull * params.loadPieces * 5);
    params.debugFlags = ctx->switches.debugFlags;
    params.tilesPerWave = 1;
    return params;
}

// The parameters of a lookup kernel that do not depend on the batch. fine: decode with the finer index (more lanes per
// word, fewer words per wavefront; memb_hip_ctx::fineIndex).
TrainedParams lookupParams(const memb_hip_ctx* ctx, bool fine = false)
{
    const uint32_t lanesPerWord = fine ? ctx->fineLanes : ctx->lanesPerWord;
    const uint32_t wordsPerWave = WAVE / lanesPerWord;
    TrainedParams params = baseTrainedParams(ctx);
    if (fine) {
        params.segmentIndex = ctx->fineIndex;
        params.fineIndex = 1;
        params.slotMagic = magicFor(params.loadPieces, 64ull * params.loadPieces * 5);
    }
    params.lanesPerWord = lanesPerWord;
    params.laneMagic = magicFor(lanesPerWord, WAVE);
    params.wordsPerWave = wordsPerWave;
    params.segmentSymbols = fine ? ctx->fineSymbols : ctx->segmentSymbols;
    params.keyRowBytes = keyRowBytes(ctx);
    params.keyTileDwords = keyTileDwords(ctx, wordsPerWave);
    params.pieceMagic = magicFor(ctx->dim / 4, uint64_t(wordsPerWave) * (ctx->dim / 4));
    if (!ctx->fast) {
        // byte keys: the PACKED kernels' table (4-byte entries, tableDwords of them incl. padding)
        params.table = ctx->table32;
        params.rootBits = ctx->byteTable.rootBits;
        params.tableDwords = packedTableDwords(ctx);
    }
    return params;
}

// The kernels index LDS and the symbol tile from these numbers without further checks.
bool lookupParamsConsistent(const memb_hip_ctx* ctx, const TrainedParams& params, const TrainedGeometry& geometry)
{
    const uint32_t wordsPerWave = params.wordsPerWave;
    const uint32_t group = ctx->fast ? 8 : 4;
    return wordsPerWave >= 1 && wordsPerWave * params.lanesPerWord <= WAVE &&
        params.slotDwords >= 4 && params.slotDwords % 4 == 0 && params.segmentSymbols % group == 0 &&
        params.loadPieces >= 1 && params.loadPieces * 4 <= params.slotDwords &&
        (!params.recordPieces || ((params.fineIndex || params.lanesPerWord <= ROW_META_MAX_LANES) && params.slotDwords >= 4 * params.recordPieces + 3)) &&
        uint64_t(params.lanesPerWord) * params.segmentSymbols >= params.dim &&
        uint64_t(params.lanesPerWord - 1) * params.segmentSymbols < params.dim &&
        params.keyRowBytes * (ctx->fast ? 2u : 1u) >= params.dim &&
        uint64_t(params.keyTileDwords) * 4 >= uint64_t(wordsPerWave) * params.keyRowBytes &&
        (params.lanesPerWord == 1 || params.segmentIndex != nullptr) &&
        geometry.ldsBytes == trainedLdsBytes(ctx, geometry.waves, wordsPerWave, true, 4 * params.codebookDwords / codebookDwords(ctx)) &&
        (ctx->fast || (params.table != nullptr && params.tableDwords >= (1u << params.rootBits))) &&
        geometry.ldsBytes <= ctx->ldsLimit;
}

// Tiles a wavefront of the one-tile kernels (decode_trained, decode_union_split) decodes one after the other, behind
// ONE copy of table(s) and codebook(s) into LDS per block. Measured (round 4, batches 2-4 and 12; `copyBytes` = what a
// block copies): the copy is 2.8 % of a 4-bit dump (4 KiB) and more than it gains back there (T = 2: -0.9 % / +1.9 % key
// order / shuffled, T = 4: +3.6 %); it is what made the 8-bit model (33 KiB) the last customer of the general persistent
// kernel (T = 2: dumps +0.1..0.3 % against it, 500 k rows -1.5 %). The split union -- 8 KiB for four tiles of four words,
// and with T > 1 a pipeline of depth one (the next tile's row regions in flight during a tile's decode and stores) --
// wants T = 2 at every size measured once its copy is overlapped with the first tile's loads (batch 12: 30 k words -6 %,
// 100 k -2 %, 160 k -3 %, 500 k -4 %, 1 M -3 % against T = 1; T = 3 and 4 are behind T = 2 everywhere).
uint32_t oneTileSteps(const memb_hip_ctx* ctx, uint64_t tiles, uint32_t copyBytes, bool unionSplit)
{
    if (ctx->switches.tilesPerWave) {
        return std::min<uint32_t>(ctx->switches.tilesPerWave, 64);
    }
    const uint64_t slots = uint64_t(ctx->cuCount) * 32;   // (the unit the thresholds below were measured in)
    if (unionSplit) {
        return 2 * tiles >= slots ? 2u : 1u;   // (from 16 k words on 256 CUs; below, halving the grid leaves CUs idle)
    }
    return copyBytes >= 16 * 1024 && tiles >= 2 * slots ? 2u : 1u;
}

// Which kernel a batch of this output shape runs, and with what launch geometry.
struct TrainedPlan {
    bool fine = false;                   // decode_trained with the finer index (small batches)
    bool persistent = false;             // decode_records_persistent (else decode_trained)
    TrainedGeometry geometry{};
    const KernelInstance<TrainedParams>* kernel = nullptr;   // the instance that runs (lookupKernel)
    uint32_t registerWavesPerCu = 32;    // persistent only: what the kernel's registers allow
    int numRegs = 0;
};

constexpr uint64_t PIPELINE_WAVES_PER_CU = 16;   // the unit R of the rule below (times the CUs)
// Do the rows of very large batches come in no particular order? The caller's word for it (MEMB_HIP_ROWS_IN_RANDOM_ORDER),
// else what the kernel of the last such batch saw (memb_hip_ctx::orderSeen); key order until something was seen.
bool rowsUnordered(const memb_hip_ctx* ctx, bool callerSaysRandom)
{
    if (callerSaysRandom) {
        return true;
    }
    return ctx->orderSeen && __atomic_load_n(ctx->orderSeen, __ATOMIC_RELAXED) == 0;
}

// (the context's device is current)
// Which kernel by batch size (n words): a STATIC rule. t = tiles of the batch, R = 16 x CUs. Round 4 measured every
// kernel of rounds 1-3 on every model kind (2-, 4-, 6-bit, byte-key 4-bit, Student-t 4-bit; key order, shuffled, 100 k,
// 500 k; round 4, batch 1, profiles/r04_experiments.txt: two boxes, A/A floor 0.5 %) and kept what wins a BASELINE configuration by 3 %:
//   decode_trained (one tile per wavefront at a time, 52-61 VGPRs; 28 wavefronts per CU by its scalar registers, 24 until
//   round 5: ONE_TILE_WAVES_PER_CU) -- everything, except
//   one round of the one-tile kernel (28 x CUs = 1.75 R) < t <= 4 R on row-record models: decode_records_persistent (24
//   wavefronts per CU, software pipeline):
//       100 000 rows -4.3..-6 % (4-bit), -8..-9 % (6-bit), -1.5 % (2-bit); at 500 k rows it is 3-11 % BEHIND.
// The general persistent pipeline lost every dump (+2.3 % 4-bit, +4.9 % 2-bit; 6-bit -1.8 % on one box) and every
// shuffled batch (+1.7..+9.4 %); with it went the per-context timing that chose between the two ("autotune").
// Block size: four wavefronts; EIGHT for batches of more than 16 R tiles (524 000 words on 256 CUs) -- dumps: the
// reference's own large batch is keys() in key order (python/memb/reader.py:27-28). Round 5, batch 7 (one box, every model
// kind, both orders; eight against four): key-order dumps 4-bit -2.4 %, 2-bit -5.0 %, 6-bit -1.0 %, 9-bit-code 4-bit
// -1.1 %, Student-t -2.5 %; the same batches SHUFFLED +3.4 %, -1.3 %, +3.6 %, +3.5 %, +2.9 %; 1 M random rows +2.0 %, -1.5 %,
// +2.5 %, +2.7 %, +2.1 %: the rule takes the dump's side for every key format and says what it costs the other order
// (HISTORY.md, "(r5) 5.0", has the table; DESIGN.md section 5.0 the rule as it stands). The 8-bit model runs blocks of eight at every size: chooseGeometry.
// force: -1 = by the rule, 0 = one tile per wavefront, 1 = decode_records_persistent where the layout allows.
// mayBeFine: whether the finer index may be chosen at all. randomOrder: rowsUnordered's answer (very large batches).
// Of the lookup, its size, the shape of its output (-> geometry.mode) and the size of its elements count: 2-byte ones
// (decode_trained_narrow) take half the LDS for the codebook.
int planTrained(const memb_hip_ctx* ctx, const Lookup& lookup, int force, bool mayBeFine, bool randomOrder, TrainedPlan* plan)
{
    const size_t n = lookup.n;
    const uint32_t outBytes = lookup.elementBytes();
    uint32_t wordsPerWave = WAVE / ctx->lanesPerWord;
    const uint64_t tiles = (n + wordsPerWave - 1) / wordsPerWave;
    const uint64_t R = uint64_t(ctx->cuCount) * PIPELINE_WAVES_PER_CU;
    // One round = the tiles the CUs hold at once (`resident` = wavefronts per CU at the block size of a small batch, by LDS
    // and registers; x CUs). Two edges of the rule are rounds:
    //   * the FINER INDEX while the batch's fine tiles all fit one round (28 600 words on 256 CUs): every wavefront has one
    //     tile, the batch is one chain of dependent steps per wavefront, and the finer index shortens its longest link, the
    //     decode. Round 5 (batches 3, 17 and 26, profiles/r05_experiments.txt; the usual index = 100 %), 1 000 /
    //     10 000 / 20 000 / 28 000 rows: 4-bit -12 / -13 / -8 / -4 % with the same batch repeated, -15 / -8 / -5 / -5 % with
    //     nothing cached between launches; 6-bit -15 / -17 / -9 / -8 % and -21 / -13 / -9 / -8 %. One row more than a round
    //     and its second round costs what the index saved (30 000 rows +9 / +5 %; nothing cached: +16 / +12 %, 50 000 rows +33 %).
    //   * decode_records_persistent from ONE ROUND OF THE USUAL INDEX on (57 344 words; until the end of round 5: from 2 R =
    //     65 536): past one round the one-tile kernel runs a nearly empty second one (56 000 -> 60 000 rows: 17.3 -> 21.0 us),
    //     the pipeline's wavefronts take a second tile instead. 58 000 / 62 000 / 65 000 rows against the one-tile kernel,
    //     nothing cached: 4-bit -9 / -10 / -11 %, 6-bit -7 / -10 / -12 %; the same batch repeated: -6 / 0 % at 60 000 rows.
    //     (For a few hours the rule sent this band to the finer index, on measurements of a repeated batch alone: -6..-12 %
    //     there, +9..+18 % with nothing cached -- 20-32 % behind the pipeline. Batch 26.)
    // (a forced kernel -- option persistent = 2, force = 1 -- wins over the rule, a forced finer index over both)
    bool fineByRule = false;
    if (mayBeFine && ctx->fineIndex && ctx->switches.fineLanes == 0 && ctx->switches.persistent != 2 && force != 1) {
        const uint32_t fineWords = WAVE / ctx->fineLanes;
        const uint64_t fineTiles = (n + fineWords - 1) / fineWords;
        const uint64_t fineRound =
            uint64_t(ctx->cuCount) * chooseGeometry(ctx, fineWords, outBytes).resident;
        fineByRule = fineTiles <= fineRound;
    }
    plan->fine = mayBeFine && ctx->fineIndex && force != 1 && (ctx->switches.fineLanes == 2 || fineByRule);
    // (models whose tables leave a CU fewer than 1.5 R wavefronts -- the 8-bit one -- keep the edge at 2 R: not measured there)
    const uint64_t usualRound =
        uint64_t(ctx->cuCount) * chooseGeometry(ctx, wordsPerWave, outBytes).resident;
    const uint64_t pipelineFrom = 2 * usualRound >= 3 * R ? std::min<uint64_t>(2 * R, usualRound) : 2 * R;
    if (plan->fine) {
        wordsPerWave = WAVE / ctx->fineLanes;
    }
    // the pipeline keeps a tile's row regions in two registers per lane: the slot image must fit two 64-lane rounds
    const bool recordsFit = ctx->recordPieces && wordsPerWave * (ctx->slotDwords / 4) <= RECORD_ROUNDS * WAVE;
    bool wantPersistent = ctx->switches.persistent == 2 || (ctx->switches.persistent == 1 && tiles > pipelineFrom && tiles <= 4 * R);
    if (force >= 0) {
        wantPersistent = force != 0;
    }
    plan->persistent = recordsFit && wantPersistent && !plan->fine;
    // Block size of very large batches (more than 16 R tiles): EIGHT wavefronts for rows in key order -- the dumps; three
    // blocks = 24 resident wavefronts per CU and a table copy per eight tiles -- and, for rows in no particular order
    // (randomOrder: the caller's hint or what the last such batch looked like, rowsUnordered), SEVEN: four whole blocks = the
    // 28 wavefronts the registers admit, which random row regions (two lines each) want in flight. Round 6, batches 2-3, two
    // boxes, seven against eight: shuffled 2.2 M rows 4-bit -4.7 / -3.7 %, 6-bit -3.6 / -4.7 %, byte-key 4-bit -4.6 %,
    // Student-t -3.8 %, 1 M random rows -5.6 / -3.8 % (four: -3.0 / -2.3, -1.2 / -3.6, -3.4, -2.8, -4.6 / -2.3 %); key-order
    // dumps -0.3 / +4.9 % (4-bit), -5.5 / -1.0 % (6-bit), +2.5 %, +5.0 %: the order decides, which is why it is looked at.
    // Models with row regions below 160 bytes (the 2-bit one) keep four: seven costs them 5-10 % in either order. And seven
    // only where it DOES hold more resident wavefronts than eight: models with large tables (8-bit: 33-45 KiB of LDS per
    // block) get their block size for residency (chooseGeometry; eight against four: -10..-15 %, round 5) and keep eight.
    // (Batch 7, the 8-bit Student-t model, 21 resident in blocks of seven against 24: seven -2.0 % shuffled, +1.2 % key order.)
    uint32_t unorderedWaves = ctx->recordPieces >= 10 ? 7u : 4u;
    if (unorderedWaves == 7 && !ctx->switches.waves &&
        chooseGeometry(ctx, wordsPerWave, outBytes, 7).resident <= chooseGeometry(ctx, wordsPerWave, outBytes, 8).resident) {
        unorderedWaves = 8;
    }
    const uint32_t preferred = !plan->persistent && tiles > 16 * R ? (randomOrder ? unorderedWaves : 8u) : 4u;
    plan->geometry = chooseGeometry(ctx, wordsPerWave, outBytes, preferred);
    // (the fp32 instance; a narrow lookup runs memb_narrow::trainedKernel of the same mode: launchTrained)
    const int mode = lookup.keysOut ? OUT_KEYS : outputMode(ctx->dim, lookup.ld, lookup.colOff, lookup.out, outBytes, wordsPerWave);
    plan->geometry.mode = mode;
    plan->kernel = &lookupKernel(ctx, plan->persistent, mode);
    if (plan->persistent && plan->geometry.waves) {
        // again with what the kernel's registers allow (a block size whose LDS would hold more wavefronts than
        // the registers admit is no better than a smaller one)
        KernelFacts facts;
        hipError_t status = kernelFacts(plan->kernel->fn, &facts);
        if (status != hipSuccess) {
            return fail(MEMB_HIP_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(status));
        }
        plan->registerWavesPerCu = facts.registerWavesPerCu;
        plan->numRegs = facts.numRegs;
        plan->geometry = chooseGeometry(ctx, wordsPerWave, outBytes, 4, plan->registerWavesPerCu);
        plan->geometry.mode = mode;
    }
    if (plan->fine && !plan->geometry.waves) {   // (cannot happen: fewer words per wavefront need less LDS)
        plan->fine = false;
        return planTrained(ctx, lookup, force, false, randomOrder, plan);
    }
    return MEMB_HIP_OK;
}

// Grid of a launch of the one-tile kernels over `tiles` tiles in blocks of `waves` wavefronts: sets params->tilesPerWave
// (oneTileSteps) and *blocks.
int oneTileBlocks(const memb_hip_ctx* ctx, uint64_t tiles, uint32_t waves, TrainedParams* params, uint32_t* blocks)
{
    params->tilesPerWave = oneTileSteps(ctx, tiles, 4u * (params->tableDwords + params->codebookDwords), false);
    const uint64_t perBlock = uint64_t(waves) * params->tilesPerWave;
    const uint64_t count = (tiles + perBlock - 1) / perBlock;
    if (count >= 0x7FFFFFFFull) {
        return fail(MEMB_HIP_ERR_INVALID, "batches too large for one launch");
    }
    *blocks = static_cast<uint32_t>(count);
    return MEMB_HIP_OK;
}

// What the union kernels share (decode_trained_union, decode_union_split, pool_trained_union): the conditions under which
// models can share one -- MEMB_HIP_UNSUPPORTED with the reason otherwise -- and their parameters: every model's own tables,
// streams and row ids, one output (whose elements are elementBytes wide), tables and codebooks laid out in the block's LDS.
struct UnionPlan {
    UnionParams params{};
    bool hasSub = false;
    bool allFast = true;
    uint32_t wordsPerWave = 0;
};

int planUnion(
    memb_hip_ctx* const* ctxs, const uint32_t* const* rows, const size_t* colOffs, size_t count, size_t n, void* out,
    size_t elementBytes, size_t ld, UnionPlan* plan)
{
    // (MEMB_HIP_UNSUPPORTED is not an error, but memb_hip_last_error() says which condition it was)
    if (count < 2 || count > UNION_MAX_MODELS || (ctxs[0] && ctxs[0]->switches.unionFused == 0)) {
        return fail(MEMB_HIP_UNSUPPORTED, "union kernel: two to four models (or switched off by the first context's option union_fused = 0)");
    }
    const memb_hip_ctx* first = ctxs[0];
    bool hasSub = false;
    bool allFast = true;
    for (size_t m = 0; m < count; ++m) {
        const memb_hip_ctx* ctx = ctxs[m];
        if (ctx->storage != memb::wire::Storage_Trained || ctx->device != first->device || ctx->dim != first->dim ||
            ctx->lanesPerWord != first->lanesPerWord ||
            ctx->segmentSymbols != first->segmentSymbols || ctx->dim % 4 != 0 || colOffs[m] % 4 != 0 ||
            ld < colOffs[m] + ctx->dim) {
            return fail(MEMB_HIP_UNSUPPORTED, "union kernel: the models differ in storage, device, dim or lane geometry");
        }
        allFast = allFast && ctx->fast;
    }
    for (size_t m = 0; m < count; ++m) {
        // (byte keys decode through the 4-byte PACKED tables, whose first level is wider: hip_trained_kernels.h)
        hasSub = hasSub || (allFast ? ctxs[m]->hostTable.hasSubTables : ctxs[m]->byteTable.hasSubTables);
    }
    if (!allFast) {
        for (size_t m = 0; m < count; ++m) {
            if (!ctxs[m]->table32) {
                return fail(MEMB_HIP_UNSUPPORTED, "union kernel: a model has no byte-key table on the device");
            }
        }
    }
    // Nibble keys (<= 16 centroids, codes <= 8 bits) only when every model has them; a mixed union decodes the
    // nibble-key models through their byte-key tables (memb_hip_ctx::table32): the same symbols, one per byte.
    // (a piece of four elements: 16 bytes of fp32, 8 of bf16 / fp16)
    if (ld % 4 != 0 || reinterpret_cast<uintptr_t>(out) % (4 * elementBytes) != 0 || n > (size_t(1) << 37)) {
        return fail(MEMB_HIP_UNSUPPORTED, "union kernel: the output is not 16-byte aligned in every row");
    }
    const uint32_t wordsPerWave = WAVE / first->lanesPerWord;

    UnionParams& params = plan->params;
    params = UnionParams{};
    uint32_t sharedDwords = 0;
    for (size_t m = 0; m < count; ++m) {
        memb_hip_ctx* ctx = ctxs[m];
        TrainedParams& p = params.model[m];
        p = baseTrainedParams(ctx);
        p.rows = rows[m];
        p.out = static_cast<float*>(out);   // (2-byte elements for a narrow type)
        p.n = n;
        p.ld = ld;
        p.colOff = colOffs[m];
        p.lanesPerWord = ctx->lanesPerWord;
        p.laneMagic = magicFor(ctx->lanesPerWord, WAVE);
        p.wordsPerWave = wordsPerWave;
        p.segmentSymbols = ctx->segmentSymbols;
        p.keyRowBytes = allFast ? keyRowBytes(ctx) : roundUp4(ctx->dim);
        p.keyTileDwords = (wordsPerWave * p.keyRowBytes + 3) / 4 + 1;
        if (!allFast) {
            // byte keys: the single-model kernels' 4-byte table entries (decodeSegment<..., PACKED>); a nibble-key model
            // beside a byte-key one goes through its own byte-key table and plain codebook
            p.table = ctx->table32;
            p.tableDwords = packedTableDwords(ctx);
            p.rootBits = ctx->byteTable.rootBits;
            if (ctx->fast) {
                p.codebook = ctx->codebookBytes;
                p.codebookDwords = 256;
            }
        }
        p.pieceMagic = magicFor(ctx->dim / 4, uint64_t(wordsPerWave) * count * (ctx->dim / 4));
        p.debugFlags = first->switches.debugFlags;   // (measurement builds: the first reader's switches for all)
        params.tableOffsetDwords[m] = sharedDwords;
        sharedDwords += p.tableDwords;
    }
    params.codebookOffsetDwords = sharedDwords;
    sharedDwords += static_cast<uint32_t>(count) * 512;
    params.sharedDwords = sharedDwords;
    plan->hasSub = hasSub;
    plan->allFast = allFast;
    plan->wordsPerWave = wordsPerWave;
    return MEMB_HIP_OK;
}

// one wavefront's LDS area in decode_trained_union and pool_trained_union: bitstream slots and a symbol tile per model
void layOutUnionWave(memb_hip_ctx* const* ctxs, size_t count, uint32_t wordsPerWave, UnionParams* params)
{
    uint32_t at = 0;
    for (size_t m = 0; m < count; ++m) {
        params->slotOffsetDwords[m] = at;
        at += roundUp4(wordsPerWave * ctxs[m]->slotDwords);
        params->keyTileOffsetDwords[m] = at;
        at += roundUp4(params->model[m].keyTileDwords);
    }
    params->perWaveDwords = at;
}

// waves per block of a union kernel: most resident wavefronts per CU -- by LDS and by the kernel's registers --, blocks of
// four on ties (as chooseGeometry); 0 when no block size fits
hipError_t chooseUnionWaves(
    const memb_hip_ctx* first, const void* kernel, uint32_t sharedDwords, uint32_t perWaveDwords, uint32_t* waves, uint32_t* ldsBytes)
{
    KernelFacts facts;
    const hipError_t status = kernelFacts(kernel, &facts);
    uint32_t bestResident = 0;
    *waves = 0;
    // (a forced block size -- option waves_per_block, 1 .. 16 -- is the only candidate, as in chooseGeometry)
    const uint32_t forced = first->switches.waves;
    for (uint32_t candidate : {forced ? forced : 4u, 8u, 2u, 1u}) {
        if (forced && candidate != forced) {
            continue;
        }
        const uint32_t bytes = 4u * (sharedDwords + candidate * perWaveDwords);
        const uint32_t resident = residentWaves(first->ldsLimit, candidate, bytes, facts.registerWavesPerCu);
        if (resident > bestResident) {
            bestResident = resident;
            *waves = candidate;
            *ldsBytes = bytes;
        }
    }
    return status;
}

constexpr uint32_t ROWWISE_THREADS = 256;

uint32_t rowwiseWordsPerBlock(uint32_t dim)
{
    // about 16 KiB of output per block (one batch of pieces per thread), at least one word
    return std::max<uint32_t>(1, std::min<uint32_t>(ROWWISE_MAX_WORDS, 4096 / std::max<uint32_t>(dim, 1)));
}

// Whether a batch of this output shape runs dequant_uniform_tile (one tile per wavefront, row regions through LDS), and
// with what geometry: output pieces of 16 bytes, a tile's regions fitting LDS (blocks of four wavefronts, fewer for very
// wide rows), 32-bit piece numbers; option `persistent` = 0 keeps the block kernel (tests). launchUniform and
// memb_hip_ctx_get_info both ask here.
struct UniformTilePlan {
    bool tiled = false;
    uint32_t waves = 0;
    uint32_t tileWords = 0;
};

UniformTilePlan planUniform(const memb_hip_ctx* ctx, const Lookup& lookup)
{
    UniformTilePlan plan;
    // (fp32 only: a narrow uniform lookup runs the block kernel)
    const bool vec = lookup.outType == MEMB_HIP_OUT_F32 && outputMode(ctx->dim, lookup.ld, lookup.colOff, lookup.out, 4, 0) != OUT_SCALAR;
    plan.tileWords = std::max<uint32_t>(1, std::min<uint32_t>(WAVE, (9600 + ctx->dim * 4 - 1) / (ctx->dim * 4)));
    plan.waves = 4;
    while (plan.waves > 1 && uint64_t(plan.waves) * plan.tileWords * ctx->regionPieces * 16 > ctx->ldsLimit) {
        plan.waves /= 2;
    }
    plan.tiled = vec && ctx->switches.persistent != 0 && uint64_t(ctx->nRows + 1) * ctx->regionPieces < (1ull << 32) &&
        uint64_t(plan.waves) * plan.tileWords * ctx->regionPieces * 16 <= ctx->ldsLimit;
    return plan;
}

// The fields UniformParams and FullParams share.
template <typename Params>
Params rowwiseParams(const memb_hip_ctx* ctx, const Lookup& lookup)
{
    Params params{};
    params.accumulate = lookup.accumulate;
    params.divisor = lookup.divisor;
    params.rows = lookup.rows;
    params.out = static_cast<float*>(lookup.out);   // (2-byte elements for a narrow type)
    params.n = lookup.n;
    params.ld = lookup.ld;
    params.colOff = lookup.colOff;
    params.nRows = ctx->nRows;
    params.dim = ctx->dim;
    params.wordsPerBlock = rowwiseWordsPerBlock(ctx->dim);
    return params;
}
