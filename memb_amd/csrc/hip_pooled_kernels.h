// Device code of the sequential pooled kernels (memb_hip_pooled.hip): a bag's entries and where its result goes, the
// symbol tile of a run of entries, the fp32 values gathered from it -- of every word or of the known ones --, the stores of
// a finished piece or column, and the row-wise bag loops. Included inside the unit's anonymous namespace, behind
// hip_device_common.h, hip_trained_kernels.h and hip_rowwise_kernels.h. Every accumulator here is fp32, whatever the
// element the result is stored as (OUT, a MEMB_HIP_OUT_*: a 2-byte element is the finished value rounded once, to
// nearest even, at its store).
#pragma once

using memb_pooled::KnownParams;
using memb_pooled::PoolParams;

constexpr int POOL_GATHER_BATCH = 4;   // entries whose values a lane gathers before it adds them one after the other
constexpr int POOL_COLUMN_BLOCK = 8;   // bf16 / fp16 column form: accumulators a lane keeps in registers, 512 columns per
                                       // walk of a bag

__device__ __forceinline__ float4 add4(float4 a, float4 b)
{
    return make_float4(addRn(a.x, b.x), addRn(a.y, b.y), addRn(a.z, b.z), addRn(a.w, b.w));
}

__device__ __forceinline__ float4 divide4(float4 a, float divisor)
{
    return make_float4(__fdiv_rn(a.x, divisor), __fdiv_rn(a.y, divisor), __fdiv_rn(a.z, divisor), __fdiv_rn(a.w, divisor));
}

// The entries [begin, end) of bag `bag`, clamped to the batch: whatever the offsets hold, no entry outside [0, n) exists.
__device__ __forceinline__ void bagRange(
    const PoolParams& pool, unsigned long long bag, unsigned long long n, unsigned long long* begin, unsigned long long* end)
{
    *begin = min(static_cast<unsigned long long>(pool.offsets[bag]), n);
    *end = min(static_cast<unsigned long long>(pool.offsets[bag + 1]), n);
}

// The tile of entries a wavefront holds decoded in its symbol tile: [start, end), word w of the tile = entry start + w.
struct PoolTile {
    unsigned long long start = 0;
    unsigned long long end = 0;
    unsigned long long absent = 0;       // nibble keys: bit w * lanesPerWord = word w is a missing row (outputTile's ballot);
                                         // every key form where decodePoolTile is asked for it (ABSENT_MASK)
    unsigned long long nextStart = ~0ull;   // the tile whose row ids are in flight already (nextRow), and its limit
    unsigned long long nextLimit = 0;
    uint32_t nextRow = MISSING;
};

// decodeTilesOfBlock's body for ONE tile that starts at ANY entry: row ids -> row regions -> LDS slots -> symbol tile.
// Entries from `limit` (<= n) on are not read; their words decode as missing rows. ABSENT_MASK: tile.absent is filled --
// what gatherPiece / gatherColumn need for nibble keys only, the kernels that skip missing rows for every key form.
template <bool HAS_SUB, bool FAST, bool ABSENT_MASK = FAST>
__device__ __forceinline__ void decodePoolTile(
    const TrainedParams& p, const WaveLds& mem, uint32_t lane, unsigned long long start, unsigned long long limit, PoolTile& tile)
{
    constexpr bool PACKED = !FAST;
    waveLdsFence();   // (the last tile's symbols have been read)
    asm volatile("" : "+v"(lane));   // (lane-derived values are worked out afresh per tile: decodeTilesOfBlock)
    const LaneRole role = laneRole(p, lane);
    const unsigned long long end = min(start + p.wordsPerWave, limit);
    uint32_t row = MISSING;
    if (tile.nextStart == start && tile.nextLimit == limit) {
        row = tile.nextRow;
    } else if (!role.spare && start + role.word < end) {
        row = p.rows[start + role.word];
    }
    tile.start = start;
    tile.end = end;
    WordMeta meta = loadWordMeta(p, row, role);
    unpackMeta(p, role, meta);
    StreamRegisters first = {};
    issueStreamLoads(p, meta, lane, 0, first);
    tile.nextStart = end;
    tile.nextLimit = limit;
    tile.nextRow = MISSING;
    if (!role.spare && end + role.word < limit) {
        tile.nextRow = p.rows[end + role.word];
    }
    writeStreams(p, mem.slots, lane, 0, first);
    const uint32_t rounds = (p.wordsPerWave * p.loadPieces + WAVE - 1) / WAVE;
    for (uint32_t round = STREAM_REGISTERS; round < rounds; round += STREAM_REGISTERS) {
        StreamRegisters v = {};
        issueStreamLoads(p, meta, lane, round, v);
        writeStreams(p, mem.slots, lane, round, v);
    }
    waveLdsFence();
    recordSegmentBits(p, mem.slots, role, meta);
    decodeSegment<HAS_SUB, OUT_VEC4, FAST, PACKED>(p, mem.table, mem.slots, mem.keyTile, role, meta);
    waveLdsFence();
    if (ABSENT_MASK) {
        tile.absent = __ballot(!(meta.row < p.nRows) && !role.spare && role.segment == 0);
    }
}

// The four values of piece c (columns 4 c ..) of word w of the symbol tile; +0.0 for a missing row (byte keys: its
// symbols are ZERO_KEY, whose centroid is 0.0f).
template <bool FAST>
__device__ __forceinline__ float4 gatherPiece(
    const TrainedParams& p, const WaveLds& mem, const PoolTile& tile, uint32_t w, uint32_t c)
{
    const uint32_t q = w * (p.dim / 4) + c;   // the symbol tile is linear in q (outputTile)
    if (FAST) {
        const float2* pairLds = reinterpret_cast<const float2*>(mem.codebook);
        const uint32_t k = reinterpret_cast<const uint16_t*>(mem.keyTile)[q];
        const float2 a = pairLds[k & 0xff];
        const float2 b = pairLds[k >> 8];
        if ((tile.absent >> (w * p.lanesPerWord)) & 1) {   // wave-uniform
            return make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return make_float4(a.x, a.y, b.x, b.y);
    }
    const float* centroidLds = reinterpret_cast<const float*>(mem.codebook);
    const uint32_t k = mem.keyTile[q];
    return make_float4(centroidLds[k & 0xff], centroidLds[(k >> 8) & 0xff], centroidLds[(k >> 16) & 0xff], centroidLds[k >> 24]);
}

// acc (+)= words [w0, w1) of the tile, in that order, for the lane's piece c. started: acc holds earlier entries of the bag.
template <bool FAST>
__device__ __forceinline__ void accumulatePiece(
    const TrainedParams& p, const WaveLds& mem, const PoolTile& tile, uint32_t w0, uint32_t w1, uint32_t c, bool started,
    float4& acc)
{
    if (!started) {
        acc = gatherPiece<FAST>(p, mem, tile, w0, c);
        ++w0;
    }
    for (uint32_t w = w0; w < w1; w += POOL_GATHER_BATCH) {
        float4 v[POOL_GATHER_BATCH];
#pragma unroll
        for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
            v[u] = gatherPiece<FAST>(p, mem, tile, min(w + u, w1 - 1), c);
        }
#pragma unroll
        for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
            if (w + u < w1) {   // wave-uniform
                acc = add4(acc, v[u]);
            }
        }
    }
}

// One value of the symbol tile: column c of word w (outputTile's scalar form).
template <bool FAST>
__device__ __forceinline__ float gatherColumn(
    const TrainedParams& p, const WaveLds& mem, const PoolTile& tile, uint32_t w, uint32_t c)
{
    const uint8_t* keyBytes = reinterpret_cast<const uint8_t*>(mem.keyTile);
    if (FAST) {
        // a lone nibble n indexes the pair of key byte n: (centroid n, centroid 0)
        const uint32_t k = keyBytes[w * p.keyRowBytes + (c >> 1)];
        const float value = reinterpret_cast<const float2*>(mem.codebook)[(k >> (4 * (c & 1))) & 15].x;
        return ((tile.absent >> (w * p.lanesPerWord)) & 1) ? 0.f : value;
    }
    return reinterpret_cast<const float*>(mem.codebook)[keyBytes[w * p.keyRowBytes + c]];
}

// Where bag `bag` goes: its first column in `out`, whose elements are OUT's (ld, colOff: in elements). A float pointer
// whatever the element: storePiece / storeColumn know what lies behind it.
template <int OUT, typename Params>
__device__ __forceinline__ float* bagDestination(const Params& p, unsigned long long bag)
{
    if constexpr (OUT == MEMB_HIP_OUT_F32) {
        return p.out + bag * p.ld + p.colOff;
    } else {
        return reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(p.out) + bag * p.ld + p.colOff);
    }
}

// Piece `piece` (four elements) of a bag's row: 16 bytes of fp32, 8 bytes of bf16 / fp16.
template <int OUT>
__device__ __forceinline__ void storePiece(float* destination, uint32_t piece, float4 v)
{
    if constexpr (OUT == MEMB_HIP_OUT_F32) {
        *reinterpret_cast<float4*>(destination + 4 * piece) = v;
    } else {
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(destination) + 4 * piece) =
            make_uint2(narrowPair<OUT>(v.x, v.y), narrowPair<OUT>(v.z, v.w));
    }
}

template <int OUT>
__device__ __forceinline__ void storeColumn(float* destination, uint32_t c, float a)
{
    if constexpr (OUT == MEMB_HIP_OUT_F32) {
        destination[c] = a;
    } else {
        reinterpret_cast<uint16_t*>(destination)[c] = static_cast<uint16_t>(narrowBits<OUT>(a));
    }
}

// The known words among [w0, w1) of the tile, bit w * lanesPerWord for word w (w0 < w1 <= wordsPerWave). heads: those bits
// of every word of a tile. Wave-uniform, like everything derived from it.
__device__ __forceinline__ unsigned long long knownWords(
    const TrainedParams& p, const PoolTile& tile, unsigned long long heads, uint32_t w0, uint32_t w1)
{
    const uint32_t low = w0 * p.lanesPerWord;    // < 64
    const uint32_t high = w1 * p.lanesPerWord;   // <= 64
    const unsigned long long mask = heads & ~tile.absent & (~0ull << low);
    return high < 64 ? mask & ~(~0ull << high) : mask;
}

// The part of a bag that lies in one tile: entries [i, upTo) = words [w0, w1) of the tile, `known` their known words.
struct KnownRange {
    unsigned long long upTo;
    uint32_t w0;
    uint32_t w1;
    unsigned long long known;
};

// The range of the bag [.., end) that starts at entry i; decodes the tile that holds i where the wavefront does not hold
// it (limit: decodePoolTile's). The known kernels' walk: the plain ones spell theirs out, without the mask.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ KnownRange knownRange(
    const TrainedParams& p, const WaveLds& mem, uint32_t lane, unsigned long long heads, unsigned long long i,
    unsigned long long end, unsigned long long limit, PoolTile& tile)
{
    if (i < tile.start || i >= tile.end) {
        decodePoolTile<HAS_SUB, FAST, true>(p, mem, lane, i, limit, tile);
    }
    KnownRange range;
    range.upTo = min(end, tile.end);
    range.w0 = static_cast<uint32_t>(i - tile.start);
    range.w1 = static_cast<uint32_t>(range.upTo - tile.start);
    range.known = knownWords(p, tile, heads, range.w0, range.w1);
    return range;
}

// acc[j] (+)= column c0 + 64 j + lane of words [w0, w1) of the tile, in that order. started: acc holds earlier entries
// of the bag. Lanes past the last column work on column dim - 1 and store nothing.
template <bool FAST>
__device__ __forceinline__ void accumulateColumns(
    const TrainedParams& p, const WaveLds& mem, const PoolTile& tile, uint32_t w0, uint32_t w1, uint32_t c0, uint32_t lane,
    bool started, float (&acc)[POOL_COLUMN_BLOCK])
{
#pragma unroll
    for (int j = 0; j < POOL_COLUMN_BLOCK; ++j) {
        if (c0 + j * WAVE < p.dim) {   // wave-uniform
            uint32_t c = min(c0 + j * WAVE + lane, p.dim - 1);
            asm volatile("" : "+v"(c));   // (worked out here, block by block: eight columns' addresses kept live cost a wavefront per SIMD)
            uint32_t w = w0;
            float a = acc[j];
            if (!started) {
                a = gatherColumn<FAST>(p, mem, tile, w, c);
                ++w;
            }
            for (; w < w1; ++w) {
                a = addRn(a, gatherColumn<FAST>(p, mem, tile, w, c));
            }
            acc[j] = a;
        }
    }
}

// The first known word from w on, or w1 where there is none (known: knownWords of a range that ends at w1).
__device__ __forceinline__ uint32_t nextKnown(const TrainedParams& p, unsigned long long known, uint32_t w, uint32_t w1)
{
    while (w < w1 && !((known >> (w * p.lanesPerWord)) & 1)) {
        ++w;
    }
    return w;
}

// accumulatePiece / accumulateColumns over the known words of [w0, w1) (at least one): acc (+)= their values in order,
// POOL_GATHER_BATCH of them gathered before they are added. started: acc holds earlier entries of the bag.
// gather(w): the lane's value of word w; add: add4 for a piece, addRn for a column.
template <typename T, typename Gather, typename Add>
__device__ __forceinline__ void accumulateKnown(
    const TrainedParams& p, unsigned long long known, uint32_t w0, uint32_t w1, bool started, T& acc, Gather gather, Add add)
{
    uint32_t w = nextKnown(p, known, w0, w1);
    if (!started) {
        acc = gather(w);
        w = nextKnown(p, known, w + 1, w1);
    }
    while (w < w1) {
        uint32_t at[POOL_GATHER_BATCH];
        T v[POOL_GATHER_BATCH];
#pragma unroll
        for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
            at[u] = w;
            if (w < w1) {
                w = nextKnown(p, known, w + 1, w1);
            }
        }
#pragma unroll
        for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
            v[u] = gather(at[u] < w1 ? at[u] : at[0]);
        }
#pragma unroll
        for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
            if (at[u] < w1) {   // wave-uniform
                acc = add(acc, v[u]);
            }
        }
    }
}

// (known words only: gatherPiece / gatherColumn are handed a tile with no missing row to blank)
template <bool FAST>
__device__ __forceinline__ void accumulateKnownPiece(
    const TrainedParams& p, const WaveLds& mem, unsigned long long known, uint32_t w0, uint32_t w1, uint32_t c, bool started,
    float4& acc)
{
    const PoolTile present;
    accumulateKnown(
        p, known, w0, w1, started, acc, [&](uint32_t w) { return gatherPiece<FAST>(p, mem, present, w, c); },
        [](float4 a, float4 b) { return add4(a, b); });
}

template <bool FAST>
__device__ __forceinline__ void accumulateKnownColumn(
    const TrainedParams& p, const WaveLds& mem, unsigned long long known, uint32_t w0, uint32_t w1, uint32_t c, bool started,
    float& acc)
{
    const PoolTile present;
    accumulateKnown(
        p, known, w0, w1, started, acc, [&](uint32_t w) { return gatherColumn<FAST>(p, mem, present, w, c); },
        [](float a, float b) { return addRn(a, b); });
}

// Uniform and full storage: one wavefront per bag. Lane l owns the columns l, l + 64, ...; per column it walks the bag's
// entries in order (the row ids are wave-uniform loads), POOL_GATHER_BATCH value loads in flight before it adds them.
// value(row, c): column c of row `row` as memb_hip_decode_rows_device writes it (+0.0 for a row that is not in the model).
template <int OUT, typename Params, typename Value>
__device__ __forceinline__ void poolBagOfWave(const Params& p, const PoolParams& pool, Value value)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long bag =
        static_cast<unsigned long long>(blockIdx.x) * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    if (bag >= pool.bags) {
        return;
    }
    unsigned long long begin, end;
    bagRange(pool, bag, p.n, &begin, &end);
    float* destination = bagDestination<OUT>(p, bag);
    const float count = static_cast<float>(static_cast<uint32_t>(end - begin));
    for (uint32_t c0 = 0; c0 < p.dim; c0 += WAVE) {
        const uint32_t c = min(c0 + lane, p.dim - 1);
        float a = 0.f;
        if (end > begin) {
            a = value(p.rows[begin], c);
            for (unsigned long long i = begin + 1; i < end; i += POOL_GATHER_BATCH) {
                float v[POOL_GATHER_BATCH];
#pragma unroll
                for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
                    v[u] = value(p.rows[min(i + u, end - 1)], c);
                }
#pragma unroll
                for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
                    if (i + u < end) {
                        a = addRn(a, v[u]);
                    }
                }
            }
            if (pool.mean) {
                a = __fdiv_rn(a, count);
            }
        }
        if (c0 + lane < p.dim) {
            storeColumn<OUT>(destination, c0 + lane, a);
        }
    }
}

// poolBagOfWave over the entries the model knows. The row ids are wave-uniform loads, POOL_GATHER_BATCH of them at a time
// (the first one among them, where poolBagOfWave takes it ahead of the batches); value() loads nothing for an id that is
// not in the model and a uniform branch leaves it out of the sum.
template <int OUT, typename Params, typename Value>
__device__ __forceinline__ void poolKnownBagOfWave(const Params& p, const PoolParams& pool, const KnownParams& counted, Value value)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long bag =
        static_cast<unsigned long long>(blockIdx.x) * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    if (bag >= pool.bags) {
        return;
    }
    unsigned long long begin, end;
    bagRange(pool, bag, p.n, &begin, &end);
    float* destination = bagDestination<OUT>(p, bag);
    for (uint32_t c0 = 0; c0 < p.dim; c0 += WAVE) {
        const uint32_t c = min(c0 + lane, p.dim - 1);
        float a = 0.f;
        uint32_t count = 0;
        for (unsigned long long i = begin; i < end; i += POOL_GATHER_BATCH) {
            uint32_t row[POOL_GATHER_BATCH];
            float v[POOL_GATHER_BATCH];
#pragma unroll
            for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
                row[u] = p.rows[min(i + u, end - 1)];
                v[u] = value(row[u], c);
            }
#pragma unroll
            for (int u = 0; u < POOL_GATHER_BATCH; ++u) {
                if (i + u < end && row[u] < p.nRows) {   // wave-uniform
                    a = count ? addRn(a, v[u]) : v[u];
                    ++count;
                }
            }
        }
        if (pool.mean && count) {
            a = __fdiv_rn(a, static_cast<float>(count));
        }
        if (c0 + lane < p.dim) {
            storeColumn<OUT>(destination, c0 + lane, a);
        }
        if (c0 == 0 && counted.counts && lane == 0) {
            counted.counts[bag] = count;
        }
    }
}

// Column c of row `row` of a uniform / full model, as dequant_uniform / gather_full write it.
__device__ __forceinline__ float uniformValue(const UniformParams& p, uint32_t row, uint32_t c)
{
    if (!(row < p.nRows)) {
        return 0.f;
    }
    const uint8_t* region = uniformRegion(p, row);
    const float2 mm = *reinterpret_cast<const float2*>(region);
    return dequant(mm.x, subRn(mm.y, mm.x), region[16 + c], p.levels);   // dequant_uniform's expression
}

__device__ __forceinline__ float fullValue(const FullParams& p, uint32_t row, uint32_t c)
{
    return row < p.nRows ? p.values[static_cast<unsigned long long>(row) * p.dim + c] : 0.f;
}
