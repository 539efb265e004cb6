// Pooled lookups (include/memb_hip_pooled.h): the sum or mean of each bag of rows, decoded and reduced in one kernel,
// gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (launchPooled) through the addresses below (hip_pooled.h). A bag's rows never reach memory: per entry a kernel reads
// the row id and the row's compressed bytes, per bag it writes dim floats.
//   pool_trained<HAS_SUB, FAST, VEC4>  decode_trained's stages up to the symbol tile (hip_trained_kernels.h: row ids ->
//                      row regions -> LDS -> decodeSegment), then accumulatePiece / gatherColumn in place of outputTile. A wavefront owns
//                      a run of whole consecutive bags; consecutive bags are consecutive entries, so it decodes full
//                      tiles across bag boundaries and only the accumulation looks at the offsets (wave-uniform).
//   pool_uniform / pool_full           one wavefront per bag, lanes own columns and loop over the bag's entries
// The contract is an ORDER: acc = v_begin, then acc = acc + v_i one entry after the other, each add one v_add_f32 (addRn:
// the packed forms flush subnormals on this part), then one correctly rounded division for the mean. A lane owns its
// columns for the whole bag, so no value crosses lanes and nothing depends on launch geometry.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_pooled.h"
#include "codec.h"
#include "hip_pooled.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

using memb_pooled::PoolParams;

constexpr int POOL_GATHER_BATCH = 4;   // entries whose values a lane gathers before it adds them one after the other

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
    unsigned long long absent = 0;       // nibble keys: bit w * lanesPerWord = word w is a missing row (outputTile's ballot)
    unsigned long long nextStart = ~0ull;   // the tile whose row ids are in flight already (nextRow), and its limit
    unsigned long long nextLimit = 0;
    uint32_t nextRow = MISSING;
};

// decodeTilesOfBlock's body for ONE tile that starts at ANY entry: row ids -> row regions -> LDS slots -> symbol tile.
// Entries from `limit` (<= n) on are not read; their words decode as missing rows.
template <bool HAS_SUB, bool FAST>
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
    if (FAST) {
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

// VEC4: lane l owns the 16-byte pieces l and l + 64 of a bag's row in registers (dim <= TRAINED_VEC4_MAX_DIM). Else, for any
// dim, lane l owns the columns l, l + 64, ... and a bag that spans tiles keeps its partial sums where its result goes: in
// the bag's own columns of `out`, each written and read back by its own lane only (a thread's load sees its earlier store).
template <bool HAS_SUB, bool FAST, bool VEC4>
__global__ MEMB_SGPR_BUDGET void pool_trained(TrainedParams p, PoolParams pool)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long firstBag =
        (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pool.bagsPerWave;
    if (firstBag >= pool.bags) {
        return;
    }
    const unsigned long long lastBag = min(firstBag + pool.bagsPerWave, pool.bags);
    // where this wavefront's entries end while the offsets ascend: tiles are not decoded past it
    const unsigned long long runEnd = min(static_cast<unsigned long long>(pool.offsets[lastBag]), p.n);
    const uint32_t pieces = p.dim / 4;
    PoolTile tile;
    float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);

#pragma nounroll
    for (unsigned long long bag = firstBag; bag < lastBag; ++bag) {
        unsigned long long begin, end;
        bagRange(pool, bag, p.n, &begin, &end);
        float* destination = p.out + bag * p.ld + p.colOff;
        if (end <= begin) {
            if (VEC4) {
                for (uint32_t c = lane; c < pieces; c += WAVE) {
                    *reinterpret_cast<float4*>(destination + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    destination[c] = 0.f;
                }
            }
            continue;
        }
        const float count = static_cast<float>(static_cast<uint32_t>(end - begin));
        bool started = false;
#pragma nounroll
        for (unsigned long long i = begin; i < end;) {
            if (i < tile.start || i >= tile.end) {
                decodePoolTile<HAS_SUB, FAST>(p, mem, lane, i, max(runEnd, end), tile);
            }
            const unsigned long long upTo = min(end, tile.end);
            const uint32_t w0 = static_cast<uint32_t>(i - tile.start);
            const uint32_t w1 = static_cast<uint32_t>(upTo - tile.start);
            if (VEC4) {
                accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane, pieces - 1), started, acc0);
                if (pieces > WAVE) {
                    accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane + WAVE, pieces - 1), started, acc1);
                }
            } else {
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    uint32_t w = w0;
                    float a;
                    if (started) {
                        a = destination[c];
                    } else {
                        a = gatherColumn<FAST>(p, mem, tile, w, c);
                        ++w;
                    }
                    for (; w < w1; ++w) {
                        a = addRn(a, gatherColumn<FAST>(p, mem, tile, w, c));
                    }
                    destination[c] = upTo == end && pool.mean ? __fdiv_rn(a, count) : a;
                }
            }
            started = true;
            i = upTo;
        }
        if (VEC4) {
            if (pool.mean) {
                acc0 = divide4(acc0, count);
                acc1 = divide4(acc1, count);
            }
            if (lane < pieces) {
                *reinterpret_cast<float4*>(destination + 4 * lane) = acc0;
            }
            if (lane + WAVE < pieces) {
                *reinterpret_cast<float4*>(destination + 4 * (lane + WAVE)) = acc1;
            }
        }
    }
}

// Uniform and full storage: one wavefront per bag. Lane l owns the columns l, l + 64, ...; per column it walks the bag's
// entries in order (the row ids are wave-uniform loads), POOL_GATHER_BATCH value loads in flight before it adds them.
// value(row, c): column c of row `row` as memb_hip_decode_rows_device writes it (+0.0 for a row that is not in the model).
template <typename Params, typename Value>
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
    float* destination = p.out + bag * p.ld + p.colOff;
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
            destination[c0 + lane] = a;
        }
    }
}

__global__ void pool_uniform(UniformParams p, PoolParams pool)
{
    poolBagOfWave(p, pool, [&p](uint32_t row, uint32_t c) -> float {
        if (!(row < p.nRows)) {
            return 0.f;
        }
        const uint8_t* region = uniformRegion(p, row);
        const float2 mm = *reinterpret_cast<const float2*>(region);
        return dequant(mm.x, subRn(mm.y, mm.x), region[16 + c], p.levels);   // dequant_uniform's expression
    });
}

__global__ void pool_full(FullParams p, PoolParams pool)
{
    poolBagOfWave(p, pool, [&p](uint32_t row, uint32_t c) -> float {
        return row < p.nRows ? p.values[static_cast<unsigned long long>(row) * p.dim + c] : 0.f;
    });
}

}  // namespace

namespace memb_pooled {

const void* trainedKernel(bool hasSub, bool fast, bool vec4)
{
    // key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and <true, false> byte keys (memb_hip.hip: KernelTable)
    static const void* const table[2][2][2] = {
        {{reinterpret_cast<const void*>(&pool_trained<false, false, false>), reinterpret_cast<const void*>(&pool_trained<false, false, true>)},
         {reinterpret_cast<const void*>(&pool_trained<false, true, false>), reinterpret_cast<const void*>(&pool_trained<false, true, true>)}},
        {{reinterpret_cast<const void*>(&pool_trained<true, false, false>), reinterpret_cast<const void*>(&pool_trained<true, false, true>)},
         {nullptr, nullptr}}};
    return table[hasSub][fast][vec4];
}

const void* uniformKernel()
{
    return reinterpret_cast<const void*>(&pool_uniform);
}

const void* fullKernel()
{
    return reinterpret_cast<const void*>(&pool_full);
}

}  // namespace memb_pooled
