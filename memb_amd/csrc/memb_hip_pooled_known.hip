// Pooled lookups over the rows a model KNOWS (include/memb_hip_pooled_known.h): the sum or mean of each bag's known
// entries, and their count, decoded and reduced in one kernel, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip_pooled.hip and memb_hip_pooled_narrow.hip,
// whose device code it shares (hip_pooled_kernels.h); memb_hip.hip plans and launches these kernels (launchPooled) through
// the addresses below (hip_pooled_known.h).
//   pool_known_trained<HAS_SUB, FAST, VEC4, OUT>
//       pool_trained up to the symbol tile: full tiles across bag boundaries, unknown entries decode as missing rows. What
//       differs is the accumulation. decodePoolTile leaves the tile's mask of missing words for EVERY key form (a byte-key
//       symbol of a missing row is ZERO_KEY, which a centroid of 0.0 has too); a bag adds the known words of its range
//       only -- the first one starts the sum, an unknown one adds nothing, not even +0.0 -- and counts them with a population
//       count of that mask, carried across tiles. Mask, count, "this bag has started" and the walk over the known words
//       are wave-uniform: scalar registers and uniform branches.
//       VEC4          register accumulators of 16-byte pieces (pool_trained's), stored as fp32 or narrowed pieces
//       else, fp32    the column form: partial sums parked in the bag's own columns of `out`, valid once a known entry
//                     has been seen; a bag that ends without one is written as zeros
//       else, narrow  register blocks of 512 columns, one walk of the bag each (pool_trained_narrow's); the count is taken
//                     on the first walk
//   pool_known_uniform<OUT> / pool_known_full<OUT>   one wavefront per bag; row ids are wave-uniform loads and an unknown id
//                     is skipped by a uniform branch
// OUT is a MEMB_HIP_OUT_*: every sum is fp32, a bf16 / fp16 element is the finished value rounded once at its store.
// counts[bag] is one ordinary store of one lane. No atomics, no value crosses lanes, no packed fp32 arithmetic.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_pooled_known.h"
#include "codec.h"
#include "hip_pooled_known.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

#include "hip_pooled_kernels.h"

using memb_pooled::KnownParams;

constexpr int POOL_COLUMN_BLOCK = 8;   // narrow column form: accumulators a lane keeps in registers (512 columns per walk)

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

// The part of a bag that lies in one tile: entries [i, upTo) = words [w0, w1) of the tile, `known` their known words.
struct KnownRange {
    unsigned long long upTo;
    uint32_t w0;
    uint32_t w1;
    unsigned long long known;
};

// The range of the bag [.., end) that starts at entry i; decodes the tile that holds i where the wavefront does not hold
// it (limit: decodePoolTile's).
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

template <int OUT>
__device__ __forceinline__ void storePiece(float* destination, uint32_t piece, float4 v)
{
    if constexpr (OUT == MEMB_HIP_OUT_F32) {
        *reinterpret_cast<float4*>(destination + 4 * piece) = v;
    } else {   // (destination: 2-byte elements)
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(destination) + 4 * piece) =
            make_uint2(narrowPair<OUT>(v.x, v.y), narrowPair<OUT>(v.z, v.w));
    }
}

// Seven wavefronts per SIMD, which launchPooled plans for (ONE_TILE_WAVES_PER_CU): asked of the compiler, as
// pool_trained_narrow does, for the forms that would otherwise end a register or two above it. No scratch
// (tests/test_pooled_known_isa.py).
template <bool HAS_SUB, bool FAST, bool VEC4, int OUT>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void pool_known_trained(
    TrainedParams p, PoolParams pool, KnownParams counted)
{
    constexpr bool F32 = OUT == MEMB_HIP_OUT_F32;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);   // (the fp32 codebook: sums are of fp32 centroids)
    const unsigned long long firstBag =
        (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pool.bagsPerWave;
    if (firstBag >= pool.bags) {
        return;
    }
    const unsigned long long lastBag = min(firstBag + pool.bagsPerWave, pool.bags);
    // where this wavefront's entries end while the offsets ascend: tiles are not decoded past it
    const unsigned long long runEnd = min(static_cast<unsigned long long>(pool.offsets[lastBag]), p.n);
    const uint32_t pieces = p.dim / 4;
    const LaneRole ownRole = laneRole(p, lane);
    const unsigned long long heads = __ballot(!ownRole.spare && ownRole.segment == 0);
    PoolTile tile;

#pragma nounroll
    for (unsigned long long bag = firstBag; bag < lastBag; ++bag) {
        unsigned long long begin, end;
        bagRange(pool, bag, p.n, &begin, &end);
        // (ld, colOff: in elements of OUT)
        float* destination = F32 ? p.out + bag * p.ld + p.colOff
                                 : reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(p.out) + bag * p.ld + p.colOff);
        uint32_t count = 0;   // the bag's known entries so far
        if constexpr (VEC4) {
            float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma nounroll
            for (unsigned long long i = begin; i < end;) {
                const KnownRange range = knownRange<HAS_SUB, FAST>(p, mem, lane, heads, i, end, max(runEnd, end), tile);
                if (range.known) {
                    accumulateKnownPiece<FAST>(p, mem, range.known, range.w0, range.w1, min(lane, pieces - 1), count != 0, acc0);
                    if (pieces > WAVE) {
                        accumulateKnownPiece<FAST>(p, mem, range.known, range.w0, range.w1, min(lane + WAVE, pieces - 1), count != 0, acc1);
                    }
                    count += __builtin_popcountll(range.known);
                }
                i = range.upTo;
            }
            if (pool.mean && count) {
                acc0 = divide4(acc0, static_cast<float>(count));
                acc1 = divide4(acc1, static_cast<float>(count));
            }
            if (lane < pieces) {
                storePiece<OUT>(destination, lane, acc0);
            }
            if (lane + WAVE < pieces) {
                storePiece<OUT>(destination, lane + WAVE, acc1);
            }
        } else if constexpr (F32) {
            bool divided = false;   // the mean's division went with the last store already
#pragma nounroll
            for (unsigned long long i = begin; i < end;) {
                const KnownRange range = knownRange<HAS_SUB, FAST>(p, mem, lane, heads, i, end, max(runEnd, end), tile);
                if (range.known) {
                    const bool started = count != 0;
                    count += __builtin_popcountll(range.known);
                    divided = range.upTo == end && pool.mean;
                    for (uint32_t c = lane; c < p.dim; c += WAVE) {
                        float a = 0.f;
                        if (started) {
                            a = destination[c];   // (parked there by this lane)
                        }
                        accumulateKnownColumn<FAST>(p, mem, range.known, range.w0, range.w1, c, started, a);
                        destination[c] = divided ? __fdiv_rn(a, static_cast<float>(count)) : a;
                    }
                }
                i = range.upTo;
            }
            if (!count) {
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    destination[c] = 0.f;
                }
            } else if (pool.mean && !divided) {   // the bag's last tile held none of its known entries
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    destination[c] = __fdiv_rn(destination[c], static_cast<float>(count));
                }
            }
        } else {
            uint16_t* narrowDestination = reinterpret_cast<uint16_t*>(destination);
#pragma nounroll
            for (uint32_t c0 = 0; c0 < p.dim; c0 += POOL_COLUMN_BLOCK * WAVE) {
                float acc[POOL_COLUMN_BLOCK] = {};
                bool started = false;
#pragma nounroll
                for (unsigned long long i = begin; i < end;) {
                    const KnownRange range = knownRange<HAS_SUB, FAST>(p, mem, lane, heads, i, end, max(runEnd, end), tile);
                    if (range.known) {
#pragma unroll
                        for (int j = 0; j < POOL_COLUMN_BLOCK; ++j) {
                            if (c0 + j * WAVE < p.dim) {   // wave-uniform
                                uint32_t c = min(c0 + j * WAVE + lane, p.dim - 1);
                                asm volatile("" : "+v"(c));   // (worked out here, block by block: accumulateColumns)
                                accumulateKnownColumn<FAST>(p, mem, range.known, range.w0, range.w1, c, started, acc[j]);
                            }
                        }
                        started = true;
                        if (c0 == 0) {   // the count is taken once, on the first walk
                            count += __builtin_popcountll(range.known);
                        }
                    }
                    i = range.upTo;
                }
#pragma unroll
                for (int j = 0; j < POOL_COLUMN_BLOCK; ++j) {
                    const uint32_t c = c0 + j * WAVE + lane;
                    if (c < p.dim) {
                        const float a = pool.mean && count ? __fdiv_rn(acc[j], static_cast<float>(count)) : acc[j];
                        narrowDestination[c] = static_cast<uint16_t>(narrowBits<OUT>(a));
                    }
                }
            }
        }
        if (counted.counts && lane == 0) {
            counted.counts[bag] = count;
        }
    }
}

// Uniform and full storage: poolBagOfWave over the known entries. The row ids are wave-uniform loads, POOL_GATHER_BATCH of
// them at a time; value() loads nothing for an id that is not in the model and a uniform branch leaves it out of the sum.
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
    float* destination = p.out + bag * p.ld + p.colOff;
    uint16_t* narrowDestination = reinterpret_cast<uint16_t*>(p.out) + bag * p.ld + p.colOff;   // (ld, colOff: in elements)
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
            if constexpr (OUT == MEMB_HIP_OUT_F32) {
                destination[c0 + lane] = a;
            } else {
                narrowDestination[c0 + lane] = static_cast<uint16_t>(narrowBits<OUT>(a));
            }
        }
        if (c0 == 0 && counted.counts && lane == 0) {
            counted.counts[bag] = count;
        }
    }
}

template <int OUT>
__global__ void pool_known_uniform(UniformParams p, PoolParams pool, KnownParams counted)
{
    poolKnownBagOfWave<OUT>(p, pool, counted, [&p](uint32_t row, uint32_t c) -> float { return uniformValue(p, row, c); });
}

template <int OUT>
__global__ void pool_known_full(FullParams p, PoolParams pool, KnownParams counted)
{
    poolKnownBagOfWave<OUT>(p, pool, counted, [&p](uint32_t row, uint32_t c) -> float { return fullValue(p, row, c); });
}

// Every instance, indexed [HAS_SUB][FAST][VEC4][out type] (trained) and [out type].
struct KnownPoolTable {
    const void* trained[2][2][2][3] = {};
    const void* uniform[3] = {};
    const void* full[3] = {};

    KnownPoolTable()
    {
        addType<MEMB_HIP_OUT_F32>();
        addType<MEMB_HIP_OUT_BF16>();
        addType<MEMB_HIP_OUT_F16>();
    }

private:
    template <int OUT>
    void addType()
    {
        addKeyForm<false, true, OUT>();
        addKeyForm<false, false, OUT>();
        addKeyForm<true, false, OUT>();
        uniform[OUT] = reinterpret_cast<const void*>(&pool_known_uniform<OUT>);
        full[OUT] = reinterpret_cast<const void*>(&pool_known_full<OUT>);
    }

    template <bool HAS_SUB, bool FAST, int OUT>
    void addKeyForm()
    {
        trained[HAS_SUB][FAST][0][OUT] = reinterpret_cast<const void*>(&pool_known_trained<HAS_SUB, FAST, false, OUT>);
        trained[HAS_SUB][FAST][1][OUT] = reinterpret_cast<const void*>(&pool_known_trained<HAS_SUB, FAST, true, OUT>);
    }
};

const KnownPoolTable& knownPoolTable()
{
    static const KnownPoolTable table;
    return table;
}

bool knownType(int outType)
{
    return outType == MEMB_HIP_OUT_F32 || outType == MEMB_HIP_OUT_BF16 || outType == MEMB_HIP_OUT_F16;
}

}  // namespace

namespace memb_pooled {

const void* trainedKernelKnown(bool hasSub, bool fast, bool vec4, int outType)
{
    return knownType(outType) ? knownPoolTable().trained[hasSub][fast][vec4][outType] : nullptr;
}

const void* uniformKernelKnown(int outType)
{
    return knownType(outType) ? knownPoolTable().uniform[outType] : nullptr;
}

const void* fullKernelKnown(int outType)
{
    return knownType(outType) ? knownPoolTable().full[outType] : nullptr;
}

}  // namespace memb_pooled
