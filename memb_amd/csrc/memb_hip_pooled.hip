// Pooled lookups (include/memb_hip_pooled.h, include/memb_hip_pooled_known.h): the sum or mean of each bag of rows, or of the
// rows of each bag that the model KNOWS, decoded and reduced in one kernel, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (launchPooled) through pooledKernel below (hip_pooled.h). A bag's rows never reach memory: per entry a kernel reads the
// row id and the row's compressed bytes, per bag it writes dim elements. The device code below the bodies of the trained
// kernels is hip_pooled_kernels.h's.
//   pool_trained<HAS_SUB, FAST, VEC4>                 fp32 rows          } decode_trained's stages up to the symbol tile
//   pool_trained_narrow<HAS_SUB, FAST, VEC4, OUT>     bf16 / fp16 rows   } (decodePoolTile), then accumulatePiece /
//   pool_known_trained<HAS_SUB, FAST, VEC4, OUT>      known rows only    } gatherColumn in place of outputTile. A wavefront
//                      owns a run of whole consecutive bags; consecutive bags are consecutive entries, so it decodes full
//                      tiles across bag boundaries and only the accumulation looks at the offsets (wave-uniform).
//                      Three bodies: one shared body does not compile to their instructions
//   pool_uniform, pool_full, pool_uniform_narrow<OUT>, pool_full_narrow<OUT>   poolBagOfWave: one wavefront per bag, lanes
//   pool_known_uniform<OUT>, pool_known_full<OUT>     poolKnownBagOfWave       own columns and loop over the bag's entries
// OUT is a MEMB_HIP_OUT_*. The contract is an ORDER: acc = v_begin, then acc = acc + v_i one entry after the other, each add
// one v_add_f32 (addRn: the packed forms flush subnormals on this part), then one correctly rounded division for the mean;
// a bf16 / fp16 element is that fp32 value rounded ONCE, to nearest even, as it is stored (hip_device_common.h: narrowBits).
// A lane owns its columns for the whole bag, so no value crosses lanes and nothing depends on launch geometry. Nothing is
// allocated, nothing but the bags' columns (and counts) is written, no atomics, no packed fp32 arithmetic.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_pooled.h"
#include "../../include/memb_hip_pooled_known.h"
#include "codec.h"
#include "hip_pooled.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

#include "hip_pooled_kernels.h"

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
        float* destination = bagDestination<MEMB_HIP_OUT_F32>(p, bag);
        if (end <= begin) {
            if (VEC4) {
                for (uint32_t c = lane; c < pieces; c += WAVE) {
                    storePiece<MEMB_HIP_OUT_F32>(destination, c, make_float4(0.f, 0.f, 0.f, 0.f));
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
                storePiece<MEMB_HIP_OUT_F32>(destination, lane, acc0);
            }
            if (lane + WAVE < pieces) {
                storePiece<MEMB_HIP_OUT_F32>(destination, lane + WAVE, acc1);
            }
        }
    }
}

// bf16 / fp16 rows: no partial sum passes through `out`, whose elements are narrow, and the codebook in LDS stays fp32.
//   VEC4   pool_trained's register accumulators of 16-byte pieces, stored as 8-byte pieces of four elements
//   else   the column form, for any dim and alignment: lane l keeps POOL_COLUMN_BLOCK fp32 accumulators, the columns
//          c0 + l + 64 j, and walks the bag once per block of 512 columns. A bag that spans tiles has its tiles decoded
//          again for every block after the first; dim <= 512 is one walk, as in pool_trained.
// Seven wavefronts per SIMD, which launchPooled plans for (ONE_TILE_WAVES_PER_CU): asked of the compiler (not of the fp32
// pool_trained, whose instructions the attribute changes), because the column form's eight accumulators, live across a
// tile's decode, otherwise end at 72-73 vector registers -- one more than seven wavefronts allow for two-level tables. It
// fits without scratch (tests/test_pooled_isa.py).
template <bool HAS_SUB, bool FAST, bool VEC4, int OUT>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void pool_trained_narrow(TrainedParams p, PoolParams pool)
{
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
    PoolTile tile;

#pragma nounroll
    for (unsigned long long bag = firstBag; bag < lastBag; ++bag) {
        unsigned long long begin, end;
        bagRange(pool, bag, p.n, &begin, &end);
        float* destination = bagDestination<OUT>(p, bag);
        if (end <= begin) {
            if (VEC4) {
                for (uint32_t c = lane; c < pieces; c += WAVE) {
                    storePiece<OUT>(destination, c, make_float4(0.f, 0.f, 0.f, 0.f));
                }
            } else {
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    storeColumn<OUT>(destination, c, 0.f);
                }
            }
            continue;
        }
        const float count = static_cast<float>(static_cast<uint32_t>(end - begin));
        if (VEC4) {
            float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
            bool started = false;
#pragma nounroll
            for (unsigned long long i = begin; i < end;) {
                if (i < tile.start || i >= tile.end) {
                    decodePoolTile<HAS_SUB, FAST>(p, mem, lane, i, max(runEnd, end), tile);
                }
                const unsigned long long upTo = min(end, tile.end);
                const uint32_t w0 = static_cast<uint32_t>(i - tile.start);
                const uint32_t w1 = static_cast<uint32_t>(upTo - tile.start);
                accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane, pieces - 1), started, acc0);
                if (pieces > WAVE) {
                    accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane + WAVE, pieces - 1), started, acc1);
                }
                started = true;
                i = upTo;
            }
            if (pool.mean) {
                acc0 = divide4(acc0, count);
                acc1 = divide4(acc1, count);
            }
            if (lane < pieces) {
                storePiece<OUT>(destination, lane, acc0);
            }
            if (lane + WAVE < pieces) {
                storePiece<OUT>(destination, lane + WAVE, acc1);
            }
        } else {
#pragma nounroll
            for (uint32_t c0 = 0; c0 < p.dim; c0 += POOL_COLUMN_BLOCK * WAVE) {
                float acc[POOL_COLUMN_BLOCK] = {};
                bool started = false;
#pragma nounroll
                for (unsigned long long i = begin; i < end;) {
                    if (i < tile.start || i >= tile.end) {
                        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, i, max(runEnd, end), tile);
                    }
                    const unsigned long long upTo = min(end, tile.end);
                    accumulateColumns<FAST>(
                        p, mem, tile, static_cast<uint32_t>(i - tile.start), static_cast<uint32_t>(upTo - tile.start), c0, lane,
                        started, acc);
                    started = true;
                    i = upTo;
                }
#pragma unroll
                for (int j = 0; j < POOL_COLUMN_BLOCK; ++j) {
                    const uint32_t c = c0 + j * WAVE + lane;
                    if (c < p.dim) {
                        storeColumn<OUT>(destination, c, pool.mean ? __fdiv_rn(acc[j], count) : acc[j]);
                    }
                }
            }
        }
    }
}

// pool_trained up to the symbol tile: full tiles across bag boundaries, unknown entries decode as missing rows. What
// differs is the accumulation. decodePoolTile leaves the tile's mask of missing words for EVERY key form (a byte-key symbol
// of a missing row is ZERO_KEY, which a centroid of 0.0 has too); a bag adds the known words of its range only -- the first
// one starts the sum, an unknown one adds nothing, not even +0.0 -- and counts them with a population count of that mask,
// carried across tiles. Mask, count, "this bag has started" and the walk over the known words are wave-uniform: scalar
// registers and uniform branches.
//   VEC4          register accumulators of 16-byte pieces (pool_trained's), stored as fp32 or narrowed pieces
//   else, fp32    the column form: partial sums parked in the bag's own columns of `out`, valid once a known entry has
//                 been seen; a bag that ends without one is written as zeros
//   else, narrow  register blocks of 512 columns, one walk of the bag each (pool_trained_narrow's); the count is taken on
//                 the first walk
// counts[bag] is one ordinary store of one lane. Seven wavefronts per SIMD, which launchPooled plans for
// (ONE_TILE_WAVES_PER_CU): asked of the compiler, as pool_trained_narrow does, for the forms that would otherwise end a
// register or two above it. No scratch (tests/test_pooled_isa.py).
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
        float* destination = bagDestination<OUT>(p, bag);
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
                        storeColumn<OUT>(destination, c, a);
                    }
                }
            }
        }
        if (counted.counts && lane == 0) {
            counted.counts[bag] = count;
        }
    }
}

// Uniform and full storage: one wavefront per bag.
__global__ void pool_uniform(UniformParams p, PoolParams pool)
{
    poolBagOfWave<MEMB_HIP_OUT_F32>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return uniformValue(p, row, c); });
}

__global__ void pool_full(FullParams p, PoolParams pool)
{
    poolBagOfWave<MEMB_HIP_OUT_F32>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return fullValue(p, row, c); });
}

template <int OUT>
__global__ void pool_uniform_narrow(UniformParams p, PoolParams pool)
{
    poolBagOfWave<OUT>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return uniformValue(p, row, c); });
}

template <int OUT>
__global__ void pool_full_narrow(FullParams p, PoolParams pool)
{
    poolBagOfWave<OUT>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return fullValue(p, row, c); });
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

constexpr int OUT_TYPES = 3;
static_assert(MEMB_HIP_OUT_F32 == 0 && MEMB_HIP_OUT_BF16 == 1 && MEMB_HIP_OUT_F16 == 2, "the tables are indexed by out type");

// Every instance of one family (KNOWN: the kernels that skip missing rows), indexed [HAS_SUB][FAST][VEC4][out type]
// (trained) and [out type]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and <true, false> byte
// keys (hip_kernel_table.h: KernelTable).
template <bool KNOWN>
struct PoolTable {
    const void* trained[2][2][2][OUT_TYPES] = {};
    const void* uniform[OUT_TYPES] = {};
    const void* full[OUT_TYPES] = {};

    PoolTable()
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
        if constexpr (KNOWN) {
            uniform[OUT] = reinterpret_cast<const void*>(&pool_known_uniform<OUT>);
            full[OUT] = reinterpret_cast<const void*>(&pool_known_full<OUT>);
        } else if constexpr (OUT == MEMB_HIP_OUT_F32) {
            uniform[OUT] = reinterpret_cast<const void*>(&pool_uniform);
            full[OUT] = reinterpret_cast<const void*>(&pool_full);
        } else {
            uniform[OUT] = reinterpret_cast<const void*>(&pool_uniform_narrow<OUT>);
            full[OUT] = reinterpret_cast<const void*>(&pool_full_narrow<OUT>);
        }
    }

    template <bool HAS_SUB, bool FAST, int OUT>
    void addKeyForm()
    {
        addForm<HAS_SUB, FAST, false, OUT>();
        addForm<HAS_SUB, FAST, true, OUT>();
    }

    template <bool HAS_SUB, bool FAST, bool VEC4, int OUT>
    void addForm()
    {
        if constexpr (KNOWN) {
            trained[HAS_SUB][FAST][VEC4][OUT] = reinterpret_cast<const void*>(&pool_known_trained<HAS_SUB, FAST, VEC4, OUT>);
        } else if constexpr (OUT == MEMB_HIP_OUT_F32) {
            trained[HAS_SUB][FAST][VEC4][OUT] = reinterpret_cast<const void*>(&pool_trained<HAS_SUB, FAST, VEC4>);
        } else {
            trained[HAS_SUB][FAST][VEC4][OUT] = reinterpret_cast<const void*>(&pool_trained_narrow<HAS_SUB, FAST, VEC4, OUT>);
        }
    }
};

template <bool KNOWN>
const void* kernelOf(memb_pooled::PoolStorage storage, bool hasSub, bool fast, bool vec4, int outType)
{
    static const PoolTable<KNOWN> table;
    switch (storage) {
        case memb_pooled::PoolStorage::Trained:
            return table.trained[hasSub][fast][vec4][outType];
        case memb_pooled::PoolStorage::Uniform:
            return table.uniform[outType];
        default:
            return table.full[outType];
    }
}

}  // namespace

namespace memb_pooled {

memb::KernelHandle pooledKernel(PoolStorage storage, bool hasSub, bool fast, bool vec4, int outType, bool known)
{
    static const char* const names[2][3] = {{"pool_trained", "pool_uniform", "pool_full"},
                                            {"pool_known_trained", "pool_known_uniform", "pool_known_full"}};
    memb::KernelHandle kernel{nullptr, names[known][static_cast<int>(storage)]};
    if (outType >= 0 && outType < OUT_TYPES) {
        kernel.address = known ? kernelOf<true>(storage, hasSub, fast, vec4, outType) : kernelOf<false>(storage, hasSub, fast, vec4, outType);
    }
    return kernel;
}

}  // namespace memb_pooled
