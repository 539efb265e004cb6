// Pooled lookups straight into bf16 / fp16 rows (include/memb_hip_pooled.h: memb_hip_pool_rows_device_typed), gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip_pooled.hip, whose device code it shares
// (hip_pooled_kernels.h); memb_hip.hip plans and launches these kernels (launchPooled) through the addresses below
// (hip_pooled.h). Every value is the fp32 value of the float kernels -- the same adds in the same order, the same one
// division -- rounded ONCE, to nearest even, as it is stored (hip_device_common.h: narrowBits). So the codebook in LDS
// stays fp32 (unlike decode_trained_narrow's), and no partial sum ever passes through `out`, whose elements are narrow:
//   pool_trained_narrow<HAS_SUB, FAST, VEC4, OUT>
//       VEC4   pool_trained's register accumulators of 16-byte pieces, stored as 8-byte pieces of four elements
//       else   the column form, for any dim and alignment: lane l keeps POOL_COLUMN_BLOCK fp32 accumulators, the columns
//              c0 + l + 64 j, and walks the bag once per block of 512 columns. A bag that spans tiles has its tiles decoded
//              again for every block after the first; dim <= 512 is one walk, as in pool_trained.
//   pool_uniform_narrow<OUT> / pool_full_narrow<OUT>   poolBagOfWave with the narrowing store
// OUT is MEMB_HIP_OUT_BF16 or MEMB_HIP_OUT_F16. Nothing is allocated and nothing but the bags' columns is written.
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

#include "hip_pooled_kernels.h"

constexpr int POOL_COLUMN_BLOCK = 8;   // column accumulators a lane keeps in registers: 512 columns per walk of a bag

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

template <int OUT>
__device__ __forceinline__ uint2 narrowPiece(float4 v)
{
    return make_uint2(narrowPair<OUT>(v.x, v.y), narrowPair<OUT>(v.z, v.w));
}

// Seven wavefronts per SIMD, which launchPooled plans for (ONE_TILE_WAVES_PER_CU): asked of the compiler, because the
// column form's eight accumulators, live across a tile's decode, otherwise end at 72-73 vector registers -- one more than
// seven wavefronts allow for two-level tables. It fits without scratch (tests/test_pooled_narrow_isa.py).
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
        uint16_t* destination = reinterpret_cast<uint16_t*>(p.out) + bag * p.ld + p.colOff;
        if (end <= begin) {
            if (VEC4) {
                for (uint32_t c = lane; c < pieces; c += WAVE) {
                    *reinterpret_cast<uint2*>(destination + 4 * c) = make_uint2(0u, 0u);
                }
            } else {
                for (uint32_t c = lane; c < p.dim; c += WAVE) {
                    destination[c] = 0;
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
                *reinterpret_cast<uint2*>(destination + 4 * lane) = narrowPiece<OUT>(acc0);
            }
            if (lane + WAVE < pieces) {
                *reinterpret_cast<uint2*>(destination + 4 * (lane + WAVE)) = narrowPiece<OUT>(acc1);
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
                        destination[c] = static_cast<uint16_t>(narrowBits<OUT>(pool.mean ? __fdiv_rn(acc[j], count) : acc[j]));
                    }
                }
            }
        }
    }
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

// Every instance, indexed [HAS_SUB][FAST][VEC4][out type - 1] (trained) and [out type - 1].
struct NarrowPoolTable {
    const void* trained[2][2][2][2] = {};
    const void* uniform[2] = {};
    const void* full[2] = {};

    NarrowPoolTable()
    {
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
        uniform[OUT - 1] = reinterpret_cast<const void*>(&pool_uniform_narrow<OUT>);
        full[OUT - 1] = reinterpret_cast<const void*>(&pool_full_narrow<OUT>);
    }

    template <bool HAS_SUB, bool FAST, int OUT>
    void addKeyForm()
    {
        trained[HAS_SUB][FAST][0][OUT - 1] = reinterpret_cast<const void*>(&pool_trained_narrow<HAS_SUB, FAST, false, OUT>);
        trained[HAS_SUB][FAST][1][OUT - 1] = reinterpret_cast<const void*>(&pool_trained_narrow<HAS_SUB, FAST, true, OUT>);
    }
};

const NarrowPoolTable& narrowPoolTable()
{
    static const NarrowPoolTable table;
    return table;
}

bool knownType(int outType)
{
    return outType == MEMB_HIP_OUT_BF16 || outType == MEMB_HIP_OUT_F16;
}

}  // namespace

namespace memb_pooled {

const void* trainedKernelNarrow(bool hasSub, bool fast, bool vec4, int outType)
{
    return knownType(outType) ? narrowPoolTable().trained[hasSub][fast][vec4][outType - 1] : nullptr;
}

const void* uniformKernelNarrow(int outType)
{
    return knownType(outType) ? narrowPoolTable().uniform[outType - 1] : nullptr;
}

const void* fullKernelNarrow(int outType)
{
    return knownType(outType) ? narrowPoolTable().full[outType - 1] : nullptr;
}

}  // namespace memb_pooled
