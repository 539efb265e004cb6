// Pooled lookups (include/memb_hip_pooled.h): the sum or mean of each bag of rows, decoded and reduced in one kernel,
// gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (launchPooled) through the addresses below (hip_pooled.h). A bag's rows never reach memory: per entry a kernel reads
// the row id and the row's compressed bytes, per bag it writes dim floats. The device code up to the stores is shared with
// the bf16 / fp16 kernels of memb_hip_pooled_narrow.hip (hip_pooled_kernels.h).
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

// Uniform and full storage: one wavefront per bag (hip_pooled_kernels.h: poolBagOfWave).
__global__ void pool_uniform(UniformParams p, PoolParams pool)
{
    poolBagOfWave<MEMB_HIP_OUT_F32>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return uniformValue(p, row, c); });
}

__global__ void pool_full(FullParams p, PoolParams pool)
{
    poolBagOfWave<MEMB_HIP_OUT_F32>(p, pool, [&p](uint32_t row, uint32_t c) -> float { return fullValue(p, row, c); });
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
