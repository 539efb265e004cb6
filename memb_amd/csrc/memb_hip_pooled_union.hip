// Pooled lookups of a ReadersUnion (include/memb_hip_pooled_union.h): the sum or mean of each bag of the union's AVERAGED
// rows, decoded, merged and reduced in one kernel, and the same reduction over a dense fp32 matrix, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (launchPooledUnion, launchPooledDense) through the selectors below (hip_pooled_union.h).
//   pool_trained_union<HAS_SUB, FAST, COUNT, OUT>   COUNT trained models of one dim and lane geometry. pool_trained's walk:
//                      a wavefront owns a run of whole consecutive bags and decodes full tiles of entries across bag
//                      boundaries -- here every model's words of the tile, each into that model's own symbol tile
//                      (decodePoolTile per model; tables, codebooks and the per-wavefront areas laid out as for
//                      decode_trained_union). For its 16-byte piece a lane gathers each model's four values (gatherPiece),
//                      merges them as decode_trained_union's AVERAGE does -- add4 in model order, one divide4 by COUNT --
//                      and adds the merged piece to the bag's accumulator. Neither the rows nor the merged rows reach memory.
//   pool_dense<OUT>    poolBagOfWave over the rows of an fp32 matrix: one wavefront per bag, lanes own columns
// OUT is a MEMB_HIP_OUT_*. The contract is memb_hip_pooled.h's ORDER over the merged rows u_i = (((v1_i + v2_i) + ..) / COUNT:
// acc = u_begin, then acc = acc + u_i one entry after the other, each add one v_add_f32 (addRn: the packed forms flush
// subnormals on this part), one correctly rounded division for the mean, a bf16 / fp16 element rounded ONCE as it is stored.
// A lane owns its columns for the whole bag: no value crosses lanes, nothing depends on launch geometry, no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "../../include/memb_hip_pooled_union.h"
#include "codec.h"
#include "hip_pooled_union.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

#include "hip_pooled_kernels.h"

using memb_pooled::DenseParams;

constexpr int UNION_GATHER_BATCH = 2;   // entries whose merged pieces a lane works out before it adds them one after the
                                        // other: COUNT gathers each (POOL_GATHER_BATCH of a single model's is four)

// One wavefront's view of every model: table and codebook in the block's shared image, slots and symbol tile in the
// wavefront's own area. Named members and compile-time selection, as AbsentMasks: arrays of these went to scratch memory.
template <int COUNT>
struct UnionLds {
    WaveLds m0, m1, m2, m3;
    PoolTile t0, t1, t2, t3;

    template <int M>
    __device__ __forceinline__ WaveLds& mem()
    {
        if constexpr (M == 0) return m0;
        else if constexpr (M == 1) return m1;
        else if constexpr (M == 2) return m2;
        else return m3;
    }

    template <int M>
    __device__ __forceinline__ PoolTile& tile()
    {
        if constexpr (M == 0) return t0;
        else if constexpr (M == 1) return t1;
        else if constexpr (M == 2) return t2;
        else return t3;
    }
};

template <int COUNT, int M = 0>
__device__ __forceinline__ void setUpWave(const UnionParams& u, uint32_t* lds, uint32_t* area, UnionLds<COUNT>& w)
{
    if constexpr (M < COUNT) {
        WaveLds& mem = w.template mem<M>();
        mem.table = reinterpret_cast<const TableEntry*>(lds + u.tableOffsetDwords[M]);
        mem.codebook = lds + u.codebookOffsetDwords + M * 512;
        mem.slots = area + u.slotOffsetDwords[M];
        mem.keyTile = area + u.keyTileOffsetDwords[M];
        setUpWave<COUNT, M + 1>(u, lds, area, w);
    }
}

// Every model's words of the tile that starts at entry `start` (decodePoolTile's limit), one model after the other.
template <bool HAS_SUB, bool FAST, int COUNT, int M = 0>
__device__ __forceinline__ void decodeUnionTile(
    const UnionParams& u, UnionLds<COUNT>& w, uint32_t lane, unsigned long long start, unsigned long long limit)
{
    if constexpr (M < COUNT) {
        decodePoolTile<HAS_SUB, FAST>(u.model[M], w.template mem<M>(), lane, start, limit, w.template tile<M>());
        decodeUnionTile<HAS_SUB, FAST, COUNT, M + 1>(u, w, lane, start, limit);
    }
}

// The sum of the models' pieces c of word `word` in model order: piece M added to `sum`, which holds models 0 .. M - 1.
template <bool FAST, int COUNT, int M>
__device__ __forceinline__ float4 addModels(const UnionParams& u, UnionLds<COUNT>& w, uint32_t word, uint32_t c, float4 sum)
{
    if constexpr (M < COUNT) {
        const float4 next = gatherPiece<FAST>(u.model[M], w.template mem<M>(), w.template tile<M>(), word, c);
        return addModels<FAST, COUNT, M + 1>(u, w, word, c, add4(sum, next));
    } else {
        return sum;
    }
}

// a / COUNT, correctly rounded. The compiler turns a division by the constant 2 or 4 into a multiplication by 0.5 or 0.25
// -- the same correctly rounded quotient, a power of two being exact -- and pairs two of them into v_pk_mul_f32, which
// flushes subnormals on this part: that multiplication is written here as the single-lane instruction. Three models
// divide (__fdiv_rn).
template <int COUNT>
__device__ __forceinline__ float4 divideByModels(float4 a)
{
    if constexpr (COUNT == 2 || COUNT == 4) {
        constexpr float reciprocal = 1.0f / COUNT;
        return make_float4(mulRn(a.x, reciprocal), mulRn(a.y, reciprocal), mulRn(a.z, reciprocal), mulRn(a.w, reciprocal));
    } else {
        return divide4(a, static_cast<float>(COUNT));
    }
}

// Piece c of the merged row of word `word` of the tile: (((v1 + v2) + ..) / COUNT, a missing row +0.0 (outputUnionTile's
// AVERAGE arithmetic).
template <bool FAST, int COUNT>
__device__ __forceinline__ float4 mergedPiece(const UnionParams& u, UnionLds<COUNT>& w, uint32_t word, uint32_t c)
{
    const float4 first = gatherPiece<FAST>(u.model[0], w.m0, w.t0, word, c);
    return divideByModels<COUNT>(addModels<FAST, COUNT, 1>(u, w, word, c, first));
}

// accumulatePiece over merged pieces: acc (+)= words [w0, w1) of the tile, in that order, for the lane's piece c.
template <bool FAST, int COUNT>
__device__ __forceinline__ void accumulateMergedPiece(
    const UnionParams& u, UnionLds<COUNT>& w, uint32_t w0, uint32_t w1, uint32_t c, bool started, float4& acc)
{
    if (!started) {
        acc = mergedPiece<FAST, COUNT>(u, w, w0, c);
        ++w0;
    }
    for (uint32_t word = w0; word < w1; word += UNION_GATHER_BATCH) {
        float4 v[UNION_GATHER_BATCH];
#pragma unroll
        for (int b = 0; b < UNION_GATHER_BATCH; ++b) {
            v[b] = mergedPiece<FAST, COUNT>(u, w, min(word + b, w1 - 1), c);
        }
#pragma unroll
        for (int b = 0; b < UNION_GATHER_BATCH; ++b) {
            if (word + b < w1) {   // wave-uniform
                acc = add4(acc, v[b]);
            }
        }
    }
}

// pool_trained's VEC4 form over COUNT models: lane l owns the 16-byte pieces l and l + 64 of a bag's row in registers.
template <bool HAS_SUB, bool FAST, int COUNT, int OUT>
__global__ void pool_trained_union(UnionParams u, PoolParams pool)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const TrainedParams& p = u.model[0];   // (n, dim, out, ld, colOff: the same in every model)
    setUpUnionLds<COUNT>(u, lds);
    UnionLds<COUNT> w;
    setUpWave<COUNT>(u, lds, lds + u.sharedDwords + wave * u.perWaveDwords, w);
    const unsigned long long firstBag =
        (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pool.bagsPerWave;
    if (firstBag >= pool.bags) {
        return;
    }
    const unsigned long long lastBag = min(firstBag + pool.bagsPerWave, pool.bags);
    // where this wavefront's entries end while the offsets ascend: tiles are not decoded past it
    const unsigned long long runEnd = min(static_cast<unsigned long long>(pool.offsets[lastBag]), p.n);
    const uint32_t pieces = p.dim / 4;

#pragma nounroll
    for (unsigned long long bag = firstBag; bag < lastBag; ++bag) {
        unsigned long long begin, end;
        bagRange(pool, bag, p.n, &begin, &end);
        float* destination = bagDestination<OUT>(p, bag);
        if (end <= begin) {
            for (uint32_t c = lane; c < pieces; c += WAVE) {
                storePiece<OUT>(destination, c, make_float4(0.f, 0.f, 0.f, 0.f));
            }
            continue;
        }
        const float count = static_cast<float>(static_cast<uint32_t>(end - begin));
        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
        bool started = false;
#pragma nounroll
        for (unsigned long long i = begin; i < end;) {
            if (i < w.t0.start || i >= w.t0.end) {
                decodeUnionTile<HAS_SUB, FAST, COUNT>(u, w, lane, i, max(runEnd, end));
            }
            const unsigned long long upTo = min(end, w.t0.end);
            const uint32_t w0 = static_cast<uint32_t>(i - w.t0.start);
            const uint32_t w1 = static_cast<uint32_t>(upTo - w.t0.start);
            accumulateMergedPiece<FAST, COUNT>(u, w, w0, w1, min(lane, pieces - 1), started, acc0);
            if (pieces > WAVE) {
                accumulateMergedPiece<FAST, COUNT>(u, w, w0, w1, min(lane + WAVE, pieces - 1), started, acc1);
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
    }
}

// A dense fp32 matrix: entry i is row i of `values`.
template <int OUT>
__global__ void pool_dense(DenseParams p, PoolParams pool)
{
    poolBagOfWave<OUT>(p, pool, [&p](unsigned long long entry, uint32_t c) -> float { return p.values[entry * p.ldValues + c]; });
}

constexpr int OUT_TYPES = 3;
static_assert(MEMB_HIP_OUT_F32 == 0 && MEMB_HIP_OUT_BF16 == 1 && MEMB_HIP_OUT_F16 == 2, "the tables are indexed by out type");

struct Instance {
    const void* address = nullptr;
    std::string name;
};

// Every instance, indexed [HAS_SUB][FAST][COUNT][out type] and [out type]. Key forms <HAS_SUB, FAST>: <false, true> nibble
// keys in every model, <false, false> and <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct UnionPoolTable {
    Instance trained[2][2][UNION_MAX_MODELS + 1][OUT_TYPES];
    Instance dense[OUT_TYPES];

    UnionPoolTable()
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
        char text[32];
        std::snprintf(text, sizeof(text), "pool_dense<%d>", OUT);
        dense[OUT] = {reinterpret_cast<const void*>(&pool_dense<OUT>), text};
    }

    template <bool HAS_SUB, bool FAST, int OUT>
    void addKeyForm()
    {
        addCount<HAS_SUB, FAST, 2, OUT>();
        addCount<HAS_SUB, FAST, 3, OUT>();
        addCount<HAS_SUB, FAST, 4, OUT>();
    }

    template <bool HAS_SUB, bool FAST, int COUNT, int OUT>
    void addCount()
    {
        char text[64];
        std::snprintf(text, sizeof(text), "pool_trained_union<%s, %s, %d, %d>", HAS_SUB ? "true" : "false", FAST ? "true" : "false", COUNT, OUT);
        trained[HAS_SUB][FAST][COUNT][OUT] = {reinterpret_cast<const void*>(&pool_trained_union<HAS_SUB, FAST, COUNT, OUT>), text};
    }
};

const UnionPoolTable& unionPoolTable()
{
    static const UnionPoolTable table;
    return table;
}

}  // namespace

namespace memb_pooled {

memb::KernelHandle pooledUnionKernel(bool hasSub, bool fast, int count, int outType)
{
    if (count < 2 || count > UNION_MAX_MODELS || outType < 0 || outType >= OUT_TYPES) {
        return memb::KernelHandle{nullptr, "pool_trained_union"};
    }
    const Instance& instance = unionPoolTable().trained[hasSub][fast][count][outType];
    return memb::KernelHandle{instance.address, instance.address ? instance.name.c_str() : "pool_trained_union"};
}

memb::KernelHandle pooledDenseKernel(int outType)
{
    if (outType < 0 || outType >= OUT_TYPES) {
        return memb::KernelHandle{nullptr, "pool_dense"};
    }
    const Instance& instance = unionPoolTable().dense[outType];
    return memb::KernelHandle{instance.address, instance.name.c_str()};
}

}  // namespace memb_pooled
