// bf16 / fp16 rows straight from the decoder (include/memb_hip_narrow.h): the kernels, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (launchTrained, launchUniform, launchFull) through the addresses below (hip_narrow.h). Every value is the fp32 value of the float kernels rounded
// once, to nearest even, by a plain cast (hip_device_common.h: narrowBits):
//   decode_trained_narrow<HAS_SUB, MODE, FAST, OUT>  decode_trained's body (hip_trained_kernels.h: decodeTilesOfBlock)
//                      with the codebook rounded as the block copies it into LDS (half the LDS of fp32) and the output
//                      stage outputTileNarrow; it never writes the batch-order word
//   dequant_uniform_narrow<VEC4, OUT>  the fp32 expression of dequant_uniform (four rounded operations), then the cast
//   gather_full_narrow<VEC4, OUT>      the stored fp32 value, cast
// OUT is MEMB_HIP_OUT_BF16 or MEMB_HIP_OUT_F16. No accumulate / divisor: the host refuses them for narrow outputs.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_narrow.h"
#include "codec.h"
#include "hip_narrow.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

template <bool HAS_SUB, int MODE, bool FAST, int OUT>
__global__ MEMB_SGPR_BUDGET void decode_trained_narrow(TrainedParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    decodeTilesOfBlock<HAS_SUB, MODE, FAST, false, OUT>(p, BatchList(), lds);
}

// Row-wise kernels of the uniform and full storages (the block form of dequant_uniform / gather_full): a block stages
// the row ids (and the uniform {min, max}) of its words in LDS, then every thread keeps ROWWISE_BATCH loads in flight
// before it converts and stores. VEC4: four values per thread and 8-byte store (dim, ld, col_off multiples of four,
// out 8-byte aligned), else one 2-byte store per value.
template <bool VEC4, int OUT>
__global__ void dequant_uniform_narrow(UniformParams p)
{
    __shared__ uint32_t rowLds[ROWWISE_MAX_WORDS];
    __shared__ float2 minMaxLds[ROWWISE_MAX_WORDS];
    const unsigned long long blockBase = static_cast<unsigned long long>(blockIdx.x) * p.wordsPerBlock;
    const uint32_t blockWords =
        static_cast<uint32_t>(min(static_cast<unsigned long long>(p.wordsPerBlock), p.n - blockBase));
    if (threadIdx.x < blockWords) {
        const uint32_t row = p.rows[blockBase + threadIdx.x];
        rowLds[threadIdx.x] = row;
        minMaxLds[threadIdx.x] = row < p.nRows ? *reinterpret_cast<const float2*>(uniformRegion(p, row)) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    uint16_t* out = reinterpret_cast<uint16_t*>(p.out);

    if (VEC4) {
        const uint32_t piecesPerWord = p.dim / 4;
        const uint32_t pieces = blockWords * piecesPerWord;
        for (uint32_t q0 = threadIdx.x; q0 < pieces; q0 += blockDim.x * ROWWISE_BATCH) {
            uint32_t word[ROWWISE_BATCH];
            uint32_t column[ROWWISE_BATCH];
            uint32_t packed[ROWWISE_BATCH];
#pragma unroll
            for (int u = 0; u < ROWWISE_BATCH; ++u) {
                const uint32_t q = min(q0 + u * blockDim.x, pieces - 1);
                word[u] = fastDivide(q, p.pieceMagic, piecesPerWord);
                column[u] = q - word[u] * piecesPerWord;
                const uint32_t row = rowLds[word[u]];
                packed[u] = row < p.nRows ? *reinterpret_cast<const uint32_t*>(uniformRegion(p, row) + 16 + 4 * column[u]) : 0u;
            }
#pragma unroll
            for (int u = 0; u < ROWWISE_BATCH; ++u) {
                if (q0 + u * blockDim.x < pieces) {
                    uint2 v = make_uint2(0u, 0u);
                    if (rowLds[word[u]] < p.nRows) {
                        const float2 mm = minMaxLds[word[u]];
                        const float range = subRn(mm.y, mm.x);
                        v.x = narrowPair<OUT>(dequant(mm.x, range, packed[u] & 0xff, p.levels),
                                              dequant(mm.x, range, (packed[u] >> 8) & 0xff, p.levels));
                        v.y = narrowPair<OUT>(dequant(mm.x, range, (packed[u] >> 16) & 0xff, p.levels),
                                              dequant(mm.x, range, packed[u] >> 24, p.levels));
                    }
                    *reinterpret_cast<uint2*>(out + (blockBase + word[u]) * p.ld + p.colOff + 4 * column[u]) = v;
                }
            }
        }
    } else {
        const uint32_t total = blockWords * p.dim;
        for (uint32_t q = threadIdx.x; q < total; q += blockDim.x) {
            const uint32_t w = q / p.dim;
            const uint32_t c = q - w * p.dim;
            const uint32_t row = rowLds[w];
            uint32_t value = 0;
            if (row < p.nRows) {
                const float2 mm = minMaxLds[w];
                value = narrowBits<OUT>(dequant(mm.x, subRn(mm.y, mm.x), uniformRegion(p, row)[16 + c], p.levels));
            }
            out[(blockBase + w) * p.ld + p.colOff + c] = static_cast<uint16_t>(value);
        }
    }
}

template <bool VEC4, int OUT>
__global__ void gather_full_narrow(FullParams p)
{
    __shared__ uint32_t rowLds[ROWWISE_MAX_WORDS];
    const unsigned long long blockBase = static_cast<unsigned long long>(blockIdx.x) * p.wordsPerBlock;
    const uint32_t blockWords =
        static_cast<uint32_t>(min(static_cast<unsigned long long>(p.wordsPerBlock), p.n - blockBase));
    if (threadIdx.x < blockWords) {
        rowLds[threadIdx.x] = p.rows[blockBase + threadIdx.x];
    }
    __syncthreads();
    uint16_t* out = reinterpret_cast<uint16_t*>(p.out);
    if (VEC4) {
        const uint32_t piecesPerWord = p.dim / 4;
        const uint32_t pieces = blockWords * piecesPerWord;
        for (uint32_t q0 = threadIdx.x; q0 < pieces; q0 += blockDim.x * ROWWISE_BATCH) {
            uint32_t word[ROWWISE_BATCH];
            uint32_t column[ROWWISE_BATCH];
            float4 f[ROWWISE_BATCH];
#pragma unroll
            for (int u = 0; u < ROWWISE_BATCH; ++u) {
                const uint32_t q = min(q0 + u * blockDim.x, pieces - 1);
                word[u] = fastDivide(q, p.pieceMagic, piecesPerWord);
                column[u] = q - word[u] * piecesPerWord;
                const uint32_t row = rowLds[word[u]];
                f[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < p.nRows) {
                    f[u] = *reinterpret_cast<const float4*>(p.values + static_cast<unsigned long long>(row) * p.dim + 4 * column[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < ROWWISE_BATCH; ++u) {
                if (q0 + u * blockDim.x < pieces) {
                    *reinterpret_cast<uint2*>(out + (blockBase + word[u]) * p.ld + p.colOff + 4 * column[u]) =
                        make_uint2(narrowPair<OUT>(f[u].x, f[u].y), narrowPair<OUT>(f[u].z, f[u].w));
                }
            }
        }
    } else {
        const uint32_t total = blockWords * p.dim;
        for (uint32_t q = threadIdx.x; q < total; q += blockDim.x) {
            const uint32_t w = q / p.dim;
            const uint32_t c = q - w * p.dim;
            const uint32_t row = rowLds[w];
            const float f = row < p.nRows ? p.values[static_cast<unsigned long long>(row) * p.dim + c] : 0.f;
            out[(blockBase + w) * p.ld + p.colOff + c] = static_cast<uint16_t>(narrowBits<OUT>(f));
        }
    }
}

// Every instance, indexed [HAS_SUB][MODE][FAST][out type - 1] (trained) and [VEC4][out type - 1].
struct NarrowTable {
    const void* trained[2][3][2][2] = {};
    const void* uniform[2][2] = {};
    const void* full[2][2] = {};

    NarrowTable()
    {
        addType<MEMB_HIP_OUT_BF16>();
        addType<MEMB_HIP_OUT_F16>();
    }

private:
    template <int OUT>
    void addType()
    {
        constexpr int type = OUT - 1;
        addKeyForm<false, true, OUT>();
        addKeyForm<false, false, OUT>();
        addKeyForm<true, false, OUT>();
        uniform[0][type] = reinterpret_cast<const void*>(&dequant_uniform_narrow<false, OUT>);
        uniform[1][type] = reinterpret_cast<const void*>(&dequant_uniform_narrow<true, OUT>);
        full[0][type] = reinterpret_cast<const void*>(&gather_full_narrow<false, OUT>);
        full[1][type] = reinterpret_cast<const void*>(&gather_full_narrow<true, OUT>);
    }

    template <bool HAS_SUB, bool FAST, int OUT>
    void addKeyForm()
    {
        constexpr int type = OUT - 1;
        trained[HAS_SUB][OUT_SCALAR][FAST][type] = reinterpret_cast<const void*>(&decode_trained_narrow<HAS_SUB, OUT_SCALAR, FAST, OUT>);
        trained[HAS_SUB][OUT_VEC4][FAST][type] = reinterpret_cast<const void*>(&decode_trained_narrow<HAS_SUB, OUT_VEC4, FAST, OUT>);
        trained[HAS_SUB][OUT_FLAT][FAST][type] = reinterpret_cast<const void*>(&decode_trained_narrow<HAS_SUB, OUT_FLAT, FAST, OUT>);
    }
};

const NarrowTable& narrowTable()
{
    static const NarrowTable table;
    return table;
}

bool knownType(int outType)
{
    return outType == MEMB_HIP_OUT_BF16 || outType == MEMB_HIP_OUT_F16;
}

}  // namespace

namespace memb_narrow {

const void* trainedKernel(bool hasSub, int mode, bool fast, int outType)
{
    if (!knownType(outType) || mode < OUT_SCALAR || mode > OUT_FLAT) {
        return nullptr;
    }
    return narrowTable().trained[hasSub][mode][fast][outType - 1];
}

const void* uniformKernel(bool vec4, int outType)
{
    return knownType(outType) ? narrowTable().uniform[vec4][outType - 1] : nullptr;
}

const void* fullKernel(bool vec4, int outType)
{
    return knownType(outType) ? narrowTable().full[vec4][outType - 1] : nullptr;
}

}  // namespace memb_narrow
