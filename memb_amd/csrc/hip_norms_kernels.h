// Device code of the norm kernels (memb_hip_norms.hip): a piece's sum of squares, the butterfly over the 64 lane
// partials, the walk of a wavefront over its run of rows of a trained model, and the one-row-per-wavefront loops over a
// dense matrix. Included inside the unit's anonymous namespace, behind hip_device_common.h, hip_trained_kernels.h,
// hip_rowwise_kernels.h and hip_pooled_kernels.h (decodePoolTile, gatherPiece, divide4, storePiece).
#pragma once

using memb_norms::DenseNormParams;
using memb_norms::NormParams;

constexpr float UNIT_EPS = 1e-12f;   // torch.nn.functional.normalize's eps

// q = ((v0 v0 + v1 v1) + v2 v2) + v3 v3: seven single-lane operations, nothing fused (the packed forms flush subnormals).
__device__ __forceinline__ float pieceSquares(float4 v)
{
    return addRn(addRn(addRn(mulRn(v.x, v.x), mulRn(v.y, v.y)), mulRn(v.z, v.z)), mulRn(v.w, v.w));
}

// p_(l xor S) for S = 1 .. 16: ds_swizzle_b32 in its bit-mask mode (and 0x1f, or 0, xor S) exchanges within 32 lanes
// without touching LDS memory. (Not DPP: its operand here is the result of an inline-assembly add, whose two wait states
// in front of a DPP read the compiler does not count.)
template <int S>
__device__ __forceinline__ float laneXor(float p)
{
    static_assert(S >= 1 && S <= 16, "within a half of the wavefront");
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(p), 0x1f | (S << 10)));
}

// The contract's butterfly: strides 1, 2, 4, 8, 16, 32 in that order, every lane ends with the same bits.
__device__ __forceinline__ float butterfly(float p, uint32_t lane)
{
    p = addRn(p, laneXor<1>(p));
    p = addRn(p, laneXor<2>(p));
    p = addRn(p, laneXor<4>(p));
    p = addRn(p, laneXor<8>(p));
    p = addRn(p, laneXor<16>(p));
    const float other = __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>((lane ^ 32u) * 4u), __float_as_int(p)));
    return addRn(p, other);
}

// sqrt(t), correctly rounded, a subnormal t included: __builtin_sqrtf under -fhip-fp32-correctly-rounded-divide-sqrt --
// v_sqrt_f32 (one ulp) on the scaled argument and the fused multiply-add fix-up behind it (tests/test_norms_isa.py looks
// for that sequence). HIP's __fsqrt_rn is NOT this: without OCML's rounded operations it is the native root alone.
__device__ __forceinline__ float correctSqrt(float t)
{
    return __builtin_sqrtf(t);
}

// What a unit row is divided by.
__device__ __forceinline__ float unitDivisor(float norm)
{
    return norm < UNIT_EPS ? UNIT_EPS : norm;
}

// pool_trained's walk with bags of one entry: a wavefront owns the rows [first, last) of the batch, decodes them tile by
// tile up to the symbol tile (decodePoolTile) and, word by word, gathers its two pieces -- lane l holds the pieces l and
// l + 64: the contract's layout --, squares, reduces and takes the root. The norms of a tile leave as one store, lane w
// word w's. UNIT: the pieces in registers are divided and stored, 16 bytes each.
template <bool HAS_SUB, bool FAST, bool UNIT>
__device__ __forceinline__ void normsOfWave(const TrainedParams& p, const NormParams& np, uint32_t* lds)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long first = (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * np.rowsPerWave;
    if (first >= p.n) {
        return;
    }
    const unsigned long long last = min(first + np.rowsPerWave, p.n);
    const uint32_t pieces = p.dim / 4;   // 1 .. 128
    PoolTile tile;

#pragma nounroll
    for (unsigned long long start = first; start < last; start += p.wordsPerWave) {
        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, start, last, tile);
        const uint32_t words = static_cast<uint32_t>(tile.end - tile.start);
        float mine = 0.f;
#pragma nounroll
        for (uint32_t w = 0; w < words; ++w) {
            const float4 v0 = gatherPiece<FAST>(p, mem, tile, w, min(lane, pieces - 1));
            float partial = lane < pieces ? pieceSquares(v0) : 0.f;
            float4 v1 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pieces > WAVE) {   // wave-uniform
                v1 = gatherPiece<FAST>(p, mem, tile, w, min(lane + WAVE, pieces - 1));
                // (a lane without a second piece adds +0.0 to a sum of squares, which is never -0.0: the same bits)
                partial = addRn(partial, lane + WAVE < pieces ? pieceSquares(v1) : 0.f);
            }
            const float norm = correctSqrt(butterfly(partial, lane));
            if (UNIT) {
                float* destination = p.out + (tile.start + w) * p.ld + p.colOff;
                const float divisor = unitDivisor(norm);
                if (lane < pieces) {
                    storePiece<MEMB_HIP_OUT_F32>(destination, lane, divide4(v0, divisor));
                }
                if (lane + WAVE < pieces) {
                    storePiece<MEMB_HIP_OUT_F32>(destination, lane + WAVE, divide4(v1, divisor));
                }
            }
            mine = lane == w ? norm : mine;
        }
        if (np.norms && lane < words) {
            np.norms[tile.start + lane] = mine;
        }
    }
}

// Piece k of a dense row of dim columns: a column >= dim is +0.0. aligned (wave-uniform): the row starts on 16 bytes and
// dim is a multiple of 4.
__device__ __forceinline__ float4 densePiece(const float* row, uint32_t dim, uint32_t k, bool aligned)
{
    if (aligned) {
        return reinterpret_cast<const float4*>(row)[k];
    }
    const uint32_t c = 4 * k;
    return make_float4(row[c], c + 1 < dim ? row[c + 1] : 0.f, c + 2 < dim ? row[c + 2] : 0.f, c + 3 < dim ? row[c + 3] : 0.f);
}

// One wavefront per row of a dense matrix: lane l adds the squares of the pieces l, l + 64, .. in that order, the
// butterfly and the root follow. UNIT: the row is then read again, column by column, divided and stored -- in place where
// out's columns are the values': every load of the first pass has returned before the butterfly ends, and in the second
// a lane reads what it alone overwrites.
template <bool UNIT>
__device__ __forceinline__ void denseRowOfWave(const DenseNormParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long i =
        static_cast<unsigned long long>(blockIdx.x) * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    if (i >= p.n) {
        return;
    }
    const float* row = p.values + i * p.ldValues;
    const bool aligned = p.dim % 4 == 0 && p.ldValues % 4 == 0 && reinterpret_cast<uintptr_t>(p.values) % 16 == 0;
    const uint32_t pieces = p.dim / 4 + (p.dim % 4 != 0);
    float partial = 0.f;
    if (lane < pieces) {
        partial = pieceSquares(densePiece(row, p.dim, lane, aligned));
        for (uint32_t k = lane + WAVE; k < pieces; k += WAVE) {
            partial = addRn(partial, pieceSquares(densePiece(row, p.dim, k, aligned)));
        }
    }
    const float norm = correctSqrt(butterfly(partial, lane));
    if (UNIT) {
        float* destination = p.out + i * p.ld + p.colOff;
        const float divisor = unitDivisor(norm);
        for (uint32_t c = lane; c < p.dim; c += WAVE) {
            destination[c] = __fdiv_rn(row[c], divisor);
        }
    }
    if (p.norms && lane == 0) {
        p.norms[i] = norm;
    }
}
