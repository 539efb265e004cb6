// Helpers shared by all kernels: magic division, wave-level LDS fence, single-lane-op IEEE arithmetic, the accumulate / divide epilogue.
//
// Device code of libmemb_hip.so (gfx950 / CDNA4). Included by memb_hip.hip and memb_hip_narrow.hip,
// inside their anonymous namespaces; see memb_hip.hip for the overview.
#pragma once

// q / d with a host-computed magic = ceil(2^32 / d) (exact while q * d < 2^32);
// magic == 0 means "no magic" (d == 1, or the range is too large): plain division.
__device__ __forceinline__ uint32_t fastDivide(uint32_t q, uint32_t magic, uint32_t d)
{
    return magic ? __umulhi(q, magic) : q / d;
}

// Orders this wave's LDS writes before its later LDS reads (and vice versa).
// LDS operations of one wave execute in order; the fence makes the compiler
// wait for them and keeps it from moving accesses across.
__device__ __forceinline__ void waveLdsFence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Single-lane-op IEEE fp32 add / sub / mul. Written as instructions because the
// optimiser otherwise pairs neighbouring operations into v_pk_add_f32 /
// v_pk_mul_f32, and the packed forms flush subnormal values on gfx950 (measured:
// min = 1e-40 came back as 0), which would break bit parity with the CPU.
__device__ __forceinline__ float addRn(float a, float b)
{
    float r;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ float subRn(float a, float b)
{
    float r;
    asm("v_sub_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ float mulRn(float a, float b)
{
    float r;
    asm("v_mul_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Epilogue of ReadersUnion 'average' (reference python/memb/readers_union.py:18:
// numpy.mean over the readers = fp32 sums in reader order, then one division
// by the reader count): later readers add to what earlier ones stored, the last
// one divides. Same operations and order as numpy, so the result is bit-identical.
__device__ __forceinline__ float epilogue(float value, const float* destination, uint32_t accumulate, float divisor)
{
    if (accumulate) {
        value = addRn(*destination, value);
    }
    if (divisor != 0.f) {
        value = __fdiv_rn(value, divisor);
    }
    return value;
}

__device__ __forceinline__ float4 epilogue4(float4 value, const float* destination, uint32_t accumulate, float divisor)
{
    if (accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(destination);
        value.x = addRn(old.x, value.x);
        value.y = addRn(old.y, value.y);
        value.z = addRn(old.z, value.z);
        value.w = addRn(old.w, value.w);
    }
    if (divisor != 0.f) {
        value.x = __fdiv_rn(value.x, divisor);
        value.y = __fdiv_rn(value.y, divisor);
        value.z = __fdiv_rn(value.z, divisor);
        value.w = __fdiv_rn(value.w, divisor);
    }
    return value;
}

// Narrow output elements (memb_hip_narrow.hip; OUT = MEMB_HIP_OUT_BF16 or MEMB_HIP_OUT_F16 of include/memb_hip_narrow.h): an
// fp32 value rounded once to the nearest even value by a plain cast -- v_cvt_pk_bf16_f32 / v_cvt_f16_f32 on gfx950, which
// under the library's float mode (subnormals kept) give torch's bits for subnormals, infinities and signed zeros and keep
// a NaN a NaN. (The integer form (u + 0x7FFF + ((u >> 16) & 1)) >> 16 turns some NaNs into zeros or infinities.)
template <int OUT>
__device__ __forceinline__ uint32_t narrowBits(float value)
{
    if constexpr (OUT == 1) {   // MEMB_HIP_OUT_BF16
        return __builtin_bit_cast(uint16_t, static_cast<__bf16>(value));
    } else {                    // MEMB_HIP_OUT_F16
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(value));
    }
}

// two values, `low` in the lower half: the dword at the lower address of a little-endian pair
template <int OUT>
__device__ __forceinline__ uint32_t narrowPair(float low, float high)
{
    return narrowBits<OUT>(low) | (narrowBits<OUT>(high) << 16);
}
