// The kernels of memb_hip_pooled.hip and memb_hip_pooled_narrow.hip (sum / mean of each bag of rows, as fp32 and as bf16 /
// fp16 elements) as memb_hip.hip launches them (launchPooled):
// host addresses for hipLaunchKernel / hipFuncGetAttributes. Their first parameter is the TrainedParams / UniformParams /
// FullParams of the device headers, which both translation units include -- rows[0 .. n) are the ENTRIES, out / ld /
// colOff describe the bags' rows -- their second the PoolParams below.
#pragma once

#include <cstdint>

namespace memb_pooled {

struct PoolParams {
    const uint32_t* offsets;     // [bags + 1]: bag b owns the entries [min(offsets[b], n), min(offsets[b + 1], n))
    unsigned long long bags;
    uint32_t bagsPerWave;        // pool_trained: consecutive bags a wavefront owns (launch geometry, never the result)
    uint32_t mean;               // MEMB_HIP_POOL_MEAN: divide each sum by its bag's entry count
};

// pool_trained<HAS_SUB, FAST, VEC4>; null where no instance exists (HAS_SUB with FAST). VEC4: register accumulators of
// 16-byte pieces (dim a multiple of 4 and at most TRAINED_VEC4_MAX_DIM, out / ld / colOff aligned to a piece), else the
// column form for any dim
constexpr uint32_t TRAINED_VEC4_MAX_DIM = 512;   // two pieces per lane
const void* trainedKernel(bool hasSub, bool fast, bool vec4);
// pool_uniform / pool_full: one wavefront per bag, blocks of ROWWISE_WAVES wavefronts
constexpr uint32_t ROWWISE_WAVES = 4;
const void* uniformKernel();
const void* fullKernel();

// memb_hip_pooled_narrow.hip: the same kernels with bags' rows of outType MEMB_HIP_OUT_BF16 / MEMB_HIP_OUT_F16 (null for
// another type). pool_trained_narrow<HAS_SUB, FAST, VEC4, OUT> -- VEC4: 8-byte pieces of four elements (dim a multiple of
// 4, out / ld / colOff aligned to a piece), else register blocks of columns for any dim, one walk of the bag per 512
// columns -- takes pool_trained's LDS (an fp32 codebook); pool_uniform_narrow<OUT> / pool_full_narrow<OUT>
const void* trainedKernelNarrow(bool hasSub, bool fast, bool vec4, int outType);
const void* uniformKernelNarrow(int outType);
const void* fullKernelNarrow(int outType);

}  // namespace memb_pooled
