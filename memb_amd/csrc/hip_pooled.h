// The kernels of memb_hip_pooled.hip (sum / mean of each bag of rows) as memb_hip.hip launches them (launchPooled):
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

}  // namespace memb_pooled
