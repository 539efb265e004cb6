// The kernels of memb_hip_bag_pairs.hip (include/memb_hip_bag_pairs.h: the cosine, the dot product and the two norms of
// pairs of summed or averaged bags of rows, from the compressed rows of a trained model) as memb_hip.hip launches them
// (hip_bag_pairs_launch.h): host addresses for hipLaunchKernel, as memb::KernelHandle. The first parameter of the
// kernel is the TrainedParams of hip_trained_kernels.h -- rows[0 .. n) are the ENTRIES; out / ld / colOff are not used --,
// its second the PoolParams of hip_pooled.h -- 2 * pairs bags, bagsPerWave an EVEN number --, its third the BagPairParams
// below.
#pragma once

#include <cstdint>

#include "hip_pairs.h"   // (the unit builds on pairs_trained's device code, which takes the PairParams)
#include "hip_pooled.h"

namespace memb_bag_pairs {

struct BagPairParams {
    float* cosines;   // [pairs] or null
    float* dots;      // [pairs] or null
    float* norms;     // [2 * pairs] or null: bag b's norm at norms[b]
};

// Wavefronts per SIMD the kernel's registers allow (tests/test_bag_pairs_isa.py): what the launch
// plans its grid for.
constexpr uint32_t TRAINED_WAVES_PER_SIMD = 7;

// bag_pairs_trained<HAS_SUB, FAST>: dim a multiple of 4 and at most memb_pooled::TRAINED_VEC4_MAX_DIM, any words per
// wavefront. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast);

}  // namespace memb_bag_pairs
