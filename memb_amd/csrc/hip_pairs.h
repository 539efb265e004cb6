// The kernels of memb_hip_pairs.hip (include/memb_hip_pairs.h: the cosine, the dot product and the two norms of pairs of
// rows, from the compressed rows of a trained model or from a dense fp32 matrix) as memb_hip.hip launches them
// (hip_pairs_launch.h): host addresses for hipLaunchKernel, as memb::KernelHandle. The first parameter of the
// trained kernel is the TrainedParams of hip_trained_kernels.h -- rows[0 .. n) are the 2 * pairs entries, a pair the
// entries 2i and 2i + 1; out / ld / colOff are not used --, its second the PairParams below; the dense kernel takes the
// DensePairParams.
#pragma once

#include <cstdint>

#include "hip_norms.h"   // (the unit builds on norms_trained's device code, which takes the NormParams)

namespace memb_pairs {

struct PairParams {
    float* cosines;            // [pairs] or null
    float* dots;               // [pairs] or null
    float* norms;              // [2 * pairs] or null: entry e's norm at norms[e]
    uint32_t entriesPerWave;   // consecutive entries a wavefront owns, an even number (launch geometry, never the result)
};

struct DensePairParams {
    const float* values;          // row r: values[r * ldValues .. + dim); pair i: the rows 2i and 2i + 1
    float* cosines;               // as in PairParams
    float* dots;
    float* norms;
    unsigned long long pairs;
    unsigned long long ldValues;  // in floats
    uint32_t dim;
};

constexpr uint32_t DENSE_WAVES = memb_norms::DENSE_WAVES;   // one pair per wavefront

// pairs_trained<HAS_SUB, FAST>: dim a multiple of 4 and at most memb_pooled::TRAINED_VEC4_MAX_DIM, at least two words per
// wavefront. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast);

// pairs_dense: one wavefront per pair, blocks of DENSE_WAVES wavefronts, any dim and alignment.
memb::KernelHandle denseKernel();

}  // namespace memb_pairs
