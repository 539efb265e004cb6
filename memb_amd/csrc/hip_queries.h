// The kernel of memb_hip_queries.hip (include/memb_hip_queries.h: the cosine, the dot product and the row norm of every
// candidate row of a group against that group's fp32 query vector, from the compressed rows of a trained model) as
// memb_hip.hip launches it (hip_queries_launch.h): host addresses for hipLaunchKernel, as memb::KernelHandle. The
// first parameter of the kernel is the TrainedParams of hip_trained_kernels.h -- rows[0 .. n) are the ENTRIES, the
// candidates of every group one after the other; out / ld / colOff are not used --, its second the QueryParams below.
#pragma once

#include <cstdint>

#include "hip_pairs.h"    // (the unit builds on pairs_trained's device code, which takes the PairParams)
#include "hip_pooled.h"   // (pooledBagsPerWave: the run a wavefront owns, hip_queries_launch.h)

namespace memb_queries {

struct QueryParams {
    const float* queries;          // query g: queries[g * ldQueries .. + dim)
    const uint32_t* offsets;       // [groups + 1]: group g owns the entries [min(offsets[g], n), min(offsets[g + 1], n))
    float* cosines;                // [n] or null, indexed by entry
    float* dots;                   // [n] or null
    float* norms;                  // [n] or null: the candidate row's norm
    unsigned long long ldQueries;  // in floats
    uint32_t groups;               // 1 .. 2^32 - 2
    uint32_t entriesPerWave;       // consecutive entries a wavefront owns (launch geometry, never the result)
};

// Wavefronts per SIMD the kernel's registers allow (tests/test_queries_isa.py): what the launch
// plans its grid for.
constexpr uint32_t TRAINED_WAVES_PER_SIMD = 7;

// query_trained<HAS_SUB, FAST>: dim a multiple of 4 and at most memb_pooled::TRAINED_VEC4_MAX_DIM, any words per
// wavefront. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast);

}  // namespace memb_queries
