// The kernel of memb_hip_query_matrix.hip (include/memb_hip_query_matrix.h: the cosine and the dot product of every one of
// n_queries fp32 query vectors against every one of n candidate rows of ONE shared list, and the candidates' norms, from the
// compressed rows of a trained model) as memb_hip.hip launches it (hip_query_matrix_launch.h): host addresses for
// hipLaunchKernel, as memb::KernelHandle. The first parameter of the kernel is the TrainedParams of
// hip_trained_kernels.h -- rows[0 .. n) are the candidates; out / ld / colOff are not used --, its second the
// QueryMatrixParams below.
#pragma once

#include <cstdint>

#include "hip_queries.h"   // (the unit builds on query_trained's device code; the grid starts from planQueryGrid's)

namespace memb_query_matrix {

struct QueryMatrixParams {
    const float* queries;          // query q: queries[q * ldQueries .. + dim)
    float* cosines;                // [nQueries rows, ldOut floats apart] or null: cosines[q * ldOut + i]
    float* dots;                   // likewise, or null
    float* norms;                  // [n] or null: the candidate row's norm, once
    unsigned long long ldQueries;  // in floats
    unsigned long long ldOut;      // in floats, >= n
    uint32_t nQueries;             // 1 .. 2^16
    uint32_t entriesPerWave;       // consecutive candidates a wavefront owns (launch geometry, never the result)
};

// Queries a wavefront holds in registers at once (eight registers each) while a tile's words go by: B of DESIGN.md
// section 5.11 and of tests/test_gpu_query_matrix.py. Launch geometry in the wide sense: never the result.
constexpr uint32_t QUERY_BLOCK = 2;
constexpr uint32_t MAX_QUERIES = 1u << 16;
// Wavefronts per SIMD the kernel's registers allow (tests/test_query_matrix_isa.py): what the
// launch plans its grid for.
constexpr uint32_t TRAINED_WAVES_PER_SIMD = 7;

// query_matrix_trained<HAS_SUB, FAST>: dim a multiple of 4 and at most memb_pooled::TRAINED_VEC4_MAX_DIM, any words per
// wavefront. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast);

}  // namespace memb_query_matrix
