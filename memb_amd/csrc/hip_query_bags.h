// The kernel of memb_hip_query_bags.hip (include/memb_hip_query_bags.h: the cosine and the dot product of every one of
// n_queries fp32 query vectors against every one of `bags` summed or averaged bags of rows, and the pooled rows' norms,
// from the compressed rows of a trained model) as memb_hip.hip launches it (hip_query_bags_launch.h): host addresses for
// hipLaunchKernel, as memb::KernelHandle. The first parameter of the kernel is the
// TrainedParams of hip_trained_kernels.h -- rows[0 .. n) are the ENTRIES; out / ld / colOff are not used --, its second
// the PoolParams of hip_pooled.h, its third the QueryMatrixParams of hip_query_matrix.h, whose n is `bags`: cosines /
// dots [nQueries rows, ldOut >= bags floats apart], norms [bags]; entriesPerWave is not used (PoolParams::bagsPerWave is).
#pragma once

#include <cstdint>

#include "hip_pooled.h"
#include "hip_query_matrix.h"   // (QueryMatrixParams, QUERY_BLOCK, MAX_QUERIES; the unit builds on that unit's device code)

namespace memb_query_bags {

// Finished pooled rows a wavefront holds in registers (eight each at dim > 256) and scores together against each block of
// QUERY_BLOCK queries: G of DESIGN.md section 5.13. One store writes floor(64 / BAG_GROUP) segments of BAG_GROUP
// consecutive floats. Launch geometry in the wide sense: never the result.
constexpr uint32_t BAG_GROUP = 2;
constexpr uint32_t QUERY_BLOCK = memb_query_matrix::QUERY_BLOCK;
constexpr uint32_t MAX_QUERIES = memb_query_matrix::MAX_QUERIES;
// Wavefronts per SIMD the kernel's registers allow (tests/test_query_bags_isa.py): what the launch
// plans its grid for.
constexpr uint32_t TRAINED_WAVES_PER_SIMD = 5;

// query_bags_trained<HAS_SUB, FAST>: dim a multiple of 4 and at most memb_pooled::TRAINED_VEC4_MAX_DIM, any words per
// wavefront. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast);

}  // namespace memb_query_bags
