// The kernels of memb_hip_pooled_known.hip (sum / mean of the KNOWN rows of each bag: include/memb_hip_pooled_known.h) as
// memb_hip.hip launches them (launchPooled): host addresses for hipLaunchKernel. Their first two parameters are those of
// the pooled kernels (hip_pooled.h), their third the KnownParams below.
#pragma once

#include <cstdint>

#include "hip_pooled.h"

namespace memb_pooled {

struct KnownParams {
    uint32_t* counts;   // [bags] or null: the known entries of each bag
};

// pool_known_trained<HAS_SUB, FAST, VEC4, OUT>, OUT a MEMB_HIP_OUT_*; null where no instance exists (HAS_SUB with FAST, an
// unknown type). VEC4: pool_trained's piece form (dim a multiple of 4 and at most TRAINED_VEC4_MAX_DIM, out / ld / colOff
// aligned to a piece of four elements); else fp32: the column form that parks partial sums in the bag's columns of `out`,
// bf16 / fp16: register blocks of 512 columns, one walk of the bag each
const void* trainedKernelKnown(bool hasSub, bool fast, bool vec4, int outType);
// pool_known_uniform<OUT> / pool_known_full<OUT>: one wavefront per bag, blocks of ROWWISE_WAVES wavefronts
const void* uniformKernelKnown(int outType);
const void* fullKernelKnown(int outType);

}  // namespace memb_pooled
