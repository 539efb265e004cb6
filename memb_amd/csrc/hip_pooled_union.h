// The kernels of memb_hip_pooled_union.hip (include/memb_hip_pooled_union.h: the sum or mean of each bag of a ReadersUnion's
// AVERAGED rows, and of each bag of rows of a dense fp32 matrix) as memb_hip.hip launches them (hip_pooled_launch.h: launchPooledUnion,
// launchPooledDense): host addresses for hipLaunchKernel / hipFuncGetAttributes, in the style of hip_pooled.h. The first
// parameter of the union kernels is the UnionParams of hip_trained_kernels.h, which both translation units include -- every
// model's rows[0 .. n) are the ENTRIES, model 0's out / ld / colOff describe the bags' rows --, that of the dense kernels
// the DenseParams below; the second is hip_pooled.h's PoolParams.
#pragma once

#include <cstdint>

#include "hip_pooled.h"

namespace memb_pooled {

// The "row ids" of a dense matrix: entry i is row i. What poolBagOfWave reads as p.rows[i].
struct EntryIds {
    __host__ __device__ unsigned long long operator[](unsigned long long i) const { return i; }
};

struct DenseParams {
    EntryIds rows;
    const float* values;          // entry i: values[i * ldValues .. + dim)
    float* out;                   // (2-byte elements for a narrow type)
    unsigned long long n;
    unsigned long long ld;        // of out, in elements
    unsigned long long colOff;
    unsigned long long ldValues;  // in floats
    uint32_t dim;
};

// pool_trained_union<HAS_SUB, FAST, COUNT, OUT>: COUNT trained models of one geometry (launchTrainedUnion's conditions),
// register accumulators of 16-byte pieces (dim a multiple of 4 and at most TRAINED_VEC4_MAX_DIM, out / ld / colOff aligned
// to a piece). address is null where no instance exists: a count outside 2 .. 4, HAS_SUB with FAST, an unknown outType.
memb::KernelHandle pooledUnionKernel(bool hasSub, bool fast, int count, int outType);

// pool_dense<OUT>: one wavefront per bag, blocks of ROWWISE_WAVES wavefronts, any dim and alignment.
memb::KernelHandle pooledDenseKernel(int outType);

}  // namespace memb_pooled
