// The kernels of memb_hip_norms.hip (include/memb_hip_norms.h: the norm of each row and rows of unit length, from the
// compressed rows of a trained model or from a dense fp32 matrix) as memb_hip.hip launches them (hip_norms_launch.h): host
// addresses for hipLaunchKernel / hipFuncGetAttributes, as memb::KernelHandle (hip_kernel_handle.h). The first parameter
// of the trained kernels is the TrainedParams of hip_trained_kernels.h, which both translation units include -- rows[0 ..
// n) are the rows, out / ld / colOff describe the unit rows --, their second the NormParams below; the dense kernels take
// the DenseNormParams.
#pragma once

#include <cstdint>

#include "hip_pooled.h"   // (the unit builds on pool_trained's device code, which takes the PoolParams; ROWWISE_WAVES)

namespace memb_norms {

struct NormParams {
    float* norms;           // [n] or null (unit_trained only: the norms are not wanted)
    uint32_t rowsPerWave;   // consecutive rows a wavefront owns (launch geometry, never the result)
};

struct DenseNormParams {
    const float* values;          // row i: values[i * ldValues .. + dim)
    float* out;                   // unit_dense: row i goes to out + i * ld + colOff (may be `values`' own columns)
    float* norms;                 // [n]; unit_dense: or null
    unsigned long long n;
    unsigned long long ld;        // of out, in floats
    unsigned long long colOff;
    unsigned long long ldValues;  // in floats
    uint32_t dim;
};

constexpr uint32_t DENSE_WAVES = memb_pooled::ROWWISE_WAVES;              // one row per wavefront

// norms_trained<HAS_SUB, FAST> (unit: unit_trained<HAS_SUB, FAST>): dim a multiple of 4 and at most
// memb_pooled::TRAINED_VEC4_MAX_DIM (two pieces per lane: the contract's layout); the unit rows' out / ld / colOff aligned
// to a piece. LDS and block size are pool_trained's (an fp32 codebook). address: null where no instance exists, HAS_SUB
// with FAST.
memb::KernelHandle trainedKernel(bool hasSub, bool fast, bool unit);

// norms_dense / unit_dense: one wavefront per row, blocks of DENSE_WAVES wavefronts, any dim and alignment.
memb::KernelHandle denseKernel(bool unit);

}  // namespace memb_norms
