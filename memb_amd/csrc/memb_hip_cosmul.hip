// 3CosMul scores (gensim's most_similar_cosmul), gfx950 / CDNA4 (include/memb_hip_cosmul.h): the stage between the cosine
// matrix of a question's terms and the selection of the k best candidates.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches the kernel
// (hip_cosmul_launch.h) through the selector below (hip_cosmul.h).
//   cosmul_scores   one thread per (question, column) of a dense fp32 matrix of cosines, one row per term:
//                   num = product of (1 + c) * 0.5 over the question's positive terms, den likewise over its negative ones,
//                   score = num / (den + 1e-6), every operation rounded to float32, in the order of the terms
// HBM-bound: (terms + 1) * 4 bytes per element. No atomics, no LDS, no scratch, nothing allocated; every result depends on
// the inputs alone.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_cosmul.h"
#include "hip_cosmul.h"

namespace {

#include "hip_cosmul_kernels.h"

__global__ __launch_bounds__(memb_cosmul::SCORE_THREADS) void cosmul_scores(CosmulParams p)
{
    cosmulScoreOfThread(p);
}

}  // namespace

namespace memb_cosmul {

memb::KernelHandle scoresKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&cosmul_scores), "cosmul_scores"};
}

}  // namespace memb_cosmul
