// The kernel of memb_hip_cosmul.hip (include/memb_hip_cosmul.h: one 3CosMul score per (question, candidate) from the
// cosines of the question's terms) as memb_hip.hip launches it (hip_cosmul_launch.h): a host address for hipLaunchKernel,
// as memb::KernelHandle. The kernel takes ONE parameter, the CosmulParams below.
#pragma once

#include <cstdint>

#include "hip_analogies.h"   // (the selection the fused call hands its scores to: ExcludedList, and the limits beneath it)

namespace memb_cosmul {

struct CosmulParams {
    const float* cosines;              // term t: cosines[t * ld .. + n)
    const uint32_t* offsets;           // nQuestions + 1: question q takes the terms offsets[q] .. offsets[q + 1]
    const uint32_t* negativesFrom;     // nQuestions: the terms from negativesFrom[q] on are negative
    float* scores;                     // question q: scores[q * ldScores .. + n)
    unsigned long long ld;             // in floats, >= n
    unsigned long long ldScores;       // in floats, >= n
    uint32_t nQuestions;
    uint32_t n;                        // columns, at most MAX_COLUMNS
    uint32_t blocksPerQuestion;        // ceil(n / SCORE_THREADS): block b scores question b / blocksPerQuestion
};

constexpr uint32_t MAX_TERMS = 64;            // per question: MEMB_HIP_COSMUL_MAX_TERMS, the width of an exclusion list
constexpr uint32_t SCORE_THREADS = 256;       // cosmul_scores: one thread per (question, column), a block inside one question
constexpr uint32_t TERMS_IN_FLIGHT = 4;       // term loads issued before the first is multiplied in (geometry, never the result)
constexpr uint64_t MAX_QUESTIONS = 1ull << 16;
constexpr uint64_t MAX_COLUMNS = 1ull << 31;  // columns travel as 32 bits
constexpr uint64_t MAX_TERM_ROWS = 1ull << 16;   // of the fused call: the matrix kernel's limit on its queries

// cosmul_scores: nQuestions * blocksPerQuestion blocks of SCORE_THREADS threads, neighbouring lanes on neighbouring
// columns of one question. No LDS.
memb::KernelHandle scoresKernel();

}  // namespace memb_cosmul
