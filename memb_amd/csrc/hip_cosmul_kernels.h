// Device code of memb_hip_cosmul.hip: the 3CosMul score of one (question, column). Included inside the unit's anonymous
// namespace.
#pragma once

using memb_cosmul::CosmulParams;

// cosmul_scores: the thread's output element (question q, column c). A block lies inside one question, so q, its offsets
// and every branch on them are wave-uniform, and neighbouring lanes read neighbouring columns of the same term row. The
// loads of a question's terms do not depend on one another: TERMS_IN_FLIGHT of them are issued, without a branch between
// them, before the first is multiplied in, in the order the contract fixes -- num over the positive terms, den over the
// negative ones, every operation one rounded float32 operation whatever the compiler's contraction setting.
__device__ __forceinline__ void cosmulScoreOfThread(const CosmulParams& p)
{
    const uint32_t question = blockIdx.x / p.blocksPerQuestion;
    const uint32_t column = (blockIdx.x % p.blocksPerQuestion) * memb_cosmul::SCORE_THREADS + threadIdx.x;
    if (question >= p.nQuestions || column >= p.n) {
        return;
    }
    const uint32_t begin = p.offsets[question];
    const uint32_t negativesFrom = p.negativesFrom[question];
    const uint32_t end = p.offsets[question + 1];
    const float* cosines = p.cosines + column;
    float num = 1.0f;
    float den = 1.0f;
    for (uint32_t first = begin; first < end; first += memb_cosmul::TERMS_IN_FLIGHT) {
        const uint32_t count = end - first;   // (>= 1; a term is `first + step` with step < count, so it cannot wrap)
        float loaded[memb_cosmul::TERMS_IN_FLIGHT];
#pragma unroll
        for (uint32_t step = 0; step < memb_cosmul::TERMS_IN_FLIGHT; ++step) {
            // (no branch between the loads: a step behind the question's last term reads that term again and is not used)
            const uint32_t term = first + (step < count ? step : count - 1);
            loaded[step] = cosines[static_cast<unsigned long long>(term) * p.ld];
        }
#pragma unroll
        for (uint32_t step = 0; step < memb_cosmul::TERMS_IN_FLIGHT; ++step) {
            const float shifted = __fmul_rn(__fadd_rn(1.0f, loaded[step]), 0.5f);
            const float nextNum = __fmul_rn(num, shifted);
            const float nextDen = __fmul_rn(den, shifted);
            const bool positive = first + step < negativesFrom;   // (wave-uniform, as is step < count)
            num = step < count && positive ? nextNum : num;
            den = step < count && !positive ? nextDen : den;
        }
    }
    p.scores[static_cast<unsigned long long>(question) * p.ldScores + column] = __fdiv_rn(num, __fadd_rn(den, 1e-6f));
}
