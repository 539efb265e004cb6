// hip_cosmul_launch.h's first part as a program of its own, for the host sanitizers (-fsanitize=address,undefined): every
// refusal of the two calls, what they accept, and how the workspace is cut into lists, cosines and scores and the candidates
// into slices. No GPU, no HIP runtime: MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_cosmul.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"
#include "../../memb_amd/csrc/hip_analogies_launch.h"
#include "../../memb_amd/csrc/hip_cosmul_launch.h"

namespace {

using namespace memb_query_topk;

int failures = 0;

void expect(bool condition, const char* what, long long a = 0, long long b = 0)
{
    if (!condition) {
        std::printf("FAILED: %s (%lld, %lld)\n", what, a, b);
        ++failures;
    }
}

bool refusedWith(const char* refusal, const char* word)
{
    return refusal && std::strstr(refusal, word);
}

void scores()
{
    static_assert(memb_cosmul::MAX_TERMS == 64 && memb_cosmul::MAX_QUESTIONS == (1u << 16), "the values below");
    std::vector<float> matrix(3 * 9 + 1), out(2 * 9 + 1);
    std::vector<uint32_t> offsets(4), negatives(3);
    const float* m = matrix.data();
    const uint32_t* o = offsets.data();
    const uint32_t* f = negatives.data();
    float* r = out.data();
    expect(!cosmulScoresRefusal(0, m, 9, o, f, 2, 7, r, 9), "a good call");
    expect(!cosmulScoresRefusal(0, m + 1, 7, o + 1, f + 1, 2, 7, r + 1, 7), "aligned to 4 bytes only, ld == n");
    expect(!cosmulScoresRefusal(0, nullptr, 0, o, f, 2, 0, r, 0), "no column: no matrix is needed");
    expect(!cosmulScoresRefusal(0, m, 9, o, f, 0, 7, r, 9), "no question");
    expect(!cosmulScoresRefusal(0, m, 1ull << 31, o, f, 1ull << 16, 1ull << 31, r, 1ull << 31), "the largest sizes");
    expect(refusedWith(cosmulScoresRefusal(-1, m, 9, o, f, 2, 7, r, 9), "device"), "a negative device");
    expect(refusedWith(cosmulScoresRefusal(0, m, 9, nullptr, f, 2, 7, r, 9), "null"), "null offsets");
    expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, nullptr, 2, 7, r, 9), "null"), "null negatives_from");
    expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, f, 2, 7, nullptr, 9), "null"), "null scores");
    expect(refusedWith(cosmulScoresRefusal(0, nullptr, 9, o, f, 2, 7, r, 9), "cosines"), "null cosines with n > 0");
    expect(refusedWith(cosmulScoresRefusal(0, m, 6, o, f, 2, 7, r, 9), "at least n"), "ld < n");
    expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, f, 2, 7, r, 6), "at least n"), "ld_scores < n");
    expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, f, (1ull << 16) + 1, 7, r, 9), "too large"), "n_questions > 2^16");
    expect(refusedWith(cosmulScoresRefusal(0, m, 1ull << 32, o, f, 2, (1ull << 31) + 1, r, 1ull << 32), "too large"), "n > 2^31");
    const char* raw = reinterpret_cast<const char*>(matrix.data());
    for (int shift = 1; shift < 4; ++shift) {   // (never dereferenced)
        expect(refusedWith(cosmulScoresRefusal(0, reinterpret_cast<const float*>(raw + shift), 9, o, f, 2, 7, r, 9), "aligned"), "cosines", shift);
        expect(refusedWith(cosmulScoresRefusal(0, m, 9, reinterpret_cast<const uint32_t*>(raw + shift), f, 2, 7, r, 9), "aligned"), "offsets", shift);
        expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, reinterpret_cast<const uint32_t*>(raw + shift), 2, 7, r, 9), "aligned"), "negatives_from", shift);
        expect(refusedWith(cosmulScoresRefusal(0, m, 9, o, f, 2, 7, reinterpret_cast<float*>(const_cast<char*>(raw) + shift), 9), "aligned"), "scores", shift);
    }
    expect(cosmulBlocksPerQuestion(1) == 1 && cosmulBlocksPerQuestion(256) == 1 && cosmulBlocksPerQuestion(257) == 2, "blocks of 256 columns");
    expect(cosmulBlocksPerQuestion(1ull << 31) == (1u << 23), "2^31 columns");
    // every block of the largest grid lies inside one question, and too many blocks are refused by the launch (0 blocks)
    expect(memb::gridBlocks(1, 1, (1ull << 16) * cosmulBlocksPerQuestion(2196017)) == 65536u * 8579u, "2^16 questions over 2.2 M words");
    expect(memb::gridBlocks(1, 1, (1ull << 16) * cosmulBlocksPerQuestion(1ull << 31)) == 0, "2^39 blocks are no launch");
}

void workspace()
{
    // the lists are the selection's over the questions; the slice is planned from terms + questions rows
    expect(cosmulRecommendedSlice(3, 1) == topkRecommendedSlice(4) && topkRecommendedSlice(4) == (2u << 20), "an analogy: four rows");
    expect(cosmulRecommendedSlice(48, 16) == 131072, "16 analogies: 64 rows");
    expect(cosmulWorkspaceBytes(3, 1, 2196017, 10, false) == queryTopkListBytes(1, 10) + 4ull * 4 * (2u << 20), "recommended, one analogy");
    expect(cosmulWorkspaceBytes(3, 1, 2196017, 10, true) == queryTopkListBytes(1, 10) + 4ull * 4 * 64, "minimal: slices of 64");
    expect(cosmulWorkspaceBytes(192, 64, 1000, 64, false) == queryTopkListBytes(64, 64) + 4ull * 256 * 1000, "fewer candidates than a slice");
    expect(cosmulWorkspaceBytes(0, 5, 1000, 3, true) == queryTopkListBytes(5, 3) + 4ull * 5 * 64, "questions without any term");
    expect(cosmulWorkspaceBytes(3, 0, 1000, 3, false) == 0 && cosmulWorkspaceBytes(3, 1, 0, 3, false) == 0, "nothing to do");
    expect(cosmulWorkspaceBytes(3, 1, 1000, 0, false) == 0 && cosmulWorkspaceBytes(3, 1, 1000, 65, false) == 0, "k refused");
    expect(cosmulWorkspaceBytes((1 << 16) + 1, 1, 1000, 3, false) == 0 && cosmulWorkspaceBytes(3, (1 << 16) + 1, 1000, 3, false) == 0, "sizes refused");
    const uint64_t terms[] = {0, 1, 3, 48, 4096, 1 << 16};
    const uint64_t questions[] = {1, 2, 16, 64, 1 << 16};
    const uint64_t sizes[] = {1, 63, 64, 65, 200, 50000, 2196017, 1ull << 36};
    const uint64_t ranks[] = {1, 10, 64};
    for (uint64_t t : terms) {
        for (uint64_t q : questions) {
            for (uint64_t n : sizes) {
                for (uint64_t k : ranks) {
                    const uint64_t least = cosmulWorkspaceBytes(t, q, n, k, true), good = cosmulWorkspaceBytes(t, q, n, k, false);
                    expect(planCosmulSlice(t, q, n, k, least) == std::min<uint64_t>(n, MIN_SLICE), "the minimal workspace: 64 candidates", t, n);
                    expect(planCosmulSlice(t, q, n, k, least - 1) == 0, "one byte less is refused", t, n);
                    const uint64_t slice = planCosmulSlice(t, q, n, k, good);
                    expect(slice == std::min(n, cosmulRecommendedSlice(t, q)), "the recommended slice", t, n);
                    // the three areas lie inside the workspace
                    expect(queryTopkListBytes(q, k) + 4 * t * slice + 4 * q * slice <= good, "lists, cosines and scores fit", t, n);
                    expect(slice <= MAX_SLICE && slice <= memb_cosmul::MAX_COLUMNS, "a slice's columns fit 32 bits", t, n);
                }
            }
        }
    }
    expect(planCosmulSlice(3, 1, 1100, 10, ~uint64_t(0)) == 1100, "any larger workspace: one slice");
    expect(planCosmulSlice(3, 1, 1ull << 36, 10, ~uint64_t(0)) == MAX_SLICE, "never wider than MAX_SLICE");
    expect((1100 + planCosmulSlice(3, 1, 1100, 10, cosmulWorkspaceBytes(3, 1, 1100, 10, true)) - 1) / 64 == 18, "eighteen slices of 64");
}

void nearest()
{
    std::vector<float> terms(4 * 300 + 1), values(2 * 10 + 1);
    std::vector<uint32_t> offsets(4), negatives(3), rows(50);
    std::vector<int64_t> positions(2 * 10 + 1), list(2 * 4 + 1), space(1 << 16);
    const float* t = terms.data();
    const uint32_t* o = offsets.data();
    const uint32_t* f = negatives.data();
    const uint32_t* r = rows.data();
    const int64_t* e = list.data();
    const float* v = values.data();
    const int64_t* p = positions.data();
    const void* w = space.data();
    const size_t bytes = space.size() * 8;
    expect(bytes >= cosmulWorkspaceBytes(4, 2, 50, 10, false), "the workspace of the good call");
    expect(!cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "a good call");
    expect(!cosmulNearestArgumentsRefusal(t, 4, 301, 300, o, f, 2, r, 50, 10, nullptr, 0, 0, v, p, 12, w, bytes), "no list, strided");
    expect(!cosmulNearestArgumentsRefusal(nullptr, 0, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "no term at all");
    expect(!cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, nullptr, 0, 10, e, 4, 4, v, p, 10, nullptr, 0), "no candidate: no workspace");
    expect(!cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 0, r, 50, 10, nullptr, 0, 0, v, p, 10, nullptr, 0), "no question: no workspace");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 0, e, 4, 4, v, p, 10, w, bytes), "k must"), "k == 0");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 65, e, 4, 4, v, p, 65, w, bytes), "k must"), "k == 65");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, nullptr, p, 10, w, bytes), "null"), "null values");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, nullptr, 10, w, bytes), "null"), "null positions");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 9, w, bytes), "ld_out"), "ld_out < k");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, (1 << 16) + 1, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "2^16 terms"), "n_terms > 2^16");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, (1 << 16) + 1, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "2^16 questions"), "n_questions > 2^16");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, nullptr, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "offsets"), "null offsets");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, nullptr, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "negatives_from"), "null negatives_from");
    expect(refusedWith(cosmulNearestArgumentsRefusal(nullptr, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "queries"), "null terms");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, nullptr, 50, 10, e, 4, 4, v, p, 10, w, bytes), "rows"), "null rows");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 299, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "ld_queries"), "ld_terms < dim");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, (1ull << 36) + 1, 10, e, 4, 4, v, p, 10, w, bytes), "too large"), "n > 2^36");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 65, 65, v, p, 10, w, bytes), "at most 64"), "width 65");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 3, v, p, 10, w, bytes), "ld_excluded"), "ld_excluded < width");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, nullptr, 4, 4, v, p, 10, w, bytes), "null"), "a null list");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, nullptr, bytes), "workspace"), "a null workspace");
    const uint64_t least = cosmulWorkspaceBytes(4, 2, 50, 10, true);
    expect(!cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, least), "the minimal workspace");
    expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, least - 1), "workspace too small"), "one byte less");
    const char* raw = reinterpret_cast<const char*>(space.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, raw + shift, bytes - 8), "aligned"), "workspace", shift);
        expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, reinterpret_cast<const int64_t*>(raw + shift), 10, w, bytes), "aligned"), "positions", shift);
        expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, f, 2, r, 50, 10, reinterpret_cast<const int64_t*>(raw + shift), 4, 4, v, p, 10, w, bytes), "aligned"), "excluded", shift);
    }
    for (int shift = 1; shift < 4; ++shift) {
        expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, reinterpret_cast<const uint32_t*>(raw + shift), f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "aligned"), "offsets", shift);
        expect(refusedWith(cosmulNearestArgumentsRefusal(t, 4, 300, 300, o, reinterpret_cast<const uint32_t*>(raw + shift), 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "aligned"), "negatives_from", shift);
        expect(refusedWith(cosmulNearestArgumentsRefusal(reinterpret_cast<const float*>(raw + shift), 4, 300, 300, o, f, 2, r, 50, 10, e, 4, 4, v, p, 10, w, bytes), "aligned"), "terms", shift);
    }
}

}  // namespace

int main()
{
    scores();
    workspace();
    nearest();
    if (failures) {
        std::printf("cosmul planning: %d failures\n", failures);
        return 1;
    }
    std::printf("cosmul planning: ok\n");
    return 0;
}
