// hip_analogies_launch.h's argument checks as a program of its own, for the host sanitizers
// (-fsanitize=address,undefined): every refusal the two excluding calls add, what they accept, the refusals of the weighted
// sum, and the slice plan they share with the plain calls -- the figures tests/cpp/query_topk_planning_main.cpp asserts for
// the same sizes. No GPU, no HIP runtime: MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_analogies.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"
#include "../../memb_amd/csrc/hip_analogies_launch.h"

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

// The excluding calls plan with the plain calls' functions: the same segments, lists, slices and workspaces.
void sharedPlan()
{
    expect(planTopkSegments(1, 1024).segments == 1 && planTopkSegments(1, 1025).segments == 2, "two segments from 1025 columns on");
    expect(planTopkSegments(64, 2196017).segments == 127 && planTopkSegments(64, 2196017).segmentLength == 17408, "64 queries over 2.2 M words");
    expect(planTopkSegments(1, 2196017).segments == 253 && planTopkSegments(1, 2196017).segmentLength == 8704, "one query over 2.2 M words");
    expect(denseTopkWorkspaceBytes(3, 2049, 10) == 3 * 3 * 10 * 8, "three rows, three segments, k = 10");
    expect(queryTopkListBytes(64, 10) == 64 * 128 * 10 * 8 && queryTopkListBytes(1, 64) == 256 * 64 * 8, "lists");
    expect(topkRecommendedSlice(64) == 131072 && topkRecommendedSlice(1) == (8u << 20) && topkRecommendedSlice(16) == 524288, "32 MiB of matrix");
    expect(queryTopkWorkspaceBytes(64, 2196017, 10, false) == 64 * 128 * 10 * 8 + 4ull * 64 * 131072, "recommended, 64 queries");
    expect(queryTopkWorkspaceBytes(64, 2196017, 10, true) == 64 * 128 * 10 * 8 + 4ull * 64 * 64, "minimal: slices of 64");
    const uint64_t queries[] = {1, 2, 5, 64, 1 << 16};
    const uint64_t sizes[] = {1, 63, 64, 65, 200, 50000, 2196017, 1ull << 36};
    const uint64_t ranks[] = {1, 10, 64};
    for (uint64_t q : queries) {
        for (uint64_t n : sizes) {
            for (uint64_t k : ranks) {
                const uint64_t least = queryTopkWorkspaceBytes(q, n, k, true), good = queryTopkWorkspaceBytes(q, n, k, false);
                expect(planTopkSlice(q, n, k, least) == std::min<uint64_t>(n, MIN_SLICE), "the minimal workspace: 64 candidates", q, n);
                expect(planTopkSlice(q, n, k, least - 1) == 0, "one byte less is refused", q, n);
                expect(planTopkSlice(q, n, k, good) == std::min(n, topkRecommendedSlice(q)), "the recommended slice", q, n);
            }
        }
    }
    // 1100 candidates under the minimal workspace: eighteen slices
    expect((1100 + planTopkSlice(3, 1100, 10, queryTopkWorkspaceBytes(3, 1100, 10, true)) - 1) / 64 == 18, "eighteen slices of 64");
}

void excludedLists()
{
    static_assert(memb_analogies::MAX_EXCLUDED == 64, "the values below");
    std::vector<int64_t> list(3 * 70 + 1);
    const int64_t* e = list.data();   // (never dereferenced)
    expect(!excludedListRefusal(e, 64, 64), "the widest list");
    expect(!excludedListRefusal(e, 3, 70), "rows further apart than they are wide");
    expect(!excludedListRefusal(e + 1, 1, 1), "aligned to 8 bytes");
    expect(!excludedListRefusal(nullptr, 0, 0), "no list at all");
    expect(!excludedListRefusal(nullptr, 0, 5) && !excludedListRefusal(e, 0, 0), "width 0: the pointer is not looked at");
    expect(refusedWith(excludedListRefusal(e, 65, 65), "at most 64"), "width 65");
    expect(refusedWith(excludedListRefusal(e, ~size_t(0), ~size_t(0)), "at most 64"), "the largest width");
    expect(refusedWith(excludedListRefusal(e, 3, 2), "ld_excluded"), "ld_excluded < width");
    expect(refusedWith(excludedListRefusal(e, 64, 0), "ld_excluded"), "ld_excluded == 0");
    expect(refusedWith(excludedListRefusal(nullptr, 1, 1), "null"), "a null list with width > 0");
    const char* raw = reinterpret_cast<const char*>(list.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(excludedListRefusal(reinterpret_cast<const int64_t*>(raw + shift), 3, 3), "aligned"), "a misaligned list", shift);
        expect(refusedWith(excludedListRefusal(reinterpret_cast<const int64_t*>(raw + shift), 0, 0), "aligned"), "misaligned with width 0", shift);
    }
}

void weightedSums()
{
    std::vector<float> matrix(4 * 9 + 1), weights(5), out(2 * 9 + 1);
    std::vector<uint32_t> offsets(4);
    const float* m = matrix.data();
    const float* w = weights.data();
    const uint32_t* o = offsets.data();
    float* r = out.data();
    expect(!weightedRowsSumRefusal(0, m, 9, w, o, 2, 7, r, 9), "a good call");
    expect(!weightedRowsSumRefusal(0, m + 1, 7, nullptr, o + 1, 2, 7, r + 1, 7), "no weights, aligned to 4 bytes only, ld == dim");
    expect(!weightedRowsSumRefusal(0, nullptr, 7, nullptr, o, 2, 7, r, 7), "no matrix: no sum has an entry");
    expect(!weightedRowsSumRefusal(0, m, 0, w, o, 0, 0, r, 0), "nothing to do");
    expect(refusedWith(weightedRowsSumRefusal(-1, m, 9, w, o, 2, 7, r, 9), "device"), "a negative device");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, nullptr, 2, 7, r, 9), "null"), "null offsets");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, o, 2, 7, nullptr, 9), "null"), "null out");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 6, w, o, 2, 7, r, 9), "at least dim"), "ld < dim");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, o, 2, 7, r, 6), "at least dim"), "ld_out < dim");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, o, (1ull << 24) + 1, 7, r, 9), "too large"), "n_sums > 2^24");
    expect(refusedWith(weightedRowsSumRefusal(0, m, 1 << 17, w, o, 2, (1 << 16) + 1, r, 1 << 17), "too large"), "dim > 2^16");
    const char* raw = reinterpret_cast<const char*>(matrix.data());
    for (int shift = 1; shift < 4; ++shift) {   // (never dereferenced)
        expect(refusedWith(weightedRowsSumRefusal(0, reinterpret_cast<const float*>(raw + shift), 9, w, o, 2, 7, r, 9), "aligned"), "matrix", shift);
        expect(refusedWith(weightedRowsSumRefusal(0, m, 9, reinterpret_cast<const float*>(raw + shift), o, 2, 7, r, 9), "aligned"), "weights", shift);
        expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, reinterpret_cast<const uint32_t*>(raw + shift), 2, 7, r, 9), "aligned"), "offsets", shift);
        expect(refusedWith(weightedRowsSumRefusal(0, m, 9, w, o, 2, 7, reinterpret_cast<float*>(const_cast<char*>(raw) + shift), 9), "aligned"), "out", shift);
    }
}

}  // namespace

int main()
{
    sharedPlan();
    excludedLists();
    weightedSums();
    if (failures) {
        std::printf("analogies planning: %d failures\n", failures);
        return 1;
    }
    std::printf("analogies planning: ok\n");
    return 0;
}
