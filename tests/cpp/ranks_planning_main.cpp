// hip_ranks_launch.h's first part as a program of its own, for the host sanitizers (-fsanitize=address,undefined): every
// refusal of the two calls, what they accept, and how the workspace is cut into partial counts and cosines and the
// candidates into slices. No GPU, no HIP runtime: MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_ranks.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"
#include "../../memb_amd/csrc/hip_analogies_launch.h"
#include "../../memb_amd/csrc/hip_ranks_launch.h"

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

void dense()
{
    static_assert(memb_ranks::BLOCK_RUN == 2048 && memb_ranks::MAX_ROWS == (1u << 16) && memb_ranks::MAX_COLUMNS == (1ull << 31), "the values below");
    std::vector<float> matrix(2 * 9 + 1), thresholds(3);
    std::vector<int64_t> marks(3), list(2 * 4 + 1), counts(3), space(16);
    const float* m = matrix.data();
    const float* t = thresholds.data();
    const int64_t* p = marks.data();
    const int64_t* e = list.data();
    const int64_t* c = counts.data();
    const void* w = space.data();
    expect(!denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, c, w, 8), "a good call");
    expect(!denseRanksArgumentsRefusal(0, m + 1, 2, 7, 7, 5, t + 1, p + 1, nullptr, 0, 0, c + 1, w, 8), "aligned to 4 bytes only, ld == n, no list");
    expect(!denseRanksArgumentsRefusal(0, nullptr, 2, 0, 0, 0, t, p, e, 4, 4, c, nullptr, 0), "no column: neither a matrix nor a workspace");
    expect(!denseRanksArgumentsRefusal(0, m, 0, 7, 9, 0, t, p, e, 4, 4, c, nullptr, 0), "no row: no workspace");
    expect(!denseRanksArgumentsRefusal(0, m, 1ull << 16, 1ull << 31, 1ull << 31, 0, t, p, e, 4, 4, c, w, ~size_t(0)), "the largest sizes");
    expect(refusedWith(denseRanksArgumentsRefusal(-1, m, 2, 7, 9, 0, t, p, e, 4, 4, c, w, 8), "device"), "a negative device");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, -1, t, p, e, 4, 4, c, w, 8), "base"), "a negative base");
    expect(refusedWith(denseRanksArgumentsRefusal(0, nullptr, 2, 7, 9, 0, t, p, e, 4, 4, c, w, 8), "matrix"), "null matrix with n > 0");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 6, 0, t, p, e, 4, 4, c, w, 8), "at least n"), "ld < n");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, nullptr, p, e, 4, 4, c, w, 8), "null"), "null thresholds");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, nullptr, e, 4, 4, c, w, 8), "null"), "null marks");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, nullptr, w, 8), "null"), "null counts");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 65, 65, c, w, 8), "at most 64"), "width 65");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 3, c, w, 8), "ld_excluded"), "ld_excluded < width");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, nullptr, 4, 4, c, w, 8), "null"), "a null list");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, (1ull << 16) + 1, 7, 9, 0, t, p, e, 4, 4, c, w, ~size_t(0)), "too large"), "n_rows > 2^16");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, (1ull << 31) + 1, 1ull << 32, 0, t, p, e, 4, 4, c, w, ~size_t(0)), "too large"), "n > 2^31");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, c, nullptr, 8), "workspace"), "a null workspace");
    expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, c, w, 7), "workspace too small"), "one byte less");
    const char* raw = reinterpret_cast<const char*>(space.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, reinterpret_cast<const int64_t*>(raw + shift), e, 4, 4, c, w, 8), "aligned"), "marks", shift);
        expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, reinterpret_cast<const int64_t*>(raw + shift), 4, 4, c, w, 8), "aligned"), "excluded", shift);
        expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, reinterpret_cast<const int64_t*>(raw + shift), w, 8), "aligned"), "counts", shift);
        expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, t, p, e, 4, 4, c, raw + shift, 8), "aligned"), "workspace", shift);
    }
    for (int shift = 1; shift < 4; ++shift) {
        expect(refusedWith(denseRanksArgumentsRefusal(0, reinterpret_cast<const float*>(raw + shift), 2, 7, 9, 0, t, p, e, 4, 4, c, w, 8), "aligned"), "matrix", shift);
        expect(refusedWith(denseRanksArgumentsRefusal(0, m, 2, 7, 9, 0, reinterpret_cast<const float*>(raw + shift), p, e, 4, 4, c, w, 8), "aligned"), "thresholds", shift);
    }
    expect(rankBlocksPerRow(0) == 0 && rankBlocksPerRow(1) == 1 && rankBlocksPerRow(2048) == 1 && rankBlocksPerRow(2049) == 2, "blocks of 2048 columns");
    expect(rankBlocksPerRow(1ull << 31) == (1u << 20), "2^31 columns");
    expect(denseRanksWorkspaceBytes(2, 7) == 8 && denseRanksWorkspaceBytes(3, 2049) == 24 && denseRanksWorkspaceBytes(1, 2048) == 8, "4 bytes per block, rounded to 8");
    expect(denseRanksWorkspaceBytes(5, 0) == 0 && denseRanksWorkspaceBytes(0, 5) == 0, "nothing to count");
    expect(denseRanksWorkspaceBytes((1 << 16) + 1, 7) == 0 && denseRanksWorkspaceBytes(2, (1ull << 31) + 1) == 0, "sizes refused");
    // every block of the largest grid lies inside one row, and too many blocks are refused by the launch (0 blocks)
    expect(memb::gridBlocks(1, 1, (1ull << 16) * rankBlocksPerRow(2196017)) == 65536u * 1073u, "2^16 rows over 2.2 M words");
    expect(memb::gridBlocks(1, 1, (1ull << 16) * rankBlocksPerRow(1ull << 31)) == 0, "2^36 blocks are no launch");
}

void workspace()
{
    expect(queryRanksWorkspaceBytes(1, 2196017, false) == rankPartialBytes(1, 2196017) + 4ull * 2196017, "one query: the model fits one slice");
    expect(queryRanksWorkspaceBytes(16, 2196017, false) == rankPartialBytes(16, 524288) + 4ull * 16 * 524288, "16 queries: slices of 32 MiB");
    expect(queryRanksWorkspaceBytes(16, 2196017, true) == 64 + 4ull * 16 * 64, "minimal: slices of 64, one block per query");
    expect(queryRanksWorkspaceBytes(3, 50, true) == 16 + 4ull * 3 * 50, "fewer candidates than a slice");
    expect(queryRanksWorkspaceBytes(0, 1000, false) == 0 && queryRanksWorkspaceBytes(3, 0, false) == 0, "nothing to do");
    expect(queryRanksWorkspaceBytes((1 << 16) + 1, 1000, false) == 0 && queryRanksWorkspaceBytes(3, (1ull << 36) + 1, false) == 0, "sizes refused");
    const uint64_t queries[] = {1, 2, 3, 16, 17, 64, 4096, 1 << 16};
    const uint64_t sizes[] = {1, 63, 64, 65, 200, 2047, 2048, 2049, 50000, 2196017, 1ull << 36};
    for (uint64_t q : queries) {
        for (uint64_t n : sizes) {
            const uint64_t least = queryRanksWorkspaceBytes(q, n, true), good = queryRanksWorkspaceBytes(q, n, false);
            expect(planRanksSlice(q, n, least) == std::min<uint64_t>(n, MIN_SLICE), "the minimal workspace: 64 candidates", q, n);
            expect(planRanksSlice(q, n, least - 1) == 0, "one byte less is refused", q, n);
            const uint64_t slice = planRanksSlice(q, n, good);
            expect(slice == std::min(n, topkRecommendedSlice(q)), "the recommended slice", q, n);
            // both areas lie inside the workspace, the cosines behind the partial counts and aligned to 8 bytes
            expect(rankPartialBytes(q, slice) % 8 == 0 && rankPartialBytes(q, slice) + 4 * q * slice <= good, "partial counts and cosines fit", q, n);
            expect(4 * q * rankBlocksPerRow(slice) <= rankPartialBytes(q, slice), "a partial count per block", q, n);
            expect(slice <= MAX_SLICE && slice <= memb_ranks::MAX_COLUMNS, "a slice's columns fit 32 bits", q, n);
            // anything between the two sizes: a multiple of 64 that fits, and 64 more would not
            const uint64_t between = least + (good - least) / 3;
            const uint64_t middle = planRanksSlice(q, n, between);
            expect(middle >= std::min<uint64_t>(n, MIN_SLICE) && middle <= slice && (middle == n || middle % MIN_SLICE == 0), "a slice in between", q, n);
            expect(rankSliceBytes(q, middle) <= between && (middle == n || middle == MAX_SLICE || rankSliceBytes(q, std::min(n, middle + MIN_SLICE)) > between),
                   "the largest multiple that fits", q, n);
        }
    }
    expect(planRanksSlice(3, 1100, ~uint64_t(0)) == 1100, "any larger workspace: one slice");
    expect(planRanksSlice(3, 1ull << 36, ~uint64_t(0)) == MAX_SLICE, "never wider than MAX_SLICE");
    expect((1100 + planRanksSlice(3, 1100, queryRanksWorkspaceBytes(3, 1100, true)) - 1) / 64 == 18, "eighteen slices of 64");
}

void fused()
{
    std::vector<float> queries(2 * 300 + 1), thresholds(3);
    std::vector<uint32_t> rows(50);
    std::vector<int64_t> marks(3), list(2 * 4 + 1), counts(3), space(1 << 12);
    const float* v = queries.data();
    const uint32_t* r = rows.data();
    const float* t = thresholds.data();
    const int64_t* p = marks.data();
    const int64_t* e = list.data();
    const int64_t* c = counts.data();
    const void* w = space.data();
    const size_t bytes = space.size() * 8;
    expect(bytes >= queryRanksWorkspaceBytes(2, 50, false), "the workspace of the good call");
    expect(!queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, c, w, bytes), "a good call");
    expect(!queryRanksArgumentsRefusal(v, 2, 301, 300, r, 50, t, p, nullptr, 0, 0, c, w, bytes), "no list, strided");
    expect(!queryRanksArgumentsRefusal(v, 2, 300, 300, nullptr, 0, t, p, e, 4, 4, c, nullptr, 0), "no candidate: no workspace");
    expect(refusedWith(queryRanksArgumentsRefusal(nullptr, 2, 300, 300, r, 50, t, p, e, 4, 4, c, w, bytes), "queries"), "null queries");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, nullptr, 50, t, p, e, 4, 4, c, w, bytes), "rows"), "null rows");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 299, 300, r, 50, t, p, e, 4, 4, c, w, bytes), "ld_queries"), "ld_queries < dim");
    expect(refusedWith(queryRanksArgumentsRefusal(v, (1 << 16) + 1, 300, 300, r, 50, t, p, e, 4, 4, c, w, bytes), "too large"), "n_queries > 2^16");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, (1ull << 36) + 1, t, p, e, 4, 4, c, w, bytes), "too large"), "n > 2^36");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, nullptr, p, e, 4, 4, c, w, bytes), "null"), "null thresholds");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, nullptr, e, 4, 4, c, w, bytes), "null"), "null marks");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, nullptr, w, bytes), "null"), "null counts");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 65, 65, c, w, bytes), "at most 64"), "width 65");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 3, c, w, bytes), "ld_excluded"), "ld_excluded < width");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, nullptr, 4, 4, c, w, bytes), "null"), "a null list");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, c, nullptr, bytes), "workspace"), "a null workspace");
    const uint64_t least = queryRanksWorkspaceBytes(2, 50, true);
    expect(!queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, c, w, least), "the minimal workspace");
    expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, c, w, least - 1), "workspace too small"), "one byte less");
    const char* raw = reinterpret_cast<const char*>(space.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, c, raw + shift, bytes - 8), "aligned"), "workspace", shift);
        expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, reinterpret_cast<const int64_t*>(raw + shift), e, 4, 4, c, w, bytes), "aligned"), "marks", shift);
        expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, reinterpret_cast<const int64_t*>(raw + shift), w, bytes), "aligned"), "counts", shift);
        expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, reinterpret_cast<const int64_t*>(raw + shift), 4, 4, c, w, bytes), "aligned"), "excluded", shift);
    }
    for (int shift = 1; shift < 4; ++shift) {
        expect(refusedWith(queryRanksArgumentsRefusal(reinterpret_cast<const float*>(raw + shift), 2, 300, 300, r, 50, t, p, e, 4, 4, c, w, bytes), "aligned"), "queries", shift);
        expect(refusedWith(queryRanksArgumentsRefusal(v, 2, 300, 300, r, 50, reinterpret_cast<const float*>(raw + shift), p, e, 4, 4, c, w, bytes), "aligned"), "thresholds", shift);
    }
}

}  // namespace

int main()
{
    dense();
    workspace();
    fused();
    if (failures) {
        std::printf("ranks planning: %d failures\n", failures);
        return 1;
    }
    std::printf("ranks planning: ok\n");
    return 0;
}
