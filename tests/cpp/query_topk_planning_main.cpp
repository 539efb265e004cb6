// hip_query_topk_launch.h's planning and argument checks as a program of its own, for the host sanitizers
// (-fsanitize=address,undefined): how a row is cut into segments, how the workspace decides the slices, the workspace
// bytes, every refusal of the two entry points, and the byte count by hand. No GPU, no HIP runtime:
// MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_query_topk.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"

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

void segments()
{
    static_assert(MIN_SEGMENT == 1024 && TARGET_WAVES == 8192 && MAX_SEGMENTS == 256 && BATCH * UNROLL == 256, "the values below");
    expect(topkMaxSegments(0) == 256 && topkMaxSegments(1) == 256 && topkMaxSegments(32) == 256, "few rows: the most lists one wavefront merges");
    expect(topkMaxSegments(33) == 249 && topkMaxSegments(64) == 128 && topkMaxSegments(8192) == 1 && topkMaxSegments(8193) == 1, "until 8192 wavefronts exist");
    expect(topkMaxSegments(1ull << 24) == 1, "many rows: one segment each");
    const uint64_t rows[] = {1, 2, 16, 64, 65, 1000, 8192, 1ull << 16, 1ull << 24};
    const uint64_t sizes[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 50000, 131072, 2196017, (1ull << 30) + 1, 1ull << 31};
    for (uint64_t r : rows) {
        for (uint64_t n : sizes) {
            const TopkSegments plan = planTopkSegments(r, n);
            expect(plan.segmentLength >= MIN_SEGMENT && plan.segmentLength % (BATCH * UNROLL) == 0, "whole unrolled batches", n, plan.segmentLength);
            expect(plan.segments <= topkMaxSegments(r), "never more lists than planned for", n, plan.segments);
            expect(uint64_t(plan.segments) * plan.segmentLength >= n, "the segments cover the columns", n, plan.segments);
            expect(n == 0 ? plan.segments == 0 : uint64_t(plan.segments - 1) * plan.segmentLength < n, "no empty segment", n, plan.segments);
            expect(r * plan.segments < (1ull << 32), "one launch", r, plan.segments);
        }
    }
    expect(planTopkSegments(1, 1024).segments == 1 && planTopkSegments(1, 1025).segments == 2, "two segments from 1025 columns on");
    expect(planTopkSegments(1, 2048).segments == 2 && planTopkSegments(1, 2049).segments == 3, "three from 2049 on");
    expect(planTopkSegments(64, 2196017).segments == 127 && planTopkSegments(64, 2196017).segmentLength == 17408, "64 queries over 2.2 M words");
    expect(planTopkSegments(1, 2196017).segments == 253 && planTopkSegments(1, 2196017).segmentLength == 8704, "one query over 2.2 M words");
    expect(planTopkSegments(1, 1ull << 31).segmentLength == (1u << 23), "the most columns");
    // NOT monotonic in n: a segment is a whole multiple of 256 columns, so fewer columns can be cut into more segments. A
    // caller who reuses one workspace for slices of several sizes sizes it for each of them (Reader.similarity_topk_device's
    // fallback does), or for topkMaxSegments as the fused call does.
    expect(planTopkSegments(33, 524288).segments == 228 && planTopkSegments(33, 509952).segments == 249, "33 queries: a shorter slice, more segments");
    expect(denseTopkWorkspaceBytes(33, 509952, 10) > denseTopkWorkspaceBytes(33, 524288, 10), "and more bytes of lists");
    expect(planTopkSegments(228, 37120).segments == 29 && planTopkSegments(228, 29952).segments == 30, "228 queries: 37 120 and 29 952 columns");
}

void workspaces()
{
    // the dense call: the lists alone, 8 bytes per rank
    expect(denseTopkWorkspaceBytes(3, 2049, 10) == 3 * 3 * 10 * 8, "three rows, three segments, k = 10");
    expect(denseTopkWorkspaceBytes(3, 0, 10) == 0 && denseTopkWorkspaceBytes(0, 100, 10) == 0, "nothing to select from");
    expect(denseTopkWorkspaceBytes(3, 100, 0) == 0 && denseTopkWorkspaceBytes(3, 100, 65) == 0, "k refused");
    expect(denseTopkWorkspaceBytes(3, (1ull << 31) + 1, 1) == 0 && denseTopkWorkspaceBytes((1ull << 24) + 1, 5, 1) == 0, "sizes refused");
    expect(denseTopkWorkspaceBytes(1ull << 24, 1ull << 31, 64) == (1ull << 24) * 64 * 8, "the largest call");
    // the fused call: lists for the most segments, then the slice's matrix
    expect(queryTopkListBytes(64, 10) == 64 * 128 * 10 * 8 && queryTopkListBytes(1, 64) == 256 * 64 * 8, "lists");
    expect(topkRecommendedSlice(64) == 131072 && topkRecommendedSlice(1) == (8u << 20) && topkRecommendedSlice(16) == 524288, "32 MiB of matrix");
    expect(topkRecommendedSlice(3) == 2796160 && topkRecommendedSlice(1 << 16) == 128 && topkRecommendedSlice(0) == (8u << 20), "whole blocks of 64 candidates");
    expect(queryTopkWorkspaceBytes(64, 2196017, 10, false) == 64 * 128 * 10 * 8 + 4ull * 64 * 131072, "recommended, 64 queries");
    expect(queryTopkWorkspaceBytes(64, 1ull << 36, 10, false) == queryTopkWorkspaceBytes(64, 2196017, 10, false), "independent of n beyond the slice");
    expect(queryTopkWorkspaceBytes(64, 50000, 10, false) == 64 * 128 * 10 * 8 + 4ull * 64 * 50000, "n below the slice: all of it");
    expect(queryTopkWorkspaceBytes(64, 2196017, 10, true) == 64 * 128 * 10 * 8 + 4ull * 64 * 64, "minimal: slices of 64");
    expect(queryTopkWorkspaceBytes(5, 7, 3, true) == 5 * 256 * 3 * 8 + 4 * 5 * 7 && queryTopkWorkspaceBytes(5, 7, 3, false) == queryTopkWorkspaceBytes(5, 7, 3, true), "seven candidates");
    expect(queryTopkWorkspaceBytes(0, 7, 3, false) == 0 && queryTopkWorkspaceBytes(5, 0, 3, false) == 0, "nothing needed");
    expect(queryTopkWorkspaceBytes(5, 7, 0, false) == 0 && queryTopkWorkspaceBytes(5, 7, 65, false) == 0, "k refused");
    expect(queryTopkWorkspaceBytes((1 << 16) + 1, 7, 3, false) == 0 && queryTopkWorkspaceBytes(5, (1ull << 36) + 1, 3, false) == 0, "sizes refused");
    // the slice a workspace gives
    const uint64_t queries[] = {1, 2, 5, 64, 1 << 16};
    const uint64_t sizes[] = {1, 63, 64, 65, 200, 50000, 2196017, 1ull << 36};
    const uint64_t ranks[] = {1, 10, 64};
    for (uint64_t q : queries) {
        for (uint64_t n : sizes) {
            for (uint64_t k : ranks) {
                const uint64_t least = queryTopkWorkspaceBytes(q, n, k, true), good = queryTopkWorkspaceBytes(q, n, k, false);
                expect(least <= good, "minimal is the smaller", q, n);
                expect(planTopkSlice(q, n, k, least) == std::min<uint64_t>(n, MIN_SLICE), "the minimal workspace: 64 candidates", q, n);
                expect(planTopkSlice(q, n, k, least - 1) == 0, "one byte less is refused", q, n);
                expect(planTopkSlice(q, n, k, good) == std::min(n, topkRecommendedSlice(q)), "the recommended slice", q, n);
                const uint64_t slice = planTopkSlice(q, n, k, good + 4 * q * 100);
                expect(slice == n || (slice % MIN_SLICE == 0 && slice < n), "whole blocks of 64 unless one slice takes all", q, n);
                expect(slice <= MAX_SLICE && queryTopkListBytes(q, k) + 4 * q * slice <= good + 4 * q * 100, "inside the workspace", q, n);
                expect(planTopkSegments(q, slice).segments <= topkMaxSegments(q), "the lists have room", q, n);
            }
        }
    }
    expect(planTopkSlice(1, 1ull << 36, 1, ~0ull) == MAX_SLICE, "never wider than 2^30");
}

void denseRefusals()
{
    std::vector<float> matrix(3 * 12 + 1), values(3 * 6 + 1);
    std::vector<int64_t> positions(3 * 6 + 1);
    std::vector<uint64_t> workspace(64);
    const float* m = matrix.data();
    float* v = values.data();
    int64_t* p = positions.data();
    void* w = workspace.data();
    const size_t bytes = workspace.size() * 8;
    expect(denseTopkWorkspaceBytes(3, 10, 5) == 120, "the workspace of the good call");
    expect(!denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, p, 6, w, bytes), "a good call");
    expect(!denseTopkArgumentsRefusal(0, m, 3, 10, 10, 1ll << 40, 5, v, p, 5, w, 120), "ld == n, ld_out == k, a base, the exact workspace");
    expect(!denseTopkArgumentsRefusal(0, m + 1, 3, 10, 12, 0, 5, v + 1, p + 1, 6, w, bytes), "matrix and values aligned to 4 bytes only");
    expect(!denseTopkArgumentsRefusal(0, nullptr, 3, 0, 0, 0, 5, v, p, 6, nullptr, 0), "no columns: neither matrix nor workspace");
    expect(!denseTopkArgumentsRefusal(0, nullptr, 0, 0, 0, 0, 5, v, p, 6, nullptr, 0), "no rows");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 0, v, p, 6, w, bytes), "k must"), "k == 0");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 65, v, p, 65, w, bytes), "k must"), "k > 64");
    expect(refusedWith(denseTopkArgumentsRefusal(0, nullptr, 3, 10, 12, 0, 5, v, p, 6, w, bytes), "null"), "null matrix");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, nullptr, p, 6, w, bytes), "null"), "null values");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, nullptr, 6, w, bytes), "null"), "null positions");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 9, 0, 5, v, p, 6, w, bytes), "ld must"), "ld < n");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, p, 4, w, bytes), "ld_out"), "ld_out < k");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, -1, 5, v, p, 6, w, bytes), "base"), "a negative base");
    expect(refusedWith(denseTopkArgumentsRefusal(-1, m, 3, 10, 12, 0, 5, v, p, 6, w, bytes), "device"), "a negative device");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, p, 6, nullptr, bytes), "workspace"), "null workspace");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, p, 6, w, 119), "workspace"), "workspace one byte short");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, (1ull << 31) + 1, ~size_t(0), 0, 5, v, p, 6, w, bytes), "too large"), "n > 2^31");
    expect(refusedWith(denseTopkArgumentsRefusal(0, m, (1ull << 24) + 1, 10, 12, 0, 5, v, p, 6, w, bytes), "too large"), "n_rows > 2^24");
    char* raw = reinterpret_cast<char*>(workspace.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, reinterpret_cast<int64_t*>(raw + shift), 6, w, bytes), "aligned"), "positions", shift);
        expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, v, p, 6, raw + shift, bytes - 8), "aligned"), "workspace", shift);
        if (shift % 4) {
            expect(refusedWith(denseTopkArgumentsRefusal(0, reinterpret_cast<const float*>(raw + shift), 3, 10, 12, 0, 5, v, p, 6, w, bytes), "aligned"), "matrix", shift);
            expect(refusedWith(denseTopkArgumentsRefusal(0, m, 3, 10, 12, 0, 5, reinterpret_cast<float*>(raw + shift), p, 6, w, bytes), "aligned"), "values", shift);
        }
    }
}

void fusedRefusals()
{
    std::vector<float> queries(2 * 303 + 1), values(2 * 12 + 1);
    std::vector<uint32_t> rows(200);
    std::vector<int64_t> positions(2 * 12 + 1);
    std::vector<uint64_t> workspace(1);
    const float* q = queries.data();
    const uint32_t* r = rows.data();
    float* v = values.data();
    int64_t* p = positions.data();
    void* w = workspace.data();   // (never dereferenced: the sizes below are only compared)
    const size_t least = queryTopkWorkspaceBytes(2, 200, 10, true);
    expect(least == 2 * 256 * 10 * 8 + 4 * 2 * 64, "the minimal workspace by hand");
    expect(!queryTopkArgumentsRefusal(q, 2, 303, 300, r, 200, 10, v, p, 12, w, least), "a good call with the minimal workspace");
    expect(!queryTopkArgumentsRefusal(q + 1, 2, 303, 300, r + 1, 199, 10, v + 1, p, 10, w, least), "aligned to 4 bytes only, ld_out == k");
    expect(!queryTopkArgumentsRefusal(q, 2, 300, 300, nullptr, 0, 10, v, p, 10, nullptr, 0), "no candidates: no workspace");
    expect(!queryTopkArgumentsRefusal(nullptr, 0, 300, 300, r, 200, 10, v, p, 10, nullptr, 0), "no queries: a no-op");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 0, v, p, 10, w, least), "k must"), "k == 0");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 65, v, p, 65, w, ~size_t(0)), "k must"), "k > 64");
    expect(refusedWith(queryTopkArgumentsRefusal(nullptr, 2, 300, 300, r, 200, 10, v, p, 10, w, least), "queries"), "null queries");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, nullptr, 200, 10, v, p, 10, w, least), "rows"), "null rows");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, nullptr, p, 10, w, least), "null"), "null values");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, nullptr, 10, w, least), "null"), "null positions");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, p, 9, w, least), "ld_out"), "ld_out < k");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 299, 300, r, 200, 10, v, p, 10, w, least), "ld_queries"), "ld_queries < dim");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, p, 10, nullptr, least), "workspace"), "null workspace");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, p, 10, w, least - 1), "workspace"), "workspace one byte short");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, p, 10, w, 0), "workspace"), "no workspace at all");
    expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, (1ull << 36) + 1, 10, v, p, 10, w, ~size_t(0)), "too large"), "n > 2^36");
    expect(refusedWith(queryTopkArgumentsRefusal(q, (1 << 16) + 1, 300, 300, r, 200, 10, v, p, 10, w, ~size_t(0)), "too large"), "n_queries > 2^16");
    char* raw = reinterpret_cast<char*>(positions.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, reinterpret_cast<int64_t*>(raw + shift), 10, w, least), "aligned"), "positions", shift);
        expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, v, p, 10, raw + shift, least), "aligned"), "workspace", shift);
        if (shift % 4) {
            expect(refusedWith(queryTopkArgumentsRefusal(reinterpret_cast<const float*>(raw + shift), 2, 300, 300, r, 200, 10, v, p, 10, w, least), "aligned"), "queries", shift);
            expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, reinterpret_cast<const uint32_t*>(raw + shift), 200, 10, v, p, 10, w, least), "aligned"), "rows", shift);
            expect(refusedWith(queryTopkArgumentsRefusal(q, 2, 300, 300, r, 200, 10, reinterpret_cast<float*>(raw + shift), p, 10, w, least), "aligned"), "values", shift);
        }
    }
}

// memb_hip_query_topk_algorithmic_bytes as the header states it, by hand: the matrix count without any matrix -- per
// candidate its id (4) and its compressed bytes, once; 4 * dim per query -- plus 12 * k per query.
void countedBytes()
{
    const uint64_t dim = 300;
    const uint64_t candidates = 28 + 775;   // seven ids and their compressed bytes (query_matrix_planning_main.cpp)
    const uint64_t withoutMatrix = queryMatrixBytes(candidates, 7, 5, dim, false, false, false);
    expect(withoutMatrix == 803 + 5 * 1200, "no matrix counted");
    expect(queryTopkBytes(withoutMatrix, 5, 10) == 803 + 5 * 1200 + 5 * 120, "bytes by hand");
    expect(queryTopkBytes(withoutMatrix, 5, 64) == 803 + 5 * 1200 + 5 * 768, "k = 64");
    expect(queryTopkBytes(queryMatrixBytes(0, 0, 3, dim, false, false, false), 3, 1) == 3 * 1200 + 36, "no candidates");
    expect(queryTopkBytes(0, 1ull << 16, 64) == (1ull << 16) * 768, "no overflow");
}

}  // namespace

int main()
{
    segments();
    workspaces();
    denseRefusals();
    fusedRefusals();
    countedBytes();
    if (failures) {
        std::printf("query topk planning: %d failures\n", failures);
        return 1;
    }
    std::printf("query topk planning: ok\n");
    return 0;
}
