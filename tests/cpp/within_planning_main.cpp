// hip_within_launch.h's first part as a program of its own, for the host sanitizers (-fsanitize=address,undefined): every
// refusal of the two calls, what they accept, and how the workspace is cut into starts, totals and cosines and the
// candidates into slices. No GPU, no HIP runtime: MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_within.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"
#include "../../memb_amd/csrc/hip_analogies_launch.h"
#include "../../memb_amd/csrc/hip_ranks_launch.h"
#include "../../memb_amd/csrc/hip_within_launch.h"

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

// The arguments of a good dense call; a test changes one of them.
struct Dense {
    int device = 0;
    const float* matrix;
    size_t nRows = 2, n = 7, ld = 9;
    int64_t base = 0;
    const float* thresholds;
    const int64_t* marks;
    const int64_t* excluded;
    size_t width = 4, ldExcluded = 4;
    const int64_t* offsets;
    const int64_t* cursors;
    const int64_t* positions;
    const float* values;
    size_t capacity = 20;
    const void* workspace;
    size_t workspaceBytes = 24;

    const char* refusal() const
    {
        return denseWithinArgumentsRefusal(
            device, matrix, nRows, n, ld, base, thresholds, marks, excluded, width, ldExcluded, offsets, cursors, positions, values,
            capacity, workspace, workspaceBytes);
    }
};

void dense()
{
    static_assert(memb_ranks::BLOCK_RUN == 2048 && memb_within::MAX_CAPACITY == (1ull << 62), "the values below");
    std::vector<float> matrix(2 * 9 + 1), thresholds(3), values(21);
    std::vector<int64_t> marks(3), list(2 * 4 + 1), offsets(4), cursors(3), positions(21), space(16);
    Dense good;
    good.matrix = matrix.data();
    good.thresholds = thresholds.data();
    good.marks = marks.data();
    good.excluded = list.data();
    good.offsets = offsets.data();
    good.cursors = cursors.data();
    good.positions = positions.data();
    good.values = values.data();
    good.workspace = space.data();
    expect(!good.refusal(), "a good call");
    Dense call = good;
    call.values = nullptr;
    expect(!call.refusal(), "no values");
    call = good;
    call.matrix += 1, call.ld = 7, call.base = 5, call.thresholds += 1, call.marks += 1, call.excluded = nullptr, call.width = call.ldExcluded = 0;
    call.offsets += 1, call.cursors += 1, call.positions += 1, call.values += 1;
    expect(!call.refusal(), "aligned to 4 bytes only, ld == n, no list");
    call = good;
    call.matrix = nullptr, call.n = call.ld = 0, call.workspace = nullptr, call.workspaceBytes = 0;
    expect(!call.refusal(), "no column: neither a matrix nor a workspace");
    call = good;
    call.nRows = 0, call.workspace = nullptr, call.workspaceBytes = 0;
    expect(!call.refusal(), "no row: no workspace");
    call = good;
    call.nRows = 1ull << 16, call.n = call.ld = 1ull << 31, call.workspaceBytes = ~size_t(0), call.capacity = 1ull << 62;
    expect(!call.refusal(), "the largest sizes");
    call = good, call.device = -1;
    expect(refusedWith(call.refusal(), "device"), "a negative device");
    call = good, call.base = -1;
    expect(refusedWith(call.refusal(), "base"), "a negative base");
    call = good, call.matrix = nullptr;
    expect(refusedWith(call.refusal(), "matrix"), "null matrix with n > 0");
    call = good, call.ld = 6;
    expect(refusedWith(call.refusal(), "at least n"), "ld < n");
    call = good, call.thresholds = nullptr;
    expect(refusedWith(call.refusal(), "null"), "null thresholds");
    call = good, call.marks = nullptr;
    expect(refusedWith(call.refusal(), "null"), "null marks");
    call = good, call.offsets = nullptr;
    expect(refusedWith(call.refusal(), "null"), "null offsets");
    call = good, call.cursors = nullptr;
    expect(refusedWith(call.refusal(), "null"), "null cursors");
    call = good, call.positions = nullptr;
    expect(refusedWith(call.refusal(), "null"), "null positions");
    call = good, call.width = call.ldExcluded = 65;
    expect(refusedWith(call.refusal(), "at most 64"), "width 65");
    call = good, call.ldExcluded = 3;
    expect(refusedWith(call.refusal(), "ld_excluded"), "ld_excluded < width");
    call = good, call.excluded = nullptr;
    expect(refusedWith(call.refusal(), "null"), "a null list");
    call = good, call.nRows = (1ull << 16) + 1, call.workspaceBytes = ~size_t(0);
    expect(refusedWith(call.refusal(), "too large"), "n_rows > 2^16");
    call = good, call.n = (1ull << 31) + 1, call.ld = 1ull << 32, call.workspaceBytes = ~size_t(0);
    expect(refusedWith(call.refusal(), "too large"), "n > 2^31");
    call = good, call.capacity = (1ull << 62) + 1;
    expect(refusedWith(call.refusal(), "capacity"), "capacity > 2^62");
    call = good, call.workspace = nullptr;
    expect(refusedWith(call.refusal(), "workspace"), "a null workspace");
    call = good, call.workspaceBytes = 23;
    expect(refusedWith(call.refusal(), "workspace too small"), "one byte less");
    const char* raw = reinterpret_cast<const char*>(space.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        const int64_t* odd = reinterpret_cast<const int64_t*>(raw + shift);
        call = good, call.marks = odd;
        expect(refusedWith(call.refusal(), "aligned"), "marks", shift);
        call = good, call.excluded = odd;
        expect(refusedWith(call.refusal(), "aligned"), "excluded", shift);
        call = good, call.offsets = odd;
        expect(refusedWith(call.refusal(), "aligned"), "offsets", shift);
        call = good, call.cursors = odd;
        expect(refusedWith(call.refusal(), "aligned"), "cursors", shift);
        call = good, call.positions = odd;
        expect(refusedWith(call.refusal(), "aligned"), "positions", shift);
        call = good, call.workspace = raw + shift;
        expect(refusedWith(call.refusal(), "aligned"), "workspace", shift);
    }
    for (int shift = 1; shift < 4; ++shift) {
        const float* odd = reinterpret_cast<const float*>(raw + shift);
        call = good, call.matrix = odd;
        expect(refusedWith(call.refusal(), "aligned"), "matrix", shift);
        call = good, call.thresholds = odd;
        expect(refusedWith(call.refusal(), "aligned"), "thresholds", shift);
        call = good, call.values = odd;
        expect(refusedWith(call.refusal(), "aligned"), "values", shift);
    }
    // an int64 start and a 32-bit total per block of 2048 columns, the totals rounded up to 8 bytes behind the starts
    expect(denseWithinWorkspaceBytes(2, 7) == 24 && denseWithinWorkspaceBytes(3, 2049) == 72 && denseWithinWorkspaceBytes(1, 2048) == 16, "12 bytes per block");
    expect(withinStartsBytes(3, 2049) == 48 && withinStartsBytes(1, 1ull << 31) == 8ull << 20, "the totals lie behind the starts");
    expect(denseWithinWorkspaceBytes(5, 0) == 0 && denseWithinWorkspaceBytes(0, 5) == 0, "nothing to list");
    expect(denseWithinWorkspaceBytes((1 << 16) + 1, 7) == 0 && denseWithinWorkspaceBytes(2, (1ull << 31) + 1) == 0, "sizes refused");
}

void workspace()
{
    expect(queryWithinWorkspaceBytes(1, 2196017, false) == withinBlockBytes(1, 2196017) + 4ull * 2196017, "one query: the model fits one slice");
    expect(queryWithinWorkspaceBytes(16, 2196017, false) == withinBlockBytes(16, 524288) + 4ull * 16 * 524288, "16 queries: slices of 32 MiB");
    expect(queryWithinWorkspaceBytes(16, 2196017, true) == 192 + 4ull * 16 * 64, "minimal: slices of 64, one block per query");
    expect(queryWithinWorkspaceBytes(3, 50, true) == 40 + 4ull * 3 * 50, "fewer candidates than a slice");
    expect(queryWithinWorkspaceBytes(0, 1000, false) == 0 && queryWithinWorkspaceBytes(3, 0, false) == 0, "nothing to do");
    expect(queryWithinWorkspaceBytes((1 << 16) + 1, 1000, false) == 0 && queryWithinWorkspaceBytes(3, (1ull << 36) + 1, false) == 0, "sizes refused");
    const uint64_t queries[] = {1, 2, 3, 16, 17, 64, 4096, 1 << 16};
    const uint64_t sizes[] = {1, 63, 64, 65, 200, 2047, 2048, 2049, 50000, 2196017, 1ull << 36};
    for (uint64_t q : queries) {
        for (uint64_t n : sizes) {
            const uint64_t least = queryWithinWorkspaceBytes(q, n, true), good = queryWithinWorkspaceBytes(q, n, false);
            expect(planWithinSlice(q, n, least) == std::min<uint64_t>(n, MIN_SLICE), "the minimal workspace: 64 candidates", q, n);
            expect(planWithinSlice(q, n, least - 1) == 0, "one byte less is refused", q, n);
            // (what this call accepts, the count pass in front of it accepts too)
            expect(planRanksSlice(q, n, least) >= std::min<uint64_t>(n, MIN_SLICE), "the count pass runs in the same workspace", q, n);
            const uint64_t slice = planWithinSlice(q, n, good);
            expect(slice == std::min(n, topkRecommendedSlice(q)), "the recommended slice", q, n);
            // the three areas lie inside the workspace: starts, totals, then the cosines, aligned to 8 bytes
            expect(withinBlockBytes(q, slice) % 8 == 0 && withinBlockBytes(q, slice) + 4 * q * slice <= good, "starts, totals and cosines fit", q, n);
            expect(withinStartsBytes(q, slice) + 4 * q * rankBlocksPerRow(slice) <= withinBlockBytes(q, slice), "a start and a total per block", q, n);
            // a shorter last slice needs no more than a whole one
            expect(withinBlockBytes(q, slice - slice / 3) <= withinBlockBytes(q, slice), "the last slice fits the areas of a whole one", q, n);
            expect(slice <= MAX_SLICE && slice <= memb_ranks::MAX_COLUMNS, "a slice's columns fit 32 bits", q, n);
            // anything between the two sizes: a multiple of 64 that fits, and 64 more would not
            const uint64_t between = least + (good - least) / 3;
            const uint64_t middle = planWithinSlice(q, n, between);
            expect(middle >= std::min<uint64_t>(n, MIN_SLICE) && middle <= slice && (middle == n || middle % MIN_SLICE == 0), "a slice in between", q, n);
            expect(withinSliceBytes(q, middle) <= between && (middle == n || middle == MAX_SLICE || withinSliceBytes(q, std::min(n, middle + MIN_SLICE)) > between),
                   "the largest multiple that fits", q, n);
        }
    }
    expect(planWithinSlice(3, 1100, ~uint64_t(0)) == 1100, "any larger workspace: one slice");
    expect(planWithinSlice(3, 1ull << 36, ~uint64_t(0)) == MAX_SLICE, "never wider than MAX_SLICE");
    expect((1100 + planWithinSlice(3, 1100, queryWithinWorkspaceBytes(3, 1100, true)) - 1) / 64 == 18, "eighteen slices of 64");
}

void fused()
{
    std::vector<float> queries(2 * 300 + 1), thresholds(3), values(21);
    std::vector<uint32_t> rows(50);
    std::vector<int64_t> marks(3), list(2 * 4 + 1), offsets(4), cursors(3), positions(21), space(1 << 12);
    const float* v = queries.data();
    const uint32_t* r = rows.data();
    const float* t = thresholds.data();
    const int64_t* p = marks.data();
    const int64_t* e = list.data();
    const int64_t* o = offsets.data();
    const int64_t* c = cursors.data();
    const int64_t* d = positions.data();
    const float* x = values.data();
    const void* w = space.data();
    const size_t bytes = space.size() * 8;
    expect(bytes >= queryWithinWorkspaceBytes(2, 50, false), "the workspace of the good call");
    expect(!queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "a good call");
    expect(!queryWithinArgumentsRefusal(v, 2, 301, 300, r, 50, t, p, nullptr, 0, 0, o, c, d, nullptr, 20, w, bytes), "no list, no values, strided");
    expect(!queryWithinArgumentsRefusal(v, 2, 300, 300, nullptr, 0, t, p, e, 4, 4, o, c, d, x, 0, nullptr, 0), "no candidate: no workspace");
    expect(refusedWith(queryWithinArgumentsRefusal(nullptr, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "queries"), "null queries");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, nullptr, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "rows"), "null rows");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 299, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "ld_queries"), "ld_queries < dim");
    expect(refusedWith(queryWithinArgumentsRefusal(v, (1 << 16) + 1, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "too large"), "n_queries > 2^16");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, (1ull << 36) + 1, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "too large"), "n > 2^36");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, nullptr, p, e, 4, 4, o, c, d, x, 20, w, bytes), "null"), "null thresholds");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, nullptr, e, 4, 4, o, c, d, x, 20, w, bytes), "null"), "null marks");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, nullptr, c, d, x, 20, w, bytes), "null"), "null offsets");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, nullptr, d, x, 20, w, bytes), "null"), "null cursors");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, nullptr, x, 20, w, bytes), "null"), "null positions");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, (1ull << 62) + 1, w, bytes), "capacity"), "capacity > 2^62");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 65, 65, o, c, d, x, 20, w, bytes), "at most 64"), "width 65");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 3, o, c, d, x, 20, w, bytes), "ld_excluded"), "ld_excluded < width");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, nullptr, 4, 4, o, c, d, x, 20, w, bytes), "null"), "a null list");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, nullptr, bytes), "workspace"), "a null workspace");
    const uint64_t least = queryWithinWorkspaceBytes(2, 50, true);
    expect(!queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, least), "the minimal workspace");
    expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, least - 1), "workspace too small"), "one byte less");
    const char* raw = reinterpret_cast<const char*>(space.data());
    for (int shift = 1; shift < 8; ++shift) {   // (never dereferenced)
        const int64_t* odd = reinterpret_cast<const int64_t*>(raw + shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, raw + shift, bytes - 8), "aligned"), "workspace", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, odd, e, 4, 4, o, c, d, x, 20, w, bytes), "aligned"), "marks", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, odd, 4, 4, o, c, d, x, 20, w, bytes), "aligned"), "excluded", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, odd, c, d, x, 20, w, bytes), "aligned"), "offsets", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, odd, d, x, 20, w, bytes), "aligned"), "cursors", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, odd, x, 20, w, bytes), "aligned"), "positions", shift);
    }
    for (int shift = 1; shift < 4; ++shift) {
        const float* odd = reinterpret_cast<const float*>(raw + shift);
        expect(refusedWith(queryWithinArgumentsRefusal(odd, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, x, 20, w, bytes), "aligned"), "queries", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, odd, p, e, 4, 4, o, c, d, x, 20, w, bytes), "aligned"), "thresholds", shift);
        expect(refusedWith(queryWithinArgumentsRefusal(v, 2, 300, 300, r, 50, t, p, e, 4, 4, o, c, d, odd, 20, w, bytes), "aligned"), "values", shift);
    }
}

}  // namespace

int main()
{
    dense();
    workspace();
    fused();
    if (failures) {
        std::printf("within planning: %d failures\n", failures);
        return 1;
    }
    std::printf("within planning: ok\n");
    return 0;
}
