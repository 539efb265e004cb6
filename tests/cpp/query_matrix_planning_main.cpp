// hip_query_matrix_launch.h's planning and argument checks as a program of its own, for the host sanitizers
// (-fsanitize=address,undefined): what memb_hip_query_matrix_device refuses before it looks at the model, how its
// candidates are spread over wavefronts and blocks, and the byte count by hand. No GPU, no HIP runtime:
// MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_query_matrix.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"

namespace {

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

void argumentChecks()
{
    std::vector<float> queries(2 * 303 + 1), outputs(2 * 12 * 2 + 10 + 1);
    std::vector<uint32_t> rows(10);
    const float* q = queries.data();
    const uint32_t* r = rows.data();
    float* c = outputs.data();
    float* d = c + 24;
    float* nm = c + 48;
    expect(!queryMatrixArgumentsRefusal(q, 2, 303, 300, r, 10, c, d, 12, nm), "a good call");
    expect(!queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, c, nullptr, 10, nullptr), "cosines alone, ld_out == n");
    expect(!queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, nullptr, nullptr, 0, nm), "norms alone: ld_out is not looked at");
    expect(!queryMatrixArgumentsRefusal(q + 1, 2, 303, 300, r, 10, c + 1, nullptr, 11, nullptr), "aligned to 4 bytes only");
    expect(!queryMatrixArgumentsRefusal(nullptr, 0, 300, 300, r, 10, c, nullptr, 10, nullptr), "no queries: a no-op");
    expect(!queryMatrixArgumentsRefusal(q, 2, 300, 300, nullptr, 0, c, nullptr, 0, nullptr), "no candidates: a no-op");
    expect(refusedWith(queryMatrixArgumentsRefusal(nullptr, 2, 300, 300, r, 10, c, nullptr, 10, nullptr), "queries"), "null queries");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, nullptr, 10, c, nullptr, 10, nullptr), "rows"), "null rows");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, nullptr, nullptr, 10, nullptr), "at least one"), "three null outputs");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 299, 300, r, 10, c, nullptr, 10, nullptr), "ld_queries"), "ld_queries < dim");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, c, nullptr, 9, nullptr), "ld_out"), "ld_out < n, cosines");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, nullptr, d, 9, nullptr), "ld_out"), "ld_out < n, dots");
    const char* bytes = reinterpret_cast<const char*>(outputs.data());
    for (int shift = 1; shift < 4; ++shift) {
        float* odd = reinterpret_cast<float*>(const_cast<char*>(bytes) + shift);   // (never dereferenced)
        expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, odd, nullptr, 10, nullptr), "aligned"), "cosines", shift);
        expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, c, odd, 10, nullptr), "aligned"), "dots", shift);
        expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, 10, c, nullptr, 10, odd), "aligned"), "norms", shift);
        expect(refusedWith(queryMatrixArgumentsRefusal(reinterpret_cast<const float*>(odd), 2, 300, 300, r, 10, c, nullptr, 10, nullptr), "aligned"), "queries", shift);
        expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, reinterpret_cast<const uint32_t*>(odd), 10, c, nullptr, 10, nullptr), "aligned"), "rows", shift);
    }
    const size_t most = size_t(1) << 36;
    expect(!queryMatrixArgumentsRefusal(q, 2, 300, 300, r, most, c, nullptr, most, nullptr), "n = 2^36");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, 2, 300, 300, r, most + 1, c, nullptr, most + 1, nullptr), "too large"), "n > 2^36");
    expect(!queryMatrixArgumentsRefusal(q, size_t(1) << 16, 300, 300, r, 10, c, nullptr, 10, nullptr), "n_queries = 2^16");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, (size_t(1) << 16) + 1, 300, 300, r, 10, c, nullptr, 10, nullptr), "too large"), "n_queries > 2^16");
    expect(refusedWith(queryMatrixArgumentsRefusal(q, ~size_t(0), ~size_t(0), 300, r, ~size_t(0), c, nullptr, ~size_t(0), nullptr), "too large"), "everything at its maximum");
}

void grids()
{
    const uint64_t sizes[] = {1, 2, 3, 63, 64, 65, 4999, 5000, 50000, 2200000, (1ull << 31) + 7, 1ull << 36};
    const uint64_t counts[] = {1, 2, 3, 4, 5, 16, 64, 1ull << 16};
    const uint32_t words[] = {1, 2, 4, 7, 21, 64};
    const uint32_t switches[] = {0, 1, 5, 64, 0xFFFFFFFFu};
    const uint32_t cus[] = {1, 256, 0xFFFFu};
    const uint32_t waves[] = {0, 1, 4, 8, 16};
    const uint64_t block = memb_query_matrix::QUERY_BLOCK;
    for (uint64_t n : sizes) {
        for (uint64_t count : counts) {
            for (uint32_t w : words) {
                for (uint32_t s : switches) {
                    for (uint32_t cu : cus) {
                        for (uint32_t v : waves) {
                            const QueryGrid one = planQueryGrid(s, w, n, cu, v);
                            const QueryGrid grid = planQueryMatrixGrid(s, w, n, count, cu, v);
                            expect(grid.entriesPerWave >= 1 && grid.entriesPerWave <= one.entriesPerWave, "never longer than one query's run", n, grid.entriesPerWave);
                            expect(count > 1 || grid.entriesPerWave == one.entriesPerWave, "one query: planQueryGrid's run", n, grid.entriesPerWave);
                            expect(grid.entriesPerWave >= std::min(w, one.entriesPerWave), "never cut below a tile", n, grid.entriesPerWave);
                            // several tiles only where one block of queries holds them all and one store takes them
                            expect(grid.entriesPerWave <= w || count <= std::min<uint64_t>(block, 64 / w), "several tiles, one block", n, count);
                            if (!grid.blocks) {
                                continue;   // refused: too many blocks for one launch
                            }
                            const uint64_t perBlock = uint64_t(v ? v : 1) * grid.entriesPerWave;
                            expect(uint64_t(grid.blocks) * perBlock >= n, "the grid covers the batch", n, grid.blocks);
                            expect(uint64_t(grid.blocks - 1) * perBlock < n, "no empty block", n, grid.blocks);
                            expect(grid.blocks < 0x7FFFFFFFu, "one launch", n, grid.blocks);
                        }
                    }
                }
            }
        }
    }
    // The values themselves, on 256 CUs of 28 wavefronts (7 168 wavefronts fill the machine), blocks of four wavefronts
    // (DESIGN.md section 5.11): the run of one query shared out among the queries, never below a tile, one tile from three
    // queries on (QUERY_BLOCK is 2). The GPU tests size their batches by this.
    static_assert(memb_query_matrix::QUERY_BLOCK == 2, "the values below are those of blocks of two queries");
    struct { uint64_t n; uint64_t queries; uint32_t words; uint32_t owned; } const planned[] = {
        {5000, 1, 8, 1}, {5000, 64, 8, 1}, {50000, 1, 8, 6}, {50000, 2, 8, 6}, {50000, 64, 8, 6},
        {2196017, 1, 8, 32}, {2196017, 2, 8, 16}, {2196017, 3, 8, 8}, {2196017, 4, 8, 8}, {2196017, 16, 8, 8}, {2196017, 64, 8, 8},
        {129023, 2, 8, 8}, {129024, 2, 8, 9}, {126301, 2, 8, 8}, {2196017, 2, 4, 8}, {2196017, 3, 4, 4}, {100352, 2, 7, 7},
        {114688, 2, 7, 8}, {2196017, 1, 1, 4}, {2196017, 2, 1, 2}, {2196017, 3, 1, 1}, {2196017, 1, 64, 256}, {2196017, 2, 64, 64},
        {2196017, 1 << 16, 8, 8}, {1ull << 36, 2, 64, 64}};
    for (const auto& plan : planned) {
        const QueryGrid grid = planQueryMatrixGrid(0, plan.words, plan.n, plan.queries, 256, 4);
        expect(grid.entriesPerWave == plan.owned, "candidates per wavefront at 256 CUs", plan.n, grid.entriesPerWave);
        expect(grid.blocks == (plan.n + 4ull * plan.owned - 1) / (4ull * plan.owned), "blocks of four wavefronts", plan.n, grid.blocks);
    }
    // the tiles_per_wave switch: 64 tiles asked for, 2 196 017 / 7 168 = 306 candidates given to one query, 153 to each of two
    expect(planQueryMatrixGrid(64, 8, 2196017, 1, 256, 4).entriesPerWave == 306, "64 tiles, one query");
    expect(planQueryMatrixGrid(64, 8, 2196017, 2, 256, 4).entriesPerWave == 153, "64 tiles, two queries");
    expect(planQueryMatrixGrid(64, 8, 2196017, 3, 256, 4).entriesPerWave == 8, "64 tiles, three queries: one tile");
    expect(planQueryMatrixGrid(1, 8, 2196017, 2, 256, 4).entriesPerWave == 8, "one tile per wavefront");
}

// memb_hip_query_matrix_algorithmic_bytes as the header states it, by hand: per candidate its id (4) and its compressed
// bytes, once; 4 * dim per query; 4 bytes per (query, candidate) and matrix; 4 bytes per candidate for the norms.
void countedBytes()
{
    const uint64_t dim = 300;
    const uint64_t compressed[7] = {150, 0 /* a missing id */, 161, 149, 0, 155, 160};
    uint64_t candidates = 0;
    for (uint64_t bytes : compressed) {
        candidates += 4 + bytes;
    }
    expect(candidates == 28 + 775, "the candidates by hand", candidates);
    for (int outputs = 0; outputs < 8; ++outputs) {
        const bool c = outputs & 1, d = outputs & 2, n = outputs & 4;
        expect(queryMatrixBytes(candidates, 7, 5, dim, c, d, n) == 803 + 5 * 1200 + 5 * 7 * 4 * (c + d) + 7 * 4 * n, "bytes by hand", outputs);
    }
    expect(queryMatrixBytes(candidates, 7, 1, dim, true, false, false) == 803 + 1200 + 28, "one query");
    expect(queryMatrixBytes(0, 0, 3, dim, true, true, true) == 3 * 1200, "no candidates: the queries alone");
    expect(queryMatrixBytes(candidates, 7, 0, dim, true, true, true) == 803 + 28, "no queries: the candidates and their norms");
    // the largest call: 2^36 candidates, 2^16 queries, two matrices
    expect(queryMatrixBytes(0, 1ull << 36, 1ull << 16, dim, true, true, false) == (1ull << 16) * 1200 + (1ull << 55), "no overflow");
}

}  // namespace

int main()
{
    argumentChecks();
    grids();
    countedBytes();
    if (failures) {
        std::printf("query matrix planning: %d failures\n", failures);
        return 1;
    }
    std::printf("query matrix planning: ok\n");
    return 0;
}
