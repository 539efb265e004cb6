// hip_query_bags_launch.h's planning and argument checks as a program of its own, for the host sanitizers
// (-fsanitize=address,undefined): the bags a wavefront owns by hand for a handful of (bags, n, Q, W), the top-k workspace
// bytes and the slicing for a minimal and a recommended workspace, every refusal of the two entry points that needs no
// device, and the byte count by hand. No GPU, no HIP runtime: MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind
// a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/memb_hip_query_bags.h"
#include "../../memb_amd/csrc/hip_query_topk.h"
#include "../../memb_amd/csrc/hip_query_bags.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"
#include "../../memb_amd/csrc/hip_query_matrix_launch.h"
#include "../../memb_amd/csrc/hip_query_topk_launch.h"
#include "../../memb_amd/csrc/hip_query_bags_launch.h"

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

// 256 CUs, five wavefronts per SIMD: 5120 wavefronts fill the machine
uint32_t owned(uint64_t bags, uint64_t n, uint64_t queries, uint32_t words, uint32_t tilesSwitch = 0)
{
    return planQueryBagsPerWave(tilesSwitch, words, n, bags, queries, 256, 4 * memb_query_bags::TRAINED_WAVES_PER_SIMD);
}

void plan()
{
    static_assert(memb_query_bags::BAG_GROUP == 2 && memb_query_bags::QUERY_BLOCK == 2, "the values below");
    static_assert(memb_query_bags::TRAINED_WAVES_PER_SIMD == 5 && memb_pooled::POOLED_TILES_PER_WAVE == 4, "the values below");
    // a million sentences of 12 words, 16 words per wavefront: four tiles are 64 entries, five bags; one block of queries
    // keeps the pooled plan's run, more queries share it out, never below a group of two bags
    expect(owned(1000000, 12000000, 1, 16) == 5 && owned(1000000, 12000000, 2, 16) == 5, "one block of queries: the pooled plan's run");
    expect(owned(1000000, 12000000, 3, 16) == 2 && owned(1000000, 12000000, 64, 16) == 2, "more queries: a group of bags");
    // a thousand documents of 2000 words: the pooled plan gives one bag to fill the machine, and it stays one
    expect(owned(1000, 2000000, 1, 16) == 1 && owned(1000, 2000000, 64, 16) == 1, "never below the run that fills the machine");
    // bags of one entry, four words per wavefront: sixteen bags (four tiles; 19 would still fill the machine)
    expect(owned(100000, 100000, 1, 4) == 16 && owned(100000, 100000, 4, 4) == 4 && owned(100000, 100000, 16, 4) == 2, "the run shared out among the queries");
    expect(owned(1, 0, 1, 16) == 1 && owned(1, 0, 64, 16) == 1 && owned(3, 0, 7, 1) == 1, "no entry at all");
    // the option tiles_per_wave = 64: 64 * 16 / 12 = 85 bags, 28 each for three queries
    expect(owned(1000000, 12000000, 1, 16, 64) == 85 && owned(1000000, 12000000, 3, 16, 64) == 28, "tiles_per_wave");
    expect(owned(1ull << 36, 1ull << 37, 1, 64) == 128 && owned(1ull << 36, 0, 1, 64) == 256, "the largest batch");
    for (uint64_t bags : {1ull, 2ull, 3ull, 13ull, 5119ull, 5120ull, 5121ull, 1000000ull, 1ull << 36}) {
        for (uint64_t queries : {1ull, 2ull, 3ull, 16ull, 65536ull}) {
            for (uint32_t words : {1u, 7u, 16u, 64u}) {
                const uint32_t run = owned(bags, 12 * bags, queries, words);
                expect(run >= 1 && run <= (1u << 16), "a run of 1 .. 2^16 whole bags", bags, run);
                expect(run <= owned(bags, 12 * bags, 1, words), "never longer than the pooled plan's", bags, queries);
            }
        }
    }
}

void workspaces()
{
    using namespace memb_query_topk;
    // five queries, 1100 bags, k = 10: the lists of 256 segments per query, then the slice of the matrix
    expect(queryBagsTopkWorkspaceBytes(5, 1100, 10, true) == 5 * 256 * 10 * 8 + 4 * 5 * 64, "minimal: slices of 64 bags");
    expect(queryBagsTopkWorkspaceBytes(5, 1100, 10, false) == 5 * 256 * 10 * 8 + 4 * 5 * 1100, "recommended: every bag where they fit");
    expect(queryBagsTopkWorkspaceBytes(64, 1000000, 64, false) == 64ull * 128 * 64 * 8 + 4ull * 64 * 131072, "recommended: a slice of 32 MiB");
    expect(queryBagsTopkWorkspaceBytes(5, 1100, 0, false) == 0 && queryBagsTopkWorkspaceBytes(5, 1100, 65, false) == 0, "k refused");
    expect(queryBagsTopkWorkspaceBytes(0, 1100, 10, false) == 0 && queryBagsTopkWorkspaceBytes(5, 0, 10, false) == 0, "nothing needed");
    expect(queryBagsTopkWorkspaceBytes(5, (1ull << 36) + 1, 10, false) == 0 && queryBagsTopkWorkspaceBytes(65537, 5, 10, false) == 0, "sizes refused");
    const uint64_t minimal = queryBagsTopkWorkspaceBytes(5, 1100, 10, true);
    const uint64_t slice = planTopkSlice(5, 1100, 10, minimal);
    expect(slice == 64 && (1100 + slice - 1) / slice == 18, "the minimal workspace: eighteen slices of 64 bags", slice);
    expect(planTopkSlice(5, 1100, 10, minimal - 1) == 0, "one byte less: too small");
    expect(planTopkSlice(5, 1100, 10, queryBagsTopkWorkspaceBytes(5, 1100, 10, false)) == 1100, "the recommended workspace: one slice");
    expect(planTopkSlice(64, 1000000, 64, queryBagsTopkWorkspaceBytes(64, 1000000, 64, false)) == 131072, "eight slices of a million bags");
}

void refusals()
{
    alignas(8) static float buffer[64];
    const float* q = buffer;
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(buffer);
    const int sum = MEMB_HIP_POOL_SUM, mean = MEMB_HIP_POOL_MEAN;
    expect(!queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "a plain call");
    expect(!queryBagsArgumentsRefusal(nullptr, 0, 300, 300, nullptr, 0, nullptr, 0, sum, nullptr, nullptr, 0, buffer), "nothing at all, norms asked for");
    expect(!queryBagsArgumentsRefusal(q, 2, 300, 300, nullptr, 0, ids, 3, sum, nullptr, buffer, 3, nullptr), "no entry: empty bags");
    expect(!queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, nullptr, nullptr, 0, buffer), "norms alone: ld_out is not looked at");
    expect(refusedWith(queryBagsArgumentsRefusal(nullptr, 2, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "queries"), "null queries");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, nullptr, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "rows or offsets"), "null rows");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, nullptr, 3, mean, buffer, nullptr, 3, nullptr), "rows or offsets"), "null offsets");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, nullptr, nullptr, 3, nullptr), "at least one"), "three null outputs");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, 2, buffer, nullptr, 3, nullptr), "mode"), "an unknown mode");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 299, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "ld_queries"), "ld_queries < dim");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 2, nullptr), "ld_out"), "ld_out < bags");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, nullptr, buffer, 2, nullptr), "ld_out"), "ld_out < bags, dots");
    const char* odd = reinterpret_cast<const char*>(buffer) + 2;
    expect(refusedWith(queryBagsArgumentsRefusal(reinterpret_cast<const float*>(odd), 2, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "aligned"), "misaligned queries");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, reinterpret_cast<const uint32_t*>(odd), 3, mean, buffer, nullptr, 3, nullptr), "aligned"), "misaligned offsets");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, reinterpret_cast<const float*>(odd)), "aligned"), "misaligned norms");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, (1ull << 36) + 1, mean, nullptr, nullptr, 0, buffer), "too large"), "too many bags");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 2, 300, 300, ids, (1ull << 37) + 1, ids, 3, mean, buffer, nullptr, 3, nullptr), "too large"), "too many entries");
    expect(refusedWith(queryBagsArgumentsRefusal(q, 65537, 300, 300, ids, 9, ids, 3, mean, buffer, nullptr, 3, nullptr), "too large"), "too many queries");

    const int64_t* positions = reinterpret_cast<const int64_t*>(buffer);
    const uint64_t enough = queryBagsTopkWorkspaceBytes(2, 3, 10, true);
    expect(!queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, positions, 10, buffer, enough), "a plain top-k call");
    expect(!queryBagsTopkArgumentsRefusal(q, 2, 300, 300, nullptr, 0, nullptr, 0, mean, 10, buffer, positions, 10, nullptr, 0), "no bag: no workspace needed");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 0, buffer, positions, 10, buffer, enough), "k must"), "k == 0");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 65, buffer, positions, 65, buffer, enough), "k must"), "k > 64");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, nullptr, positions, 10, buffer, enough), "values and positions"), "null values");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, nullptr, 10, buffer, enough), "values and positions"), "null positions");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, positions, 9, buffer, enough), "ld_out"), "ld_out < k");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, 7, 10, buffer, positions, 10, buffer, enough), "mode"), "the matrix call's own refusals");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, reinterpret_cast<const int64_t*>(buffer + 1), 10, buffer, enough), "8 bytes"), "misaligned positions");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, positions, 10, buffer + 1, enough), "8 bytes"), "misaligned workspace");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, positions, 10, buffer, enough - 1), "workspace too small"), "a workspace one byte short");
    expect(refusedWith(queryBagsTopkArgumentsRefusal(q, 2, 300, 300, ids, 9, ids, 3, mean, 10, buffer, positions, 10, nullptr, enough), "workspace too small"), "a null workspace");
}

void bytes()
{
    // 13 bags at dim 300 whose pooled count is 1 000 000: without the 13 * 1200 stored, five queries of 1200 bytes, 5 * 13
    // cosines; with every output 5 * 13 dots and 13 norms more
    expect(queryBagsBytes(1000000, 13, 5, 300, true, false, false) == 1000000 - 15600 + 6000 + 260, "cosines");
    expect(queryBagsBytes(1000000, 13, 5, 300, true, true, true) == 1000000 - 15600 + 6000 + 520 + 52, "every output");
    expect(queryBagsBytes(0, 0, 5, 300, true, true, true) == 6000, "no bag: the queries");
}

}  // namespace

int main()
{
    plan();
    workspaces();
    refusals();
    bytes();
    if (failures) {
        std::printf("query bags planning: %d FAILED\n", failures);
        return 1;
    }
    std::printf("query bags planning: ok\n");
    return 0;
}
