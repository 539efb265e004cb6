// hip_queries_launch.h's planning and argument checks as a program of its own, for the host sanitizers
// (-fsanitize=address,undefined): what memb_hip_query_similarity_device refuses before it looks at the model, how its
// entries are spread over wavefronts and blocks, and the count of the entries that lie in a group. No GPU, no HIP runtime:
// MEMB_HIP_QUERIES_PLANNING_ONLY leaves out everything behind a context.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../memb_amd/csrc/hip_queries.h"

#define MEMB_HIP_QUERIES_PLANNING_ONLY
#include "../../memb_amd/csrc/hip_queries_launch.h"

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
    std::vector<float> queries(2 * 303 + 1), outputs(3 * 10 + 1);
    std::vector<uint32_t> rows(10), offsets(3);
    const float* q = queries.data();
    const uint32_t* r = rows.data();
    const uint32_t* o = offsets.data();
    float* c = outputs.data();
    expect(!queryArgumentsRefusal(q, 2, 303, 300, r, 10, o, c, c + 10, c + 20), "a good call");
    expect(!queryArgumentsRefusal(q, 2, 300, 300, r, 10, o, nullptr, nullptr, c), "norms alone");
    expect(!queryArgumentsRefusal(q + 1, 2, 303, 300, r, 10, o, c + 1, nullptr, nullptr), "aligned to 4 bytes only");
    expect(!queryArgumentsRefusal(nullptr, 0, 300, 300, r, 10, nullptr, c, nullptr, nullptr), "no groups: a no-op");
    expect(!queryArgumentsRefusal(q, 2, 300, 300, nullptr, 0, o, c, nullptr, nullptr), "no entries: a no-op");
    expect(refusedWith(queryArgumentsRefusal(nullptr, 2, 300, 300, r, 10, o, c, nullptr, nullptr), "queries or offsets"), "null queries");
    expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, nullptr, c, nullptr, nullptr), "queries or offsets"), "null offsets");
    expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, nullptr, 10, o, c, nullptr, nullptr), "rows"), "null rows");
    expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, o, nullptr, nullptr, nullptr), "at least one"), "three null outputs");
    expect(refusedWith(queryArgumentsRefusal(q, 2, 299, 300, r, 10, o, c, nullptr, nullptr), "ld_queries"), "ld_queries < dim");
    const char* bytes = reinterpret_cast<const char*>(outputs.data());
    for (int shift = 1; shift < 4; ++shift) {
        float* odd = reinterpret_cast<float*>(const_cast<char*>(bytes) + shift);   // (never dereferenced)
        expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, o, odd, nullptr, nullptr), "aligned"), "cosines", shift);
        expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, o, c, odd, nullptr), "aligned"), "dots", shift);
        expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, o, c, nullptr, odd), "aligned"), "norms", shift);
        expect(refusedWith(queryArgumentsRefusal(reinterpret_cast<const float*>(odd), 2, 300, 300, r, 10, o, c, nullptr, nullptr), "aligned"), "queries", shift);
        expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, reinterpret_cast<const uint32_t*>(odd), 10, o, c, nullptr, nullptr), "aligned"), "rows", shift);
        expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, 10, reinterpret_cast<const uint32_t*>(odd), c, nullptr, nullptr), "aligned"), "offsets", shift);
    }
    expect(!queryArgumentsRefusal(q, 2, 300, 300, r, size_t(1) << 36, o, c, nullptr, nullptr), "n = 2^36");
    expect(refusedWith(queryArgumentsRefusal(q, 2, 300, 300, r, (size_t(1) << 36) + 1, o, c, nullptr, nullptr), "too large"), "n > 2^36");
    expect(!queryArgumentsRefusal(q, 0xFFFFFFFEull, 300, 300, r, 10, o, c, nullptr, nullptr), "groups = 2^32 - 2");
    expect(refusedWith(queryArgumentsRefusal(q, 0xFFFFFFFFull, 300, 300, r, 10, o, c, nullptr, nullptr), "too large"), "groups > 2^32 - 2");
    expect(refusedWith(queryArgumentsRefusal(q, ~size_t(0), ~size_t(0), 300, r, ~size_t(0), o, c, nullptr, nullptr), "too large"), "everything at its maximum");
}

void grids()
{
    const uint64_t sizes[] = {1, 2, 3, 63, 64, 65, 4999, 5000, 50000, 2200000, (1ull << 31) + 7, 1ull << 36};
    const uint32_t words[] = {1, 2, 4, 7, 21, 64};
    const uint32_t switches[] = {0, 1, 5, 64, 0xFFFFFFFFu};
    const uint32_t cus[] = {1, 256, 0xFFFFu};
    const uint32_t waves[] = {0, 1, 4, 8, 16};
    for (uint64_t n : sizes) {
        for (uint32_t w : words) {
            for (uint32_t s : switches) {
                for (uint32_t cu : cus) {
                    for (uint32_t v : waves) {
                        const QueryGrid grid = planQueryGrid(s, w, n, cu, v);
                        expect(grid.entriesPerWave >= 1 && grid.entriesPerWave <= (1u << 16), "entries per wavefront", n, grid.entriesPerWave);
                        if (!grid.blocks) {
                            continue;   // refused: too many blocks for one launch
                        }
                        // every entry is owned by exactly one wavefront of the grid, and the last block is not empty
                        const uint64_t perBlock = uint64_t(v ? v : 1) * grid.entriesPerWave;
                        expect(uint64_t(grid.blocks) * perBlock >= n, "the grid covers the batch", n, grid.blocks);
                        expect(uint64_t(grid.blocks - 1) * perBlock < n, "no empty block", n, grid.blocks);
                        expect(grid.blocks < 0x7FFFFFFFu, "one launch", n, grid.blocks);
                    }
                }
            }
        }
    }
    // The values themselves, on 256 CUs of 28 wavefronts (7 168 wavefronts fill the machine): below 14 336 entries a wavefront
    // owns ONE entry, then n / 7 168 of them, and four tiles of W from n = 4 W * 7 168 on. The GPU tests size their batches
    // by this.
    struct { uint64_t n; uint32_t words; uint32_t owned; } const planned[] = {
        {1, 8, 1}, {5000, 4, 1}, {7167, 8, 1}, {14335, 8, 1}, {14336, 8, 2}, {50000, 8, 6}, {126301, 8, 17}, {111169, 7, 15},
        {229375, 8, 31}, {229376, 8, 32}, {2196017, 8, 32}, {2196017, 4, 16}, {2196017, 1, 4}, {2196017, 64, 256}, {1ull << 36, 64, 256}};
    for (const auto& plan : planned) {
        const QueryGrid grid = planQueryGrid(0, plan.words, plan.n, 256, 4);
        expect(grid.entriesPerWave == plan.owned, "entries per wavefront at 256 CUs", plan.n, grid.entriesPerWave);
        expect(grid.blocks == (plan.n + 4ull * plan.owned - 1) / (4ull * plan.owned), "blocks of four wavefronts", plan.n, grid.blocks);
    }
    // the tiles_per_wave switch replaces the four tiles, and cannot lift a run above what fills the machine
    expect(planQueryGrid(1, 8, 2196017, 256, 4).entriesPerWave == 8, "one tile per wavefront");
    expect(planQueryGrid(64, 8, 2196017, 256, 4).entriesPerWave == 306, "64 tiles asked for, 2 196 017 / 7 168 given");
    expect(planQueryGrid(64, 8, 5000, 256, 4).entriesPerWave == 1, "64 tiles asked for, 5 000 entries");
    // one group of the whole vocabulary spreads over the machine: 5 000 entries are 1 250 blocks of four wavefronts
    const QueryGrid spread = planQueryGrid(0, 4, 5000, 256, 4);
    expect(spread.blocks == 1250 && spread.entriesPerWave == 1, "5 000 entries spread", spread.blocks, spread.entriesPerWave);
}

// memb::gridBlocks (hip_kernel_handle.h), which every launch whose wavefronts own a run of items sizes its grid with:
// ceil(count / (waves * perWave)) blocks, 0 from 0x7FFFFFFF blocks on.
void blockCounts()
{
    expect(memb::gridBlocks(4, 1, 1) == 1, "one item: one block");
    expect(memb::gridBlocks(16, 65536, 1) == 1, "one item under the longest run: one block");
    expect(memb::gridBlocks(4, 6, 24 * 10) == 10, "whole blocks", memb::gridBlocks(4, 6, 24 * 10));
    expect(memb::gridBlocks(4, 6, 24 * 10 + 1) == 11, "one item more: one block more", memb::gridBlocks(4, 6, 24 * 10 + 1));
    expect(memb::gridBlocks(4, 6, 24 * 10 - 1) == 10, "one item fewer: the last block is not full");
    expect(memb::gridBlocks(0, 0, 5) == 5, "0 counts as 1 in either factor");
    // the limit: 0x7FFFFFFE blocks still fit one launch, 0x7FFFFFFF do not
    const uint64_t perBlock = 4 * 3;
    const uint64_t fits = 0x7FFFFFFEull * perBlock;   // the largest count of 0x7FFFFFFE blocks
    expect(memb::gridBlocks(4, 3, fits) == 0x7FFFFFFEu, "the largest count that fits", memb::gridBlocks(4, 3, fits));
    expect(memb::gridBlocks(4, 3, fits + 1) == 0, "the smallest count that does not");
    expect(memb::gridBlocks(1, 1, 0x7FFFFFFEull) == 0x7FFFFFFEu && memb::gridBlocks(1, 1, 0x7FFFFFFFull) == 0, "blocks of one item");
    expect(memb::gridBlocks(4, 1, 1ull << 37) == 0, "far beyond the limit");
    // planQueryGrid sizes its grid with it
    const QueryGrid grid = planQueryGrid(0, 8, 50000, 256, 4);
    expect(grid.blocks == memb::gridBlocks(4, grid.entriesPerWave, 50000) && grid.blocks == 2084, "planQueryGrid's blocks", grid.blocks);
    expect(planQueryGrid(0, 8, 1ull << 36, 1, 1).blocks == 0, "planQueryGrid: too many blocks");
}

void countedEntries()
{
    uint64_t entries = 0, nonEmpty = 0;
    {
        const std::vector<uint32_t> offsets = {2, 2, 5, 5, 5, 9};
        queryGroupEntries(offsets.data(), 5, 12, &entries, &nonEmpty);
        expect(entries == 7 && nonEmpty == 2, "ascending offsets", entries, nonEmpty);
        queryGroupEntries(offsets.data(), 5, 4, &entries, &nonEmpty);   // clamped to n
        expect(entries == 2 && nonEmpty == 1, "offsets beyond n", entries, nonEmpty);
        queryGroupEntries(offsets.data(), 0, 4, &entries, &nonEmpty);
        expect(entries == 0 && nonEmpty == 0, "no groups", entries, nonEmpty);
    }
    {
        const std::vector<uint32_t> offsets = {9, 0xFFFFFFFFu, 0, 7, 3};   // descending: a backwards range is empty
        queryGroupEntries(offsets.data(), 4, 8, &entries, &nonEmpty);
        expect(entries == 7 && nonEmpty == 1, "descending offsets", entries, nonEmpty);
    }
    {
        const std::vector<uint32_t> offsets = {0};   // groups + 1 entries and not one more (an exact allocation)
        queryGroupEntries(offsets.data(), 0, 100, &entries, &nonEmpty);
        expect(entries == 0, "one offset", entries, nonEmpty);
    }
}

// memb_hip_query_algorithmic_bytes as the header states it, by hand: 8 bytes of offsets per group, per entry that lies in a
// group its id (4) and its compressed bytes, 4 * dim for the query of every group that is not empty, 4 bytes per entry in
// a group and output. `pooled` is put together here as memb_hip_pooled_algorithmic_bytes counts it.
void countedBytes()
{
    const uint64_t dim = 300;
    const std::vector<uint32_t> offsets = {2, 2, 5, 5, 5, 9};   // five groups, two of them not empty, seven entries of twelve
    const uint64_t compressed[12] = {0, 0, 150, 0 /* a missing id */, 161, 149, 0, 155, 160, 0, 0, 0};
    uint64_t entries = 0, nonEmpty = 0;
    queryGroupEntries(offsets.data(), 5, 12, &entries, &nonEmpty);
    uint64_t pooled = 5 * (8 + 4 * dim);
    uint64_t byHand = 5 * 8 + nonEmpty * 4 * dim;
    for (uint32_t i = 2; i < 9; ++i) {
        pooled += 4 + compressed[i];
        byHand += 4 + compressed[i];
    }
    for (int outputs = 0; outputs < 8; ++outputs) {
        const bool c = outputs & 1, d = outputs & 2, n = outputs & 4;
        expect(queryBytes(pooled, 5, nonEmpty, entries, dim, c, d, n) == byHand + entries * 4 * (c + d + n), "bytes by hand", outputs);
    }
    expect(queryBytes(0, 0, 0, 0, dim, true, true, true) == 0, "no groups, no bytes");
    expect(queryBytes(3 * (8 + 4 * dim), 3, 0, 0, dim, true, false, false) == 24, "empty groups: their offsets alone");
}

}  // namespace

int main()
{
    argumentChecks();
    grids();
    blockCounts();
    countedEntries();
    countedBytes();
    if (failures) {
        std::printf("queries planning: %d failures\n", failures);
        return 1;
    }
    std::printf("queries planning: ok\n");
    return 0;
}
