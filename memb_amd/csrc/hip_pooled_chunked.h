// The kernels of memb_hip_pooled_chunked.hip (pooled lookups under the chunked order: include/memb_hip_pooled_chunked.h) as
// memb_hip.hip launches them (hip_pooled_launch.h: pool_rows_chunked_checked): host addresses for hipLaunchKernel, their parameters, and the caller's workspace as both
// sides lay it out. Three stages on one stream:
//   (a) the chunk plan    chunk_block_sums -> chunk_scan_sums -> chunk_bag_starts -> chunk_offsets (ChunkPlanParams)
//   (b) partial sums      launchPooled, MEMB_HIP_POOL_SUM over the derived offsets into the workspace: the kernels of
//                         memb_hip_pooled.hip (plain or known) as they are
//   (c) the bags' sums    pool_chunks<OUT> (ChunkSumParams)
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/memb_hip_pooled_chunked.h"

namespace memb_pooled {

constexpr uint32_t POOL_CHUNK = MEMB_HIP_POOL_CHUNK;
static_assert(POOL_CHUNK >= 8 && (POOL_CHUNK & (POOL_CHUNK - 1)) == 0, "a power of two and a multiple of 8");

constexpr uint32_t PLAN_THREADS = 256;                                  // every kernel here: blocks of four wavefronts
constexpr uint32_t PLAN_BAGS_PER_THREAD = 8;                            // consecutive bags a thread of the scan owns
constexpr uint32_t PLAN_BAGS_PER_BLOCK = PLAN_THREADS * PLAN_BAGS_PER_THREAD;

// The workspace: every section starts on 16 bytes. maxChunks = bags + ceil(n / C) bounds the chunks of ascending offsets:
// a bag of L entries has max(1, ceil(L / C)) <= 1 + floor(L / C) of them, and the bags' entries do not overlap.
struct ChunkWorkspace {
    unsigned long long maxChunks;
    unsigned long long planBlocks;   // blocks of the scan over the bags
    size_t bagStart;                 // uint32 [bags + 1]: the bag's first chunk, min(.., maxChunks); [bags]: all chunks
    size_t blockSums;                // uint64 [planBlocks]: chunks of the bags before the block's
    size_t derived;                  // uint32 [maxChunks + 1]: the chunks as bags of the sequential kernels; behind the last
                                     // chunk min(offsets[bags], n), where the last bag ends: empty bags
    size_t chunkCounts;              // uint32 [maxChunks]: known entries per chunk (skip_missing)
    size_t partials;                 // float [maxChunks, dim]
    size_t bytes;
};

inline ChunkWorkspace chunkWorkspace(size_t n, size_t bags, uint32_t dim)
{
    const auto aligned = [](size_t bytes) { return (bytes + 15) & ~size_t(15); };
    ChunkWorkspace w{};
    w.maxChunks = static_cast<unsigned long long>(bags) + (static_cast<unsigned long long>(n) + POOL_CHUNK - 1) / POOL_CHUNK;
    w.planBlocks = (static_cast<unsigned long long>(bags) + PLAN_BAGS_PER_BLOCK - 1) / PLAN_BAGS_PER_BLOCK;
    w.bagStart = 0;
    w.blockSums = w.bagStart + aligned(4 * (bags + 1));
    w.derived = w.blockSums + aligned(8 * w.planBlocks);
    w.chunkCounts = w.derived + aligned(4 * (w.maxChunks + 1));
    w.partials = w.chunkCounts + aligned(4 * w.maxChunks);
    w.bytes = w.partials + aligned(4 * w.maxChunks * dim);
    return w;
}

struct ChunkPlanParams {
    const uint32_t* offsets;          // [bags + 1], the caller's
    unsigned long long bags;
    unsigned long long n;
    unsigned long long maxChunks;
    unsigned long long planBlocks;
    unsigned long long* blockSums;
    uint32_t* bagStart;
    uint32_t* derived;
};

struct ChunkSumParams {
    const uint32_t* offsets;          // [bags + 1], the caller's
    const uint32_t* bagStart;
    const float* partials;            // [maxChunks, dim]
    const uint32_t* chunkCounts;      // null: every chunk counts (an unknown entry is a row of +0.0)
    void* out;                        // bag b: columns [colOff, colOff + dim) of out + b * ld, in elements of OUT
    uint32_t* counts;                 // [bags] or null
    unsigned long long bags;
    unsigned long long n;
    unsigned long long ld;
    unsigned long long colOff;
    uint32_t dim;
    uint32_t mean;
};

// chunk_block_sums / chunk_scan_sums / chunk_bag_starts / chunk_offsets (ChunkPlanParams), blocks of PLAN_THREADS:
//   chunk_block_sums   planBlocks blocks: the chunks of the block's PLAN_BAGS_PER_BLOCK bags -> blockSums
//   chunk_scan_sums    ONE block: blockSums -> their exclusive scan, in place (planBlocks > 1 only)
//   chunk_bag_starts   planBlocks blocks: bagStart (planBlocks == 1: blockSums is not read)
//   chunk_offsets      ceil((maxChunks + 1) / PLAN_THREADS) blocks: derived
// No block waits for another: the order is that of the launches on the stream.
const void* chunkBlockSumsKernel();
const void* chunkScanSumsKernel();
const void* chunkBagStartsKernel();
const void* chunkOffsetsKernel();
// pool_chunks<OUT> (ChunkSumParams), OUT a MEMB_HIP_OUT_*; null for an unknown type. One wavefront per bag and 64 columns,
// blocks of PLAN_THREADS.
const void* poolChunksKernel(int outType);

}  // namespace memb_pooled
