// Pooled lookups under the chunked order (include/memb_hip_pooled_chunked.h), gfx950 / CDNA4: what happens before and
// after the partial sums.
//
// A translation unit of its own, linked into libmemb_hip.so; memb_hip.hip lays out the caller's workspace and launches these
// kernels through the addresses below (hip_pooled_chunked.h). The partial sums themselves -- one per chunk of
// MEMB_HIP_POOL_CHUNK entries -- are MEMB_HIP_POOL_SUM of the sequential kernels (memb_hip_pooled.hip, plain or known)
// over the derived offsets that the plan writes; those kernels are not touched.
//   chunk_block_sums / chunk_scan_sums / chunk_bag_starts
//       the exclusive scan of the bags' chunk counts max(1, ceil(L / C)), in three passes: sums per block of bags, the scan
//       of those sums by ONE block, the scan inside each block on top of its sum. No block reads what a block of the same
//       launch writes and none spins on a flag: the passes are ordered by the stream. Sums are 64-bit (offsets that
//       decrease can make them exceed the workspace's bound); what is stored is min(start, maxChunks), so everything
//       downstream indexes inside the workspace whatever the offsets hold.
//   chunk_offsets
//       chunk k of the workspace -> its bag (binary search of bagStart) -> derived[k] = begin + C (k - bagStart[bag]); the
//       tail up to maxChunks, and derived[maxChunks], is min(offsets[bags], n), the end of the last bag: its last chunk
//       ends there, and the slots behind it are empty bags for the kernels of stage (b).
//   pool_chunks<OUT>
//       one wavefront per bag and 64 columns, a lane per column: the bag's partial sums added in chunk order by single
//       v_add_f32 (the packed forms flush subnormals on gfx950), POOL_CHUNK_BATCH loads in flight before they are added;
//       chunks without a known entry are left out by a wave-uniform branch; one __fdiv_rn for the mean; a bf16 / fp16
//       element is narrowed once at its store. Plain vector stores, no atomics, no value crosses lanes, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_pooled_chunked.h"
#include "hip_pooled_chunked.h"

namespace {

constexpr int WAVE = 64;

#include "hip_device_common.h"

using memb_pooled::ChunkPlanParams;
using memb_pooled::ChunkSumParams;
using memb_pooled::PLAN_BAGS_PER_BLOCK;
using memb_pooled::PLAN_BAGS_PER_THREAD;
using memb_pooled::PLAN_THREADS;
using memb_pooled::POOL_CHUNK;

constexpr int POOL_CHUNK_BATCH = 8;   // partial sums a lane loads before it adds them one after the other

// The chunks of bag `bag`: max(1, ceil(L / C)) for its L entries, clamped to the batch as bagRange clamps them; a bag
// whose offsets decrease is empty.
__device__ __forceinline__ unsigned long long chunksOfBag(const ChunkPlanParams& p, unsigned long long bag)
{
    const unsigned long long begin = min(static_cast<unsigned long long>(p.offsets[bag]), p.n);
    const unsigned long long end = min(static_cast<unsigned long long>(p.offsets[bag + 1]), p.n);
    const unsigned long long length = end > begin ? end - begin : 0;
    return length ? (length + POOL_CHUNK - 1) / POOL_CHUNK : 1;
}

// The chunks of the thread's PLAN_BAGS_PER_THREAD consecutive bags (0 for a bag behind the last).
__device__ __forceinline__ unsigned long long chunksOfThread(
    const ChunkPlanParams& p, unsigned long long firstBag, unsigned long long (&chunks)[PLAN_BAGS_PER_THREAD])
{
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t u = 0; u < PLAN_BAGS_PER_THREAD; ++u) {
        chunks[u] = firstBag + u < p.bags ? chunksOfBag(p, firstBag + u) : 0;
        sum += chunks[u];
    }
    return sum;
}

// The inclusive scan of `value` over the block's PLAN_THREADS threads (Hillis-Steele in LDS); every thread calls it.
__device__ __forceinline__ unsigned long long blockInclusiveScan(unsigned long long value, unsigned long long* lds)
{
    const uint32_t t = threadIdx.x;
    lds[t] = value;
    __syncthreads();
#pragma unroll
    for (uint32_t step = 1; step < PLAN_THREADS; step *= 2) {
        const unsigned long long below = t >= step ? lds[t - step] : 0;
        __syncthreads();
        lds[t] += below;
        __syncthreads();
    }
    return lds[t];
}

__global__ __launch_bounds__(PLAN_THREADS) void chunk_block_sums(ChunkPlanParams p)
{
    __shared__ unsigned long long lds[PLAN_THREADS];
    unsigned long long chunks[PLAN_BAGS_PER_THREAD];
    const unsigned long long firstBag =
        static_cast<unsigned long long>(blockIdx.x) * PLAN_BAGS_PER_BLOCK + threadIdx.x * PLAN_BAGS_PER_THREAD;
    const unsigned long long sum = blockInclusiveScan(chunksOfThread(p, firstBag, chunks), lds);
    if (threadIdx.x == PLAN_THREADS - 1) {
        p.blockSums[blockIdx.x] = sum;
    }
}

// ONE block: blockSums[0 .. planBlocks) -> their exclusive scan, PLAN_THREADS of them at a time with a carry.
__global__ __launch_bounds__(PLAN_THREADS) void chunk_scan_sums(ChunkPlanParams p)
{
    __shared__ unsigned long long lds[PLAN_THREADS];
    unsigned long long carry = 0;
    for (unsigned long long first = 0; first < p.planBlocks; first += PLAN_THREADS) {
        const unsigned long long at = first + threadIdx.x;
        const unsigned long long own = at < p.planBlocks ? p.blockSums[at] : 0;
        const unsigned long long inclusive = blockInclusiveScan(own, lds);
        if (at < p.planBlocks) {
            p.blockSums[at] = carry + inclusive - own;
        }
        carry += lds[PLAN_THREADS - 1];
        __syncthreads();   // (the next round writes lds)
    }
}

__global__ __launch_bounds__(PLAN_THREADS) void chunk_bag_starts(ChunkPlanParams p)
{
    __shared__ unsigned long long lds[PLAN_THREADS];
    unsigned long long chunks[PLAN_BAGS_PER_THREAD];
    const unsigned long long firstBag =
        static_cast<unsigned long long>(blockIdx.x) * PLAN_BAGS_PER_BLOCK + threadIdx.x * PLAN_BAGS_PER_THREAD;
    const unsigned long long own = chunksOfThread(p, firstBag, chunks);
    unsigned long long start = blockInclusiveScan(own, lds) - own;
    if (p.planBlocks > 1) {
        start += p.blockSums[blockIdx.x];
    }
#pragma unroll
    for (uint32_t u = 0; u < PLAN_BAGS_PER_THREAD; ++u) {
        if (firstBag + u < p.bags) {
            p.bagStart[firstBag + u] = static_cast<uint32_t>(min(start, p.maxChunks));
            start += chunks[u];
            if (firstBag + u + 1 == p.bags) {
                p.bagStart[p.bags] = static_cast<uint32_t>(min(start, p.maxChunks));
            }
        }
    }
}

__global__ __launch_bounds__(PLAN_THREADS) void chunk_offsets(ChunkPlanParams p)
{
    const unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * PLAN_THREADS + threadIdx.x;
    if (k > p.maxChunks) {
        return;
    }
    // the bags whose chunks end at or before k: bagStart ascends, so they are the first `low` of them
    unsigned long long low = 0, high = p.bags;
    while (low < high) {
        const unsigned long long middle = low + (high - low) / 2;
        if (p.bagStart[middle + 1] <= k) {
            low = middle + 1;
        } else {
            high = middle;
        }
    }
    // behind the last chunk: empty bags where the last bag ends, which is also where its last chunk has to end
    unsigned long long value = min(static_cast<unsigned long long>(p.offsets[p.bags]), p.n);
    if (low < p.bags) {   // bagStart[low] <= k < bagStart[low + 1]: chunk k - bagStart[low] of bag `low`, which has that many
        const unsigned long long begin = min(static_cast<unsigned long long>(p.offsets[low]), p.n);
        value = begin + static_cast<unsigned long long>(POOL_CHUNK) * (k - p.bagStart[low]);
    }
    p.derived[k] = static_cast<uint32_t>(value);
}

template <int OUT>
__global__ __launch_bounds__(PLAN_THREADS) void pool_chunks(ChunkSumParams p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t columnBlocks = (p.dim + WAVE - 1) / WAVE;
    const unsigned long long wave =
        static_cast<unsigned long long>(blockIdx.x) * (PLAN_THREADS / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const unsigned long long bag = wave / columnBlocks;
    if (bag >= p.bags) {
        return;
    }
    const uint32_t c0 = static_cast<uint32_t>(wave % columnBlocks) * WAVE;
    const uint32_t c = min(c0 + lane, p.dim - 1);
    // (both at most maxChunks: the partial sums read lie inside the workspace whatever the offsets hold)
    const unsigned long long first = p.bagStart[bag];
    const unsigned long long last = p.bagStart[bag + 1];
    const float* partial = p.partials + c;
    float r = 0.f;
    uint32_t count = 0;
    if (p.chunkCounts) {
        for (unsigned long long k = first; k < last; k += POOL_CHUNK_BATCH) {
            uint32_t known[POOL_CHUNK_BATCH];
            float v[POOL_CHUNK_BATCH];
#pragma unroll
            for (int u = 0; u < POOL_CHUNK_BATCH; ++u) {
                const unsigned long long at = min(k + u, last - 1);
                known[u] = p.chunkCounts[at];
                v[u] = partial[at * p.dim];
            }
#pragma unroll
            for (int u = 0; u < POOL_CHUNK_BATCH; ++u) {
                if (k + u < last && known[u]) {   // wave-uniform
                    r = count ? addRn(r, v[u]) : v[u];
                    count += known[u];
                }
            }
        }
        if (p.mean && count) {
            r = __fdiv_rn(r, static_cast<float>(count));
        }
        if (p.counts && c0 == 0 && lane == 0) {
            p.counts[bag] = count;
        }
    } else {
        if (first < last) {
            r = partial[first * p.dim];
        }
        for (unsigned long long k = first + 1; k < last; k += POOL_CHUNK_BATCH) {
            float v[POOL_CHUNK_BATCH];
#pragma unroll
            for (int u = 0; u < POOL_CHUNK_BATCH; ++u) {
                v[u] = partial[min(k + u, last - 1) * p.dim];
            }
#pragma unroll
            for (int u = 0; u < POOL_CHUNK_BATCH; ++u) {
                if (k + u < last) {   // wave-uniform
                    r = addRn(r, v[u]);
                }
            }
        }
        const unsigned long long begin = min(static_cast<unsigned long long>(p.offsets[bag]), p.n);
        const unsigned long long end = min(static_cast<unsigned long long>(p.offsets[bag + 1]), p.n);
        if (p.mean && end > begin) {
            r = __fdiv_rn(r, static_cast<float>(static_cast<uint32_t>(end - begin)));
        }
    }
    if (c0 + lane < p.dim) {
        const unsigned long long at = bag * p.ld + p.colOff + c0 + lane;   // (ld, colOff: in elements)
        if constexpr (OUT == MEMB_HIP_OUT_F32) {
            static_cast<float*>(p.out)[at] = r;
        } else {
            static_cast<uint16_t*>(p.out)[at] = static_cast<uint16_t>(narrowBits<OUT>(r));
        }
    }
}

}  // namespace

namespace memb_pooled {

const void* chunkBlockSumsKernel()
{
    return reinterpret_cast<const void*>(&chunk_block_sums);
}

const void* chunkScanSumsKernel()
{
    return reinterpret_cast<const void*>(&chunk_scan_sums);
}

const void* chunkBagStartsKernel()
{
    return reinterpret_cast<const void*>(&chunk_bag_starts);
}

const void* chunkOffsetsKernel()
{
    return reinterpret_cast<const void*>(&chunk_offsets);
}

const void* poolChunksKernel(int outType)
{
    switch (outType) {
        case MEMB_HIP_OUT_F32:
            return reinterpret_cast<const void*>(&pool_chunks<MEMB_HIP_OUT_F32>);
        case MEMB_HIP_OUT_BF16:
            return reinterpret_cast<const void*>(&pool_chunks<MEMB_HIP_OUT_BF16>);
        case MEMB_HIP_OUT_F16:
            return reinterpret_cast<const void*>(&pool_chunks<MEMB_HIP_OUT_F16>);
        default:
            return nullptr;
    }
}

}  // namespace memb_pooled
