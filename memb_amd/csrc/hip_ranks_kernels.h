// Device code of memb_hip_ranks.hip: the predicate "this candidate precedes the row's mark", a block's count of a run of
// columns, and the wavefront that folds a row's partial counts. Included inside the unit's anonymous namespace, behind
// hip_query_topk_kernels.h (topkKey: the order both the selection and these counts go by; topkReadLane).
#pragma once

using memb_ranks::RankParams;

// The columns of this launch that precede the mark among EQUAL keys are those below the result: mark - base cut to
// 0 .. n. (base >= 0, so mark - base cannot overflow once mark > base.)
__device__ __forceinline__ uint32_t rankTieLimit(long long mark, long long base, uint32_t n)
{
    if (mark <= base) {
        return 0;
    }
    const long long relative = mark - base;
    return relative < static_cast<long long>(n) ? static_cast<uint32_t>(relative) : n;
}

// The contract's predicate on the bits of a value, integer operations only. (| and &, not || and &&: nothing here is worth
// a branch, and a branch around a value would pull its load in behind it.)
__device__ __forceinline__ bool rankPrecedes(uint32_t bits, uint32_t column, uint32_t markKey, uint32_t tieLimit)
{
    const uint32_t key = topkKey(bits);
    return (key > markKey) | ((key == markKey) & (column < tieLimit));
}

// rank_count: the block's row and its run of BLOCK_RUN columns. A block lies inside one row, so the row's threshold and
// mark are scalar loads and every condition on them is wave-uniform; neighbouring lanes read neighbouring columns, thread
// t the columns first + t, first + t + 256, ... The COLUMNS_PER_THREAD loads are issued without a branch between them: a
// column behind the row's last reads the last again and is not counted. One ballot and one population count per load, the
// four wavefronts' sums through LDS, ONE store of the block's partial count. The list of non-candidates is rank_fold's.
__device__ __forceinline__ void rankCountOfBlock(const RankParams& p, uint32_t* waveCounts)
{
    const uint32_t row = blockIdx.x / p.blocksPerRow;
    const uint32_t first = (blockIdx.x % p.blocksPerRow) * memb_ranks::BLOCK_RUN;   // (< n <= 2^31: first + BLOCK_RUN fits 32 bits)
    if (row >= p.nRows) {   // (block-uniform)
        return;
    }
    const uint32_t markKey = topkKey(__float_as_uint(p.thresholds[row]));
    const uint32_t tieLimit = rankTieLimit(p.marks[row], p.base, p.n);
    // (read as bits: the key is built from them)
    const uint32_t* values = reinterpret_cast<const uint32_t*>(p.matrix) + static_cast<unsigned long long>(row) * p.ld;
    const uint32_t last = p.n - 1;   // (n >= 1 wherever this kernel is launched)
    uint32_t loaded[memb_ranks::COLUMNS_PER_THREAD];
#pragma unroll
    for (uint32_t step = 0; step < memb_ranks::COLUMNS_PER_THREAD; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        loaded[step] = values[column < last ? column : last];
    }
    uint32_t count = 0;   // (wave-uniform: the wavefront's count so far)
#pragma unroll
    for (uint32_t step = 0; step < memb_ranks::COLUMNS_PER_THREAD; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        const bool precedes = (column < p.n) & rankPrecedes(loaded[step], column, markKey, tieLimit);
        count += static_cast<uint32_t>(__popcll(__ballot(precedes)));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        waveCounts[threadIdx.x / WAVE] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t wave = 0; wave < memb_ranks::COUNT_THREADS / WAVE; ++wave) {
            total += waveCounts[wave];
        }
        p.partials[blockIdx.x] = total;
    }
}

// rank_fold: the wavefront's row. Lane e holds entry e of the row's list of non-candidates; where that is a column of this
// launch and the first occurrence of its value in the list, the lane reads the candidate's value and applies the
// predicate: rank_count counted exactly those, and one ballot says how many to take off. Then the lanes add the row's
// partial counts (integers: no order to fix) and lane 0 stores the count, or adds it to what counts holds.
__device__ __forceinline__ void rankFoldOfWave(const RankParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t row = blockIdx.x * memb_ranks::FOLD_WAVES + threadIdx.x / WAVE;
    if (row >= p.nRows) {   // (wave-uniform)
        return;
    }
    long long entry = -1;
    if (lane < p.width) {
        entry = p.excluded[static_cast<unsigned long long>(row) * p.ldExcluded + lane];
    }
    bool repeated = false;
    for (uint32_t other = 0; other < p.width; ++other) {   // (wave-uniform trip count and lane index)
        const long long earlier = topkReadLane(entry, other);
        repeated = repeated || (other < lane && earlier == entry);
    }
    // (base >= 0: entry - base cannot overflow once entry >= base)
    const bool inside = entry >= p.base && entry - p.base < static_cast<long long>(p.n) && !repeated;
    bool counted = false;
    if (inside) {
        const uint32_t column = static_cast<uint32_t>(entry - p.base);
        const uint32_t markKey = topkKey(__float_as_uint(p.thresholds[row]));
        const uint32_t tieLimit = rankTieLimit(p.marks[row], p.base, p.n);
        const uint32_t bits = reinterpret_cast<const uint32_t*>(p.matrix)[static_cast<unsigned long long>(row) * p.ld + column];
        counted = rankPrecedes(bits, column, markKey, tieLimit);
    }
    const uint32_t removed = static_cast<uint32_t>(__popcll(__ballot(counted)));
    uint32_t sum = 0;   // (a row's count is at most n <= 2^31)
    const uint32_t* partials = p.partials + static_cast<unsigned long long>(row) * p.blocksPerRow;
    for (uint32_t block = lane; block < p.blocksPerRow; block += WAVE) {
        sum += partials[block];
    }
#pragma unroll
    for (int stride = WAVE / 2; stride > 0; stride >>= 1) {
        sum += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum), stride));
    }
    if (lane == 0) {
        const long long count = static_cast<long long>(sum - removed);
        p.counts[row] = p.accumulate ? p.counts[row] + count : count;
    }
}
