// Device code of memb_hip_within.hip: a block's run of columns with the row's non-candidates inside it, the count of the
// run's listed columns, the wavefront that turns a row's counts into the blocks' first destinations, and the ordered
// compaction of a run. Included inside the unit's anonymous namespace, behind hip_query_topk_kernels.h (topkKey,
// topkReadLane) and hip_ranks_kernels.h (rankPrecedes, rankTieLimit: the predicate, shared and not restated).
#pragma once

using memb_within::WithinParams;

constexpr uint32_t WITHIN_STEPS = memb_ranks::COLUMNS_PER_THREAD;
constexpr uint32_t WITHIN_WAVES = memb_ranks::COUNT_THREADS / WAVE;
constexpr uint32_t WITHIN_PARTS = WITHIN_STEPS * WITHIN_WAVES;   // the (step, wavefront) parts of a run, in column order

static_assert(WITHIN_PARTS <= uint32_t(WAVE) && (WITHIN_PARTS & (WITHIN_PARTS - 1)) == 0, "one lane per part in the scan of within_write");
static_assert(memb_analogies::MAX_EXCLUDED <= uint32_t(WAVE), "one lane per entry of a row's list");

// The row's non-candidates inside a block's run, kept in LDS.
struct WithinNamed {
    uint32_t columns[memb_analogies::MAX_EXCLUDED];   // counted from the run's first column
    uint32_t count;
};

// The block's run: thread t loads the columns first + t, first + t + 256, ... back to back with no branch between them; a
// column behind the row's last reads the last again and is never listed. (first < n <= 2^31: first + BLOCK_RUN fits 32
// bits.)
__device__ __forceinline__ void withinLoadRun(const WithinParams& p, uint32_t row, uint32_t first, uint32_t (&loaded)[WITHIN_STEPS])
{
    // (read as bits: the key is built from them, and within_write stores them as they are)
    const uint32_t* values = reinterpret_cast<const uint32_t*>(p.matrix) + static_cast<unsigned long long>(row) * p.ld;
    const uint32_t last = p.n - 1;   // (n >= 1 wherever these kernels are launched)
#pragma unroll
    for (uint32_t step = 0; step < WITHIN_STEPS; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        loaded[step] = values[column < last ? column : last];
    }
}

// The row's non-candidates among THIS THREAD's columns, as a mask over its load steps. Lane e of the first wavefront
// holds entry e of the row's list; a ballot packs the entries inside the block's run into LDS as columns. Behind the
// barrier every thread walks the packed entries -- block-uniform, and none for nearly every block -- and marks the step
// whose column one names. Repeats mark the same bit again: a column is named or it is not. (width is the launch's: with
// none the barrier is left out for every block alike.)
__device__ __forceinline__ uint32_t withinNamedSteps(const WithinParams& p, uint32_t row, uint32_t first, WithinNamed* named)
{
    if (p.width == 0) {
        return 0;
    }
    if (threadIdx.x < WAVE) {   // (wave-uniform)
        const uint32_t lane = threadIdx.x;
        long long entry = -1;
        if (lane < p.width) {
            entry = p.excluded[static_cast<unsigned long long>(row) * p.ldExcluded + lane];
        }
        const uint32_t end = first + memb_ranks::BLOCK_RUN < p.n ? first + memb_ranks::BLOCK_RUN : p.n;
        // (unsigned: the difference of any two int64 is defined, and it is looked at only where entry >= base >= 0)
        const unsigned long long relative = static_cast<unsigned long long>(entry) - static_cast<unsigned long long>(p.base);
        const bool inside = entry >= p.base && relative >= first && relative < end;
        const unsigned long long ballot = __ballot(inside);
        if (inside) {
            named->columns[__popcll(ballot & ((1ull << lane) - 1))] = static_cast<uint32_t>(relative) - first;
        }
        if (lane == 0) {
            named->count = static_cast<uint32_t>(__popcll(ballot));
        }
    }
    __syncthreads();
    const uint32_t count = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(named->count)));
    uint32_t steps = 0;
    for (uint32_t entry = 0; entry < count; ++entry) {
        const uint32_t inRun = named->columns[entry];   // (below BLOCK_RUN: step * COUNT_THREADS + thread)
        if (inRun % memb_ranks::COUNT_THREADS == threadIdx.x) {
            steps |= 1u << (inRun / memb_ranks::COUNT_THREADS);
        }
    }
    return steps;
}

// The contract's "is listed" for the column of one load step: inside the row, precedes the mark, and is not named.
__device__ __forceinline__ bool withinListed(
    const WithinParams& p, uint32_t bits, uint32_t column, uint32_t step, uint32_t markKey, uint32_t tieLimit, uint32_t namedSteps)
{
    return (column < p.n) & rankPrecedes(bits, column, markKey, tieLimit) & ((namedSteps >> step & 1u) == 0);
}

// within_count: the block's row and its run of BLOCK_RUN columns, as in the rank unit's count -- a block lies inside one
// row, so the row's threshold and mark are scalar loads -- but with the row's non-candidates taken out here, since the
// total decides where the next block writes. One ballot and one population count per load, the four wavefronts' sums
// through LDS, ONE store of the block's total.
__device__ __forceinline__ void withinCountOfBlock(const WithinParams& p, WithinNamed* named, uint32_t* waveCounts)
{
    const uint32_t row = blockIdx.x / p.blocksPerRow;
    const uint32_t first = (blockIdx.x % p.blocksPerRow) * memb_ranks::BLOCK_RUN;
    if (row >= p.nRows) {   // (block-uniform)
        return;
    }
    const uint32_t markKey = topkKey(__float_as_uint(p.thresholds[row]));
    const uint32_t tieLimit = rankTieLimit(p.marks[row], p.base, p.n);
    uint32_t loaded[WITHIN_STEPS];
    withinLoadRun(p, row, first, loaded);
    const uint32_t namedSteps = withinNamedSteps(p, row, first, named);
    uint32_t count = 0;   // (wave-uniform: the wavefront's count so far)
#pragma unroll
    for (uint32_t step = 0; step < WITHIN_STEPS; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        count += static_cast<uint32_t>(__popcll(__ballot(withinListed(p, loaded[step], column, step, markKey, tieLimit, namedSteps))));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        waveCounts[threadIdx.x / WAVE] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t wave = 0; wave < WITHIN_WAVES; ++wave) {
            total += waveCounts[wave];
        }
        p.totals[blockIdx.x] = total;
    }
}

// The inclusive scan of one value per lane over groups of `group` lanes (a power of two, at most the wavefront).
__device__ __forceinline__ uint32_t withinScan(uint32_t value, uint32_t lane, uint32_t group)
{
#pragma unroll
    for (uint32_t delta = 1; delta < group; delta <<= 1) {
        const uint32_t lower = static_cast<uint32_t>(__shfl_up(static_cast<int>(value), delta));
        if ((lane & (group - 1)) >= delta) {
            value += lower;
        }
    }
    return value;
}

// within_starts: the wavefront's row. The row's block totals 64 at a time: an exclusive scan across the lanes plus what
// the blocks before them found is each block's first destination, counted from where the row goes on -- offsets[q], or
// offsets[q] + cursors[q] under accumulate. Then lane 0 stores the cursor. With no column at all there is no block, and the
// cursor is all this kernel writes.
__device__ __forceinline__ void withinStartsOfWave(const WithinParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t row = blockIdx.x * memb_within::STARTS_WAVES + threadIdx.x / WAVE;
    if (row >= p.nRows) {   // (wave-uniform)
        return;
    }
    const long long held = p.accumulate ? p.cursors[row] : 0;
    const long long origin = p.offsets[row] + held;
    const uint32_t* totals = p.totals + static_cast<unsigned long long>(row) * p.blocksPerRow;
    long long* starts = p.starts + static_cast<unsigned long long>(row) * p.blocksPerRow;
    long long found = 0;   // (wave-uniform: what the blocks before these 64 found; a row finds at most n <= 2^31)
    for (uint32_t firstBlock = 0; firstBlock < p.blocksPerRow; firstBlock += WAVE) {   // (wave-uniform trip count)
        const uint32_t block = firstBlock + lane;
        const uint32_t total = block < p.blocksPerRow ? totals[block] : 0;
        const uint32_t inclusive = withinScan(total, lane, WAVE);   // (at most 64 * BLOCK_RUN)
        if (block < p.blocksPerRow) {
            starts[block] = origin + found + static_cast<long long>(inclusive - total);
        }
        found += static_cast<long long>(topkReadLane(inclusive, WAVE - 1));
    }
    if (lane == 0) {
        p.cursors[row] = held + found;
    }
}

// within_write: within_count's block again -- the same loads, the same predicate, so the same columns -- and now every
// listed column's place: the eight load steps by four wavefronts are 32 parts of the run in ascending column order, a
// ballot per part gives the part's count (to LDS) and the lane's place inside it (the listed lanes below it); behind the
// barrier every wavefront scans the 32 counts for itself, and the destination is the block's start + the parts before +
// the lanes below. The position and, where asked for, the value's bits are stored only inside the row's segment and the
// buffers, whatever the offsets and the cursors hold.
__device__ __forceinline__ void withinWriteOfBlock(const WithinParams& p, WithinNamed* named, uint32_t* partCounts)
{
    const uint32_t row = blockIdx.x / p.blocksPerRow;
    const uint32_t first = (blockIdx.x % p.blocksPerRow) * memb_ranks::BLOCK_RUN;
    if (row >= p.nRows) {   // (block-uniform)
        return;
    }
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x / WAVE)));
    const uint32_t markKey = topkKey(__float_as_uint(p.thresholds[row]));
    const uint32_t tieLimit = rankTieLimit(p.marks[row], p.base, p.n);
    uint32_t loaded[WITHIN_STEPS];
    withinLoadRun(p, row, first, loaded);
    const uint32_t namedSteps = withinNamedSteps(p, row, first, named);
    const unsigned long long lanesBelow = (1ull << lane) - 1;
    uint32_t place[WITHIN_STEPS];   // the listed lanes below this one in its part
    uint32_t listedSteps = 0;       // bit `step`: this thread's column of that step is listed
#pragma unroll
    for (uint32_t step = 0; step < WITHIN_STEPS; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        const bool listed = withinListed(p, loaded[step], column, step, markKey, tieLimit, namedSteps);
        const unsigned long long ballot = __ballot(listed);
        place[step] = static_cast<uint32_t>(__popcll(ballot & lanesBelow));
        listedSteps |= static_cast<uint32_t>(listed) << step;
        if (lane == 0) {
            partCounts[step * WITHIN_WAVES + wave] = static_cast<uint32_t>(__popcll(ballot));
        }
    }
    __syncthreads();
    // (the upper half of the wavefront scans a second copy: no lane sits out a shuffle)
    const uint32_t partCount = partCounts[lane & (WITHIN_PARTS - 1)];
    const uint32_t partsBefore = withinScan(partCount, lane, WITHIN_PARTS) - partCount;
    const long long start = p.starts[blockIdx.x];
    const long long segment = p.offsets[row], segmentEnd = p.offsets[row + 1];
    const long long lowest = segment > 0 ? segment : 0;
    const long long limit = segmentEnd < p.capacity ? segmentEnd : p.capacity;
#pragma unroll
    for (uint32_t step = 0; step < WITHIN_STEPS; ++step) {
        const uint32_t column = first + step * memb_ranks::COUNT_THREADS + threadIdx.x;
        const long long destination =
            start + static_cast<long long>(topkReadLane(partsBefore, step * WITHIN_WAVES + wave)) + static_cast<long long>(place[step]);
        if ((listedSteps >> step & 1u) != 0 && destination >= lowest && destination < limit) {
            p.positions[destination] = p.base + static_cast<long long>(column);
            if (p.values) {
                reinterpret_cast<uint32_t*>(p.values)[destination] = loaded[step];
            }
        }
    }
}
