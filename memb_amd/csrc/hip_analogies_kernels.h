// Device code of memb_hip_analogies.hip: topk_select's body with the row's exclusion list in one register, and the sum of
// weighted rows. Included inside the unit's anonymous namespace, behind hip_query_topk_kernels.h (topkKey, TopkList,
// topkBefore, topkReadLane, topkFromBelow).
#pragma once

using memb_analogies::ExcludedList;
using memb_analogies::WeightedSumParams;

// topkOffer with one more test of a survivor: lane e holds the excluded column e of this launch (EMPTY_COLUMN: none), and
// a broadcast survivor that any lane holds is skipped like one the raised threshold turns away. The batch's one ballot
// stays as it is, so the cost is a compare per survivor, never per column. Every branch is wave-uniform.
__device__ __forceinline__ void topkOfferExcluding(
    TopkList<uint32_t>& list, uint32_t k, uint32_t lane, bool valid, uint32_t key, uint32_t bits, uint32_t position,
    uint32_t heldColumn)
{
    uint32_t lastKey = topkReadLane(list.key, k - 1);
    uint32_t lastPosition = topkReadLane(list.position, k - 1);
    unsigned long long survivors = __ballot(valid && topkBefore(key, position, lastKey, lastPosition));
    while (survivors) {
        const uint32_t source = static_cast<uint32_t>(__ffsll(survivors)) - 1;
        survivors &= survivors - 1;
        const uint32_t newKey = topkReadLane(key, source);
        const uint32_t newPosition = topkReadLane(position, source);
        if (!topkBefore(newKey, newPosition, lastKey, lastPosition)) {
            continue;
        }
        if (__ballot(heldColumn == newPosition)) {   // (a column is never EMPTY_COLUMN: n <= 2^31)
            continue;
        }
        // (the insertion of topkOffer, word for word: that header stays as it is, so that topk_select keeps its instructions)
        const uint32_t newBits = topkReadLane(bits, source);
        const bool stays = topkBefore(list.key, list.position, newKey, newPosition);
        const uint32_t belowKey = topkFromBelow(list.key);
        const uint32_t belowBits = topkFromBelow(list.bits);
        const uint32_t belowPosition = topkFromBelow(list.position);
        const uint32_t belowOutcome = topkFromBelow(static_cast<uint32_t>(stays));
        const bool belowStays = lane == 0 || belowOutcome != 0;
        if (!stays) {
            list.key = belowStays ? newKey : belowKey;
            list.bits = belowStays ? newBits : belowBits;
            list.position = belowStays ? newPosition : belowPosition;
        }
        lastKey = topkReadLane(list.key, k - 1);
        lastPosition = topkReadLane(list.position, k - 1);
    }
}

// topk_select_excluding: topkSelectOfWave with the row's list loaded once, entry e into lane e as a column of this launch
// -- excluded - base where that lies in [0, n), so a negative entry, padding and a position of another slice hold
// EMPTY_COLUMN. The list the wavefront writes holds no excluded column.
__device__ __forceinline__ void topkSelectExcludingOfWave(const TopkParams& p, const ExcludedList& e)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wave =
        static_cast<unsigned long long>(blockIdx.x) * memb_query_topk::WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (wave >= static_cast<unsigned long long>(p.nRows) * p.segments) {   // (wave-uniform)
        return;
    }
    const uint32_t row = static_cast<uint32_t>(wave / p.segments);
    const uint32_t segment = static_cast<uint32_t>(wave % p.segments);
    uint32_t heldColumn = memb_query_topk::EMPTY_COLUMN;
    if (lane < e.width) {
        const long long entry = e.excluded[static_cast<unsigned long long>(row) * e.ld + lane];
        // (base >= 0: entry - base cannot overflow once entry >= base)
        if (entry >= p.base && entry - p.base < static_cast<long long>(p.n)) {
            heldColumn = static_cast<uint32_t>(entry - p.base);
        }
    }
    // (read and written as bits: a NaN keeps its payload)
    const uint32_t* values = reinterpret_cast<const uint32_t*>(p.matrix) + static_cast<unsigned long long>(row) * p.ld;
    const uint32_t first = segment * p.segmentLength;   // (< n <= 2^31)
    const uint32_t end = p.n - first < p.segmentLength ? p.n : first + p.segmentLength;
    TopkList<uint32_t> list;
    for (uint32_t start = first; start < end; start += memb_query_topk::BATCH * memb_query_topk::UNROLL) {
        uint32_t loaded[memb_query_topk::UNROLL];
#pragma unroll
        for (uint32_t batch = 0; batch < memb_query_topk::UNROLL; ++batch) {
            const uint32_t column = start + batch * memb_query_topk::BATCH + lane;
            loaded[batch] = column < end ? values[column] : 0;
        }
#pragma unroll
        for (uint32_t batch = 0; batch < memb_query_topk::UNROLL; ++batch) {
            const uint32_t column = start + batch * memb_query_topk::BATCH + lane;
            topkOfferExcluding(list, p.k, lane, column < end, topkKey(loaded[batch]), loaded[batch], column, heldColumn);
        }
    }
    if (lane < p.k) {
        const unsigned long long slot = wave * p.k + lane;
        p.listValues[slot] = list.bits;
        p.listColumns[slot] = list.key == TOPK_EMPTY_KEY ? memb_query_topk::EMPTY_COLUMN : list.position;
    }
}

// weighted_rows_sum: the thread's output element (sum q, column c), its bag's entries in order from +0.0. The product and
// the sum are two separately rounded float32 operations, whatever the compiler's contraction setting. Neighbouring lanes
// read neighbouring columns of the same entry.
__device__ __forceinline__ void weightedSumOfThread(const WeightedSumParams& p)
{
    const unsigned long long element = static_cast<unsigned long long>(blockIdx.x) * memb_analogies::SUM_THREADS + threadIdx.x;
    if (element >= static_cast<unsigned long long>(p.nSums) * p.dim) {
        return;
    }
    const uint32_t sum = static_cast<uint32_t>(element / p.dim);
    const uint32_t column = static_cast<uint32_t>(element % p.dim);
    const uint32_t end = p.offsets[sum + 1];
    float total = 0.0f;
    for (uint32_t entry = p.offsets[sum]; entry < end; ++entry) {
        const float value = p.matrix[static_cast<unsigned long long>(entry) * p.ld + column];
        total = __fadd_rn(total, __fmul_rn(p.weights ? p.weights[entry] : 1.0f, value));
    }
    p.out[static_cast<unsigned long long>(sum) * p.ldOut + column] = total;
}
