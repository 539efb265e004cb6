// Device code of the selection kernels (memb_hip_query_topk.hip): the order of include/memb_hip_query_topk.h as a 32-bit
// key, a wavefront's sorted list of its best 64 entries with one rank per lane, and the insertion both kernels share.
// Included inside the unit's anonymous namespace.
#pragma once

using memb_query_topk::TopkParams;

constexpr uint32_t TOPK_EMPTY_KEY = 0;   // below the key of every value: an empty slot loses against a real -inf

// The contract's order on values as an unsigned key, greater first: every NaN the one greatest key, -0.0 the key of
// +0.0, -inf the smallest, which is 0x007FFFFF. No value has key 0.
__device__ __forceinline__ uint32_t topkKey(uint32_t bits)
{
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) {
        return 0xFFFFFFFFu;
    }
    if (bits == 0x80000000u) {
        bits = 0;
    }
    return bits & 0x80000000u ? ~bits : bits | 0x80000000u;
}

// (key, position) a comes before b: the greater key, the lower position among equal keys
template <typename Position>
__device__ __forceinline__ bool topkBefore(uint32_t keyA, Position positionA, uint32_t keyB, Position positionB)
{
    return keyA > keyB || (keyA == keyB && positionA < positionB);
}

__device__ __forceinline__ uint32_t topkReadLane(uint32_t value, uint32_t lane)
{
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(value), static_cast<int>(lane)));
}

__device__ __forceinline__ long long topkReadLane(long long value, uint32_t lane)
{
    const unsigned long long bits = static_cast<unsigned long long>(value);
    const unsigned long long low = topkReadLane(static_cast<uint32_t>(bits), lane);
    const unsigned long long high = topkReadLane(static_cast<uint32_t>(bits >> 32), lane);
    return static_cast<long long>(high << 32 | low);
}

__device__ __forceinline__ uint32_t topkFromBelow(uint32_t value)
{
    return static_cast<uint32_t>(__shfl_up(static_cast<int>(value), 1));
}

__device__ __forceinline__ long long topkFromBelow(long long value)
{
    const unsigned long long bits = static_cast<unsigned long long>(value);
    const unsigned long long low = topkFromBelow(static_cast<uint32_t>(bits));
    const unsigned long long high = topkFromBelow(static_cast<uint32_t>(bits >> 32));
    return static_cast<long long>(high << 32 | low);
}

// The wavefront's best 64 entries so far in the contract's order, lane r holding rank r. Only the first k ranks are ever
// stored, and rank k - 1 is the threshold a new entry has to come before.
template <typename Position>
struct TopkList {
    uint32_t key = TOPK_EMPTY_KEY;
    uint32_t bits = 0xFF800000u;   // -inf
    Position position = 0;
};

// Up to 64 entries, one per lane (`valid`: the lane holds one), offered to the list: ONE ballot against rank k - 1, then
// each survivor in lane order, tested again against the threshold it may have raised, broadcast, and inserted by a shift
// of one lane from its rank on. Every branch is wave-uniform.
template <typename Position>
__device__ __forceinline__ void topkOffer(
    TopkList<Position>& list, uint32_t k, uint32_t lane, bool valid, uint32_t key, uint32_t bits, Position position)
{
    uint32_t lastKey = topkReadLane(list.key, k - 1);
    Position lastPosition = topkReadLane(list.position, k - 1);
    unsigned long long survivors = __ballot(valid && topkBefore(key, position, lastKey, lastPosition));
    while (survivors) {
        const uint32_t source = static_cast<uint32_t>(__ffsll(survivors)) - 1;
        survivors &= survivors - 1;
        const uint32_t newKey = topkReadLane(key, source);
        const Position newPosition = topkReadLane(position, source);
        if (!topkBefore(newKey, newPosition, lastKey, lastPosition)) {
            continue;
        }
        const uint32_t newBits = topkReadLane(bits, source);
        const bool stays = topkBefore(list.key, list.position, newKey, newPosition);
        const uint32_t belowKey = topkFromBelow(list.key);
        const uint32_t belowBits = topkFromBelow(list.bits);
        const Position belowPosition = topkFromBelow(list.position);
        // (every lane takes part in the exchange: a lane that sat it out would be read as 0 by the lane above)
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

// topk_select: the wavefront's (row, segment), its columns 64 at a time, UNROLL batches loaded before the first is tested;
// the list goes to the workspace, EMPTY_COLUMN in the ranks the segment did not fill.
__device__ __forceinline__ void topkSelectOfWave(const TopkParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wave =
        static_cast<unsigned long long>(blockIdx.x) * memb_query_topk::WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (wave >= static_cast<unsigned long long>(p.nRows) * p.segments) {   // (wave-uniform)
        return;
    }
    const uint32_t row = static_cast<uint32_t>(wave / p.segments);
    const uint32_t segment = static_cast<uint32_t>(wave % p.segments);
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
            topkOffer(list, p.k, lane, column < end, topkKey(loaded[batch]), loaded[batch], column);
        }
    }
    if (lane < p.k) {
        const unsigned long long slot = wave * p.k + lane;
        p.listValues[slot] = list.bits;
        p.listColumns[slot] = list.key == TOPK_EMPTY_KEY ? memb_query_topk::EMPTY_COLUMN : list.position;
    }
}

// topk_merge: the wavefront's row. With `merge` the k entries the output holds (position -1: empty) are offered first,
// then the row's segment lists 64 entries at a time, their columns as base + column. Ranks the candidates did not fill
// are stored as -inf and -1.
__device__ __forceinline__ void topkMergeOfWave(const TopkParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t row = blockIdx.x * memb_query_topk::WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= p.nRows) {   // (wave-uniform)
        return;
    }
    uint32_t* values = reinterpret_cast<uint32_t*>(p.values) + static_cast<unsigned long long>(row) * p.ldOut;
    long long* positions = p.positions + static_cast<unsigned long long>(row) * p.ldOut;
    TopkList<long long> list;
    if (p.merge) {
        const bool inside = lane < p.k;
        const long long held = inside ? positions[lane] : -1;
        const uint32_t bits = inside ? values[lane] : 0;
        topkOffer(list, p.k, lane, held >= 0, topkKey(bits), bits, held);
    }
    const uint32_t entries = p.segments * p.k;   // (<= 256 * 64)
    const unsigned long long firstSlot = static_cast<unsigned long long>(row) * entries;
    for (uint32_t start = 0; start < entries; start += memb_query_topk::BATCH) {
        const uint32_t entry = start + lane;
        const uint32_t column = entry < entries ? p.listColumns[firstSlot + entry] : memb_query_topk::EMPTY_COLUMN;
        const uint32_t bits = entry < entries ? p.listValues[firstSlot + entry] : 0;
        topkOffer(list, p.k, lane, column != memb_query_topk::EMPTY_COLUMN, topkKey(bits), bits,
                  p.base + static_cast<long long>(column));
    }
    if (lane < p.k) {
        const bool empty = list.key == TOPK_EMPTY_KEY;
        values[lane] = empty ? 0xFF800000u : list.bits;
        positions[lane] = empty ? -1 : list.position;
    }
}
