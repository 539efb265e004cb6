// Device code of the query kernel (memb_hip_queries.hip): the group an entry lies in, and the walk of a wavefront over its
// run of candidate entries of a trained model with the current group's query in registers. Included inside the unit's
// anonymous namespace, behind hip_pooled_kernels.h (decodePoolTile, gatherPiece), hip_norms_kernels.h (densePiece) and
// hip_pairs_kernels.h, whose pieceSums, addSums, butterflies and pairOfSums are used as they are.
#pragma once

using memb_queries::QueryParams;

// offsets[g] as the kernel reads it: g clamped to [0, groups], the value clamped to the batch (bagRange's clamping).
__device__ __forceinline__ unsigned long long groupOffset(const QueryParams& qp, unsigned long long g, unsigned long long n)
{
    return min(static_cast<unsigned long long>(qp.offsets[min(g, static_cast<unsigned long long>(qp.groups))]), n);
}

// The group whose query entry i is scored against, where the offsets ascend: the last g with offsets[g] <= i, 0 where
// there is none and groups - 1 at most. A wave-uniform binary search for the first j in [0, groups] with offsets[j] > i;
// every index it reads lies in [0, groups] whatever the offsets hold.
__device__ __forceinline__ uint32_t groupOfEntry(const QueryParams& qp, unsigned long long i, unsigned long long n)
{
    unsigned long long low = 0;
    unsigned long long high = static_cast<unsigned long long>(qp.groups) + 1;   // the answer lies in [low, high]
#pragma nounroll
    while (low < high) {
        const unsigned long long middle = low + (high - low) / 2;   // < high <= groups + 1
        if (groupOffset(qp, middle, n) > i) {
            high = middle;
        } else {
            low = middle + 1;
        }
    }
    const unsigned long long g = low ? low - 1 : 0;
    return static_cast<uint32_t>(min(g, static_cast<unsigned long long>(qp.groups - 1)));
}

// pairsOfWave's walk split by ENTRIES, with x a query that stays in registers: a wavefront owns the entries [first, last)
// of the n candidates, finds the group of `first`, decodes its run tile by tile up to the symbol tile (decodePoolTile, full
// tiles: no pair straddles anything here) and, word by word, steps to the next group where the walk has passed the end of
// the current one, loads that group's query pieces l and l + 64 (densePiece) when the first of its entries turns up,
// gathers the word's two pieces, multiplies, reduces the three partials side by side and finishes the pair (query,
// candidate row). Lane w keeps word w's cosine, dot and norm; a tile's results leave as at most three stores, masked to
// the entries that lie in a group. No row is stored.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ void queriesOfWave(const TrainedParams& p, const QueryParams& qp, uint32_t* lds)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long first = (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * qp.entriesPerWave;
    if (first >= p.n) {
        return;
    }
    const unsigned long long last = min(first + qp.entriesPerWave, p.n);
    const uint32_t pieces = p.dim / 4;   // 1 .. 128
    const bool aligned = qp.ldQueries % 4 == 0 && reinterpret_cast<uintptr_t>(qp.queries) % 16 == 0;   // wave-uniform
    uint32_t group = groupOfEntry(qp, first, p.n);   // < groups
    unsigned long long begin = groupOffset(qp, group, p.n);
    unsigned long long end = groupOffset(qp, group + 1ull, p.n);
    bool loaded = false;   // query0 / query1 hold the pieces of `group`
    float4 query0 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 query1 = make_float4(0.f, 0.f, 0.f, 0.f);
    PoolTile tile;

#pragma nounroll
    for (unsigned long long start = first; start < last; start += p.wordsPerWave) {
        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, start, last, tile);
        const uint32_t words = static_cast<uint32_t>(tile.end - tile.start);
        unsigned long long scored = 0;   // bit w: word w lies in a group
        float cosine = 0.f;
        float dot = 0.f;
        float norm = 0.f;
#pragma nounroll
        for (uint32_t w = 0; w < words; ++w) {
            const unsigned long long i = tile.start + w;
            // (group only grows: at most `groups` steps per wavefront whatever the offsets hold)
            while (i >= end && group + 1 < qp.groups) {
                ++group;
                begin = groupOffset(qp, group, p.n);
                end = groupOffset(qp, group + 1ull, p.n);
                loaded = false;
            }
            if (i < begin || i >= end) {   // wave-uniform: before offsets[0], from offsets[groups] on
                continue;
            }
            if (!loaded) {
                const float* row = qp.queries + group * qp.ldQueries;
                uint32_t l = lane;
                asm volatile("" : "+v"(l));   // (the query's addresses are worked out here, once per group, not kept live)
                query0 = densePiece(row, p.dim, min(l, pieces - 1), aligned);
                if (pieces > WAVE) {
                    query1 = densePiece(row, p.dim, min(l + WAVE, pieces - 1), aligned);
                }
                loaded = true;
            }
            PairSums sums = pieceSums(query0, gatherPiece<FAST>(p, mem, tile, w, min(lane, pieces - 1)));
            if (lane >= pieces) {
                sums = PairSums{0.f, 0.f, 0.f};
            }
            if (pieces > WAVE) {   // wave-uniform
                const PairSums both =
                    addSums(sums, pieceSums(query1, gatherPiece<FAST>(p, mem, tile, w, min(lane + WAVE, pieces - 1))));
                // (selected, not added to +0.0: a lane without a second piece keeps the bits of a -0.0 product)
                if (lane + WAVE < pieces) {
                    sums = both;
                }
            }
            const PairResult r = pairOfSums(butterflies(sums, lane));
            cosine = lane == w ? r.cosine : cosine;
            dot = lane == w ? r.dot : dot;
            norm = lane == w ? r.nb : norm;
            scored |= 1ull << w;
        }
        const bool mine = lane < words && ((scored >> lane) & 1);
        if (qp.cosines && mine) {
            qp.cosines[tile.start + lane] = cosine;
        }
        if (qp.dots && mine) {
            qp.dots[tile.start + lane] = dot;
        }
        if (qp.norms && mine) {
            qp.norms[tile.start + lane] = norm;
        }
    }
}
