// Device code of the query-bags kernel (memb_hip_query_bags.hip): the walk of a wavefront over its run of whole bags of a
// trained model, each pooled in registers and scored against every query. Included inside the unit's anonymous namespace,
// behind hip_pooled_kernels.h (bagRange, decodePoolTile, accumulatePiece, divide4), hip_norms_kernels.h (pieceSquares,
// correctSqrt, unitDivisor, densePiece), hip_pairs_kernels.h (pieceProducts), hip_queries_kernels.h and
// hip_query_matrix_kernels.h (lanePartial, butterfliesOfBlock), which are used as they are.
#pragma once

constexpr uint32_t BAG_GROUP = memb_query_bags::BAG_GROUP;
static_assert(BAG_GROUP % QUERY_BLOCK == 0 && WAVE % BAG_GROUP == 0 && (WAVE / BAG_GROUP) % QUERY_BLOCK == 0,
              "the group's norms are reduced a block at a time, and a block of queries never straddles a store");

// bagPairsOfWave's pooling with queryMatrixOfWave's scoring where bagPairsOfWave multiplies two bags: a wavefront owns the
// bags [firstBag, lastBag). It decodes full tiles across bag boundaries (decodePoolTile), adds a bag's entries in order
// into the pieces l and l + 64 of its row (accumulatePiece) -- the contract's layout -- and divides them once for the
// mean. BAG_GROUP finished rows wait in registers ("held"); then
//   per held row             the bb reduction and its root, QUERY_BLOCK rows side by side; lane g keeps row g's norm
//   per block of queries     up to QUERY_BLOCK queries' pieces l and l + 64 (densePiece) into registers; their aa reductions
//                            and roots where the wavefront does not hold them already (normsAt): across groups only
//                            where one block holds every query
//   per (query, held row)    the piece products, the lane partial, ONE butterfly -- the block's side by side
// Lane s * BAG_GROUP + g collects the dot of the s-th query since the last store and held row g; after 64 / BAG_GROUP
// queries (or the last one) every lane divides its own dot by its own two norms -- the tail of pairOfSums, once per result
// -- and one store per output writes 64 / BAG_GROUP segments of BAG_GROUP consecutive floats. No row is stored.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ void queryBagsOfWave(const TrainedParams& p, const PoolParams& pool, const QueryMatrixParams& qp, uint32_t* lds)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long firstBag = (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pool.bagsPerWave;
    if (firstBag >= pool.bags) {
        return;
    }
    const unsigned long long lastBag = min(firstBag + pool.bagsPerWave, pool.bags);
    // where this wavefront's entries end while the offsets ascend: tiles are not decoded past it
    const unsigned long long runEnd = min(static_cast<unsigned long long>(pool.offsets[lastBag]), p.n);
    const uint32_t pieces = p.dim / 4;   // 1 .. 128
    const bool aligned = qp.ldQueries % 4 == 0 && reinterpret_cast<uintptr_t>(qp.queries) % 16 == 0;   // wave-uniform
    constexpr uint32_t perStore = WAVE / BAG_GROUP;   // queries whose results one store writes
    uint32_t normsAt = ~0u;   // na holds the norms of the block of queries that starts here
    float na[QUERY_BLOCK] = {};
    PoolTile tile;
    float4 held0[BAG_GROUP];
    float4 held1[BAG_GROUP];
#pragma unroll
    for (uint32_t j = 0; j < BAG_GROUP; ++j) {
        held0[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        held1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

#pragma nounroll
    for (unsigned long long groupFirst = firstBag; groupFirst < lastBag; groupFirst += BAG_GROUP) {
        const uint32_t count = static_cast<uint32_t>(min(static_cast<unsigned long long>(BAG_GROUP), lastBag - groupFirst));
#pragma nounroll
        for (uint32_t g = 0; g < count; ++g) {
            float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);   // an empty bag is a row of +0.0 and takes part like any other
            float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
            unsigned long long begin, end;
            bagRange(pool, groupFirst + g, p.n, &begin, &end);
            if (end > begin) {
                const float entries = static_cast<float>(static_cast<uint32_t>(end - begin));
                bool started = false;
#pragma nounroll
                for (unsigned long long i = begin; i < end;) {
                    if (i < tile.start || i >= tile.end) {
                        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, i, max(runEnd, end), tile);
                    }
                    const unsigned long long upTo = min(end, tile.end);
                    const uint32_t w0 = static_cast<uint32_t>(i - tile.start);
                    const uint32_t w1 = static_cast<uint32_t>(upTo - tile.start);
                    accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane, pieces - 1), started, acc0);
                    if (pieces > WAVE) {
                        accumulatePiece<FAST>(p, mem, tile, w0, w1, min(lane + WAVE, pieces - 1), started, acc1);
                    }
                    started = true;
                    i = upTo;
                }
                if (pool.mean) {
                    acc0 = divide4(acc0, entries);
                    if (pieces > WAVE) {   // wave-uniform
                        acc1 = divide4(acc1, entries);
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < BAG_GROUP; ++j) {
                if (g == j) {   // wave-uniform
                    held0[j] = acc0;
                    held1[j] = acc1;
                }
            }
        }
        float mine = 0.f;   // lane g: held row g's norm
#pragma unroll
        for (uint32_t g0 = 0; g0 < BAG_GROUP; g0 += QUERY_BLOCK) {
            if (g0 < count) {   // wave-uniform
                float bb[QUERY_BLOCK];
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    bb[b] = lanePartial(pieceSquares(held0[g0 + b]), pieces > WAVE ? pieceSquares(held1[g0 + b]) : 0.f, lane, pieces);
                }
                butterfliesOfBlock(bb, lane);
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    const float norm = correctSqrt(bb[b]);
                    mine = lane == g0 + b ? norm : mine;
                }
            }
        }
        if (qp.norms && lane < count) {
            qp.norms[groupFirst + lane] = mine;
        }
        if (!qp.cosines && !qp.dots) {   // wave-uniform
            continue;
        }
        uint32_t l = lane;
        asm volatile("" : "+v"(l));   // (what a lane collects and the queries' addresses are worked out per group, not kept live)
        const uint32_t slot = l / BAG_GROUP;          // which of the queries since the last store this lane collects
        const uint32_t row = l - slot * BAG_GROUP;    // and which held row
        const float nbLane = __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>(row * 4u), __float_as_int(mine)));
        float naLane = 0.f;
        float dotLane = 0.f;
        uint32_t used = 0;   // queries collected since the last store, < perStore
#pragma nounroll
        for (uint32_t qb = 0; qb < qp.nQueries;) {
            // (a block never straddles a store: at least one query, at most what the lanes still have room for)
            const uint32_t valid = min(min(QUERY_BLOCK, perStore - used), qp.nQueries - qb);
            float4 x0[QUERY_BLOCK];
            float4 x1[QUERY_BLOCK];
#pragma unroll
            for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                const float* query = qp.queries + static_cast<unsigned long long>(min(qb + b, qp.nQueries - 1)) * qp.ldQueries;
                x0[b] = densePiece(query, p.dim, min(l, pieces - 1), aligned);
                x1[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pieces > WAVE) {
                    x1[b] = densePiece(query, p.dim, min(l + WAVE, pieces - 1), aligned);
                }
            }
            if (qb != normsAt) {   // wave-uniform
                float aa[QUERY_BLOCK];
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    aa[b] = lanePartial(pieceSquares(x0[b]), pieces > WAVE ? pieceSquares(x1[b]) : 0.f, lane, pieces);
                }
                butterfliesOfBlock(aa, lane);
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    na[b] = correctSqrt(aa[b]);
                }
                normsAt = qb;
            }
#pragma unroll
            for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                if (b < valid) {   // wave-uniform
                    naLane = slot == used + b ? na[b] : naLane;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < BAG_GROUP; ++j) {
                if (j < count) {   // wave-uniform
                    float dot[QUERY_BLOCK];
#pragma unroll
                    for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                        dot[b] = lanePartial(
                            pieceProducts(x0[b], held0[j]), pieces > WAVE ? pieceProducts(x1[b], held1[j]) : 0.f, lane, pieces);
                    }
                    butterfliesOfBlock(dot, lane);
#pragma unroll
                    for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                        if (b < valid) {   // wave-uniform
                            dotLane = lane == (used + b) * BAG_GROUP + j ? dot[b] : dotLane;
                        }
                    }
                }
            }
            qb += valid;
            used += valid;
            if (used == perStore || qb == qp.nQueries) {   // wave-uniform
                // slot s holds query qb - used + s (< nQueries) for s < used; row < count: groupFirst + row < bags <= ldOut
                if (slot < used && row < count) {
                    const unsigned long long at = (qb - used + slot) * qp.ldOut + groupFirst + row;
                    if (qp.dots) {
                        qp.dots[at] = dotLane;
                    }
                    if (qp.cosines) {
                        qp.cosines[at] = __fdiv_rn(dotLane, mulRn(unitDivisor(naLane), unitDivisor(nbLane)));
                    }
                }
                used = 0;
            }
        }
    }
}
