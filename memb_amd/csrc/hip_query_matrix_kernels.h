// Device code of the query-matrix kernel (memb_hip_query_matrix.hip): a lane's partial of one reduction, QUERY_BLOCK
// butterflies run side by side, and the walk of a wavefront over its run of the ONE shared candidate list with a block of
// queries in registers. Included inside the unit's anonymous namespace, behind hip_pooled_kernels.h (decodePoolTile,
// gatherPiece), hip_norms_kernels.h (pieceSquares, laneXor, correctSqrt, unitDivisor, densePiece), hip_pairs_kernels.h
// (pieceProducts, halfXor) and hip_queries_kernels.h, which are used as they are.
#pragma once

using memb_query_matrix::QueryMatrixParams;

constexpr uint32_t QUERY_BLOCK = memb_query_matrix::QUERY_BLOCK;
static_assert(QUERY_BLOCK == 2 || QUERY_BLOCK == 4, "addExchangedBlock spells out two or four sums");

// The lane partial of one reduction as queriesOfWave forms each of its three: the sum over the lane's piece l (`first`)
// and its piece l + 64 (`second`), zero for a lane without a piece, and SELECTED, not added to +0.0, for a lane without a
// second piece, which keeps the bits of a -0.0 product.
__device__ __forceinline__ float lanePartial(float first, float second, uint32_t lane, uint32_t pieces)
{
    float partial = lane < pieces ? first : 0.f;
    if (pieces > WAVE) {   // wave-uniform
        const float both = addRn(partial, second);
        if (lane + WAVE < pieces) {
            partial = both;
        }
    }
    return partial;
}

// s[b] += the value exchanged for it, as ONE statement (addExchanged's reason: every exchange is issued before the first sum).
__device__ __forceinline__ void addExchangedBlock(float (&s)[2], const float (&e)[2])
{
    asm("v_add_f32_e32 %0, %0, %2\n\tv_add_f32_e32 %1, %1, %3" : "+v"(s[0]), "+v"(s[1]) : "v"(e[0]), "v"(e[1]));
}

__device__ __forceinline__ void addExchangedBlock(float (&s)[4], const float (&e)[4])
{
    asm("v_add_f32_e32 %0, %0, %4\n\tv_add_f32_e32 %1, %1, %5\n\tv_add_f32_e32 %2, %2, %6\n\tv_add_f32_e32 %3, %3, %7"
        : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3])
        : "v"(e[0]), "v"(e[1]), "v"(e[2]), "v"(e[3]));
}

template <int S>
__device__ __forceinline__ void strideOfBlock(float (&s)[QUERY_BLOCK])
{
    float e[QUERY_BLOCK];
#pragma unroll
    for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
        e[b] = laneXor<S>(s[b]);
    }
    addExchangedBlock(s, e);
}

// The contract's butterfly (butterflies()' order: laneXor strides 1 .. 16, then halfXor) over QUERY_BLOCK independent
// partials at once: the same binary tree for each, QUERY_BLOCK exchanges in flight per stride. Every lane ends with the
// same sums.
__device__ __forceinline__ void butterfliesOfBlock(float (&s)[QUERY_BLOCK], uint32_t lane)
{
    strideOfBlock<1>(s);
    strideOfBlock<2>(s);
    strideOfBlock<4>(s);
    strideOfBlock<8>(s);
    strideOfBlock<16>(s);
    float e[QUERY_BLOCK];
#pragma unroll
    for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
        e[b] = halfXor(s[b], lane);
    }
    addExchangedBlock(s, e);
}

// queriesOfWave's walk over ONE list that every query shares: a wavefront owns the candidates [first, last), decodes its
// run tile by tile up to the symbol tile (decodePoolTile, full tiles) and scores each tile against ALL queries before it
// moves on, so a compressed row is fetched and decoded once whatever nQueries is.
//   per candidate and tile   the bb reduction and its root, QUERY_BLOCK words side by side; lane w keeps word w's norm
//   per block of queries     up to QUERY_BLOCK queries' pieces l and l + 64 (densePiece, through the cache, any alignment)
//                            into registers; their aa reductions and roots where the wavefront does not hold them already
//                            (normsAt): the launch gives a wavefront several tiles only where one block holds every query
//   per (query, candidate)   the piece products, the lane partial, ONE butterfly -- the block's side by side
//   ONE query                 the word's dot and its bb are the two sums of one block: one pass over the tile
// Lane s * W + w collects the dot of the s-th query since the last store and word w, W = wordsPerWave; after floor(64 / W)
// queries (or the last one) every lane divides its own dot by its own two norms -- the tail of pairOfSums, once per
// result -- and one store per output writes floor(64 / W) row segments of W floats. No row is stored.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ void queryMatrixOfWave(const TrainedParams& p, const QueryMatrixParams& qp, uint32_t* lds)
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
    const uint32_t perStore = WAVE / p.wordsPerWave;   // >= 1: queries whose results one store writes
    uint32_t normsAt = ~0u;   // na holds the norms of the block of queries that starts here
    float na[QUERY_BLOCK] = {};
    PoolTile tile;

#pragma nounroll
    for (unsigned long long start = first; start < last; start += p.wordsPerWave) {
        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, start, last, tile);
        const uint32_t words = static_cast<uint32_t>(tile.end - tile.start);   // 1 .. wordsPerWave
        float mine = 0.f;   // lane w: word w's norm
        if (qp.nQueries == 1 && (qp.cosines || qp.dots)) {   // wave-uniform
            // ONE query: a word's dot and its bb are the two sums of one block -- queriesOfWave's walk with the query's
            // squares taken out of it: the word's pieces are gathered once and no second pass goes over the tile
            uint32_t l = lane;
            asm volatile("" : "+v"(l));   // (the query's addresses are worked out here, per tile, not kept live)
            const float4 x0 = densePiece(qp.queries, p.dim, min(l, pieces - 1), aligned);
            float4 x1 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pieces > WAVE) {   // wave-uniform
                x1 = densePiece(qp.queries, p.dim, min(l + WAVE, pieces - 1), aligned);
            }
            if (normsAt != 0) {   // wave-uniform: once per wavefront
                na[0] = correctSqrt(butterfly(lanePartial(pieceSquares(x0), pieces > WAVE ? pieceSquares(x1) : 0.f, l, pieces), l));
                normsAt = 0;
            }
            float dot = 0.f;
#pragma nounroll
            for (uint32_t w = 0; w < words; ++w) {
                const float4 y0 = gatherPiece<FAST>(p, mem, tile, w, min(l, pieces - 1));
                float4 y1 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pieces > WAVE) {   // wave-uniform
                    y1 = gatherPiece<FAST>(p, mem, tile, w, min(l + WAVE, pieces - 1));
                }
                float sums[QUERY_BLOCK] = {};
                sums[0] = lanePartial(pieceProducts(x0, y0), pieces > WAVE ? pieceProducts(x1, y1) : 0.f, l, pieces);
                sums[1] = lanePartial(pieceSquares(y0), pieces > WAVE ? pieceSquares(y1) : 0.f, l, pieces);
                butterfliesOfBlock(sums, l);
                const float norm = correctSqrt(sums[1]);
                dot = l == w ? sums[0] : dot;
                mine = l == w ? norm : mine;
            }
            if (l < words) {
                if (qp.norms) {
                    qp.norms[tile.start + l] = mine;
                }
                if (qp.dots) {
                    qp.dots[tile.start + l] = dot;
                }
                if (qp.cosines) {
                    qp.cosines[tile.start + l] = __fdiv_rn(dot, mulRn(unitDivisor(na[0]), unitDivisor(mine)));
                }
            }
            continue;
        }
#pragma nounroll
        for (uint32_t w0 = 0; w0 < words; w0 += QUERY_BLOCK) {
            float bb[QUERY_BLOCK];
#pragma unroll
            for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                const uint32_t w = min(w0 + b, words - 1);
                const float one = pieceSquares(gatherPiece<FAST>(p, mem, tile, w, min(lane, pieces - 1)));
                float two = 0.f;
                if (pieces > WAVE) {   // wave-uniform
                    two = pieceSquares(gatherPiece<FAST>(p, mem, tile, w, min(lane + WAVE, pieces - 1)));
                }
                bb[b] = lanePartial(one, two, lane, pieces);
            }
            butterfliesOfBlock(bb, lane);
#pragma unroll
            for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                if (w0 + b < words) {   // wave-uniform
                    const float norm = correctSqrt(bb[b]);
                    mine = lane == w0 + b ? norm : mine;
                }
            }
        }
        if (qp.norms && lane < words) {
            qp.norms[tile.start + lane] = mine;
        }
        if (!qp.cosines && !qp.dots) {   // wave-uniform
            continue;
        }
        uint32_t l = lane;
        asm volatile("" : "+v"(l));   // (what a lane collects and the queries' addresses are worked out per tile, not kept live)
        const uint32_t slot = l / p.wordsPerWave;          // which of the queries since the last store this lane collects
        const uint32_t word = l - slot * p.wordsPerWave;   // and which word of the tile
        const float nbLane = __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>(word * 4u), __float_as_int(mine)));
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
                const float* row = qp.queries + static_cast<unsigned long long>(min(qb + b, qp.nQueries - 1)) * qp.ldQueries;
                x0[b] = densePiece(row, p.dim, min(l, pieces - 1), aligned);
                x1[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pieces > WAVE) {
                    x1[b] = densePiece(row, p.dim, min(l + WAVE, pieces - 1), aligned);
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
#pragma nounroll
            for (uint32_t w = 0; w < words; ++w) {
                const float4 y0 = gatherPiece<FAST>(p, mem, tile, w, min(lane, pieces - 1));
                float4 y1 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pieces > WAVE) {   // wave-uniform
                    y1 = gatherPiece<FAST>(p, mem, tile, w, min(lane + WAVE, pieces - 1));
                }
                float dot[QUERY_BLOCK];
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    dot[b] = lanePartial(pieceProducts(x0[b], y0), pieces > WAVE ? pieceProducts(x1[b], y1) : 0.f, lane, pieces);
                }
                butterfliesOfBlock(dot, lane);
#pragma unroll
                for (uint32_t b = 0; b < QUERY_BLOCK; ++b) {
                    if (b < valid) {   // wave-uniform
                        dotLane = lane == (used + b) * p.wordsPerWave + w ? dot[b] : dotLane;
                    }
                }
            }
            qb += valid;
            used += valid;
            if (used == perStore || qb == qp.nQueries) {   // wave-uniform
                // slot s holds query qb - used + s (< nQueries) for s < used; word < words: tile.start + word < n <= ldOut
                if (slot < used && word < words) {
                    const unsigned long long at = (qb - used + slot) * qp.ldOut + tile.start + word;
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
