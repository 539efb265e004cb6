// Device code of the pair kernels (memb_hip_pairs.hip): a piece's sum of products, three butterflies run side by side, the
// tail that turns the three sums into a cosine, the walk of a wavefront over its run of entries of a trained model, and
// the one-pair-per-wavefront loop over a dense matrix. Included inside the unit's anonymous namespace, behind
// hip_norms_kernels.h, whose pieceSquares, laneXor, correctSqrt, unitDivisor and densePiece are used as they are.
#pragma once

using memb_pairs::DensePairParams;
using memb_pairs::PairParams;

// d = ((x0 y0 + x1 y1) + x2 y2) + x3 y3: seven single-lane operations, nothing fused (pieceSquares with two rows).
__device__ __forceinline__ float pieceProducts(float4 x, float4 y)
{
    return addRn(addRn(addRn(mulRn(x.x, y.x), mulRn(x.y, y.y)), mulRn(x.z, y.z)), mulRn(x.w, y.w));
}

// The lane partials x.y, x.x, y.y of one pair.
struct PairSums {
    float dot;
    float aa;
    float bb;
};

__device__ __forceinline__ PairSums pieceSums(float4 x, float4 y)
{
    return PairSums{pieceProducts(x, y), pieceSquares(x), pieceSquares(y)};
}

__device__ __forceinline__ PairSums addSums(PairSums a, PairSums b)
{
    return PairSums{addRn(a.dot, b.dot), addRn(a.aa, b.aa), addRn(a.bb, b.bb)};
}

// s += the three values exchanged for it, as ONE statement: the compiler waits for all three exchanges in front of it, so
// it has to issue all three before the first sum (three separate addRn it schedules as two chains and a third behind them).
__device__ __forceinline__ void addExchanged(PairSums& s, float dot, float aa, float bb)
{
    asm("v_add_f32_e32 %0, %0, %3\n\tv_add_f32_e32 %1, %1, %4\n\tv_add_f32_e32 %2, %2, %5"
        : "+v"(s.dot), "+v"(s.aa), "+v"(s.bb)
        : "v"(dot), "v"(aa), "v"(bb));
}

__device__ __forceinline__ float halfXor(float p, uint32_t lane)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>((lane ^ 32u) * 4u), __float_as_int(p)));
}

// The contract's butterfly (hip_norms_kernels.h: butterfly) over the three partials at once. The three chains do not
// depend on one another, so per stride three exchanges are in flight where a single butterfly has one: the dependent
// exchange chain is what bounds norms_trained. Every lane ends with the same three sums.
__device__ __forceinline__ PairSums butterflies(PairSums s, uint32_t lane)
{
    addExchanged(s, laneXor<1>(s.dot), laneXor<1>(s.aa), laneXor<1>(s.bb));
    addExchanged(s, laneXor<2>(s.dot), laneXor<2>(s.aa), laneXor<2>(s.bb));
    addExchanged(s, laneXor<4>(s.dot), laneXor<4>(s.aa), laneXor<4>(s.bb));
    addExchanged(s, laneXor<8>(s.dot), laneXor<8>(s.aa), laneXor<8>(s.bb));
    addExchanged(s, laneXor<16>(s.dot), laneXor<16>(s.aa), laneXor<16>(s.bb));
    addExchanged(s, halfXor(s.dot, lane), halfXor(s.aa, lane), halfXor(s.bb, lane));
    return s;
}

// What a pair gives: cos = dot / (max(na, eps) * max(nb, eps)), one correctly rounded product and one correctly rounded
// quotient, not clamped.
struct PairResult {
    float cosine;
    float dot;
    float na;
    float nb;
};

__device__ __forceinline__ PairResult pairOfSums(PairSums total)
{
    PairResult r;
    r.dot = total.dot;
    r.na = correctSqrt(total.aa);
    r.nb = correctSqrt(total.bb);
    r.cosine = __fdiv_rn(r.dot, mulRn(unitDivisor(r.na), unitDivisor(r.nb)));
    return r;
}

// normsOfWave's walk with bags of two entries: a wavefront owns the entries [first, last) of the 2 * pairs entries (p.rows,
// p.n), first and last even, decodes them tile by tile up to the symbol tile (decodePoolTile) in tiles of an EVEN number
// of words, so that no pair straddles two tiles, and, pair by pair, gathers the pieces l and l + 64 of both words -- the
// contract's layout --, multiplies, reduces the three partials side by side and finishes the pair. Lane j keeps pair j's
// cosine and dot, lane w word w's norm; a tile's results leave as at most three stores. No row is stored.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ void pairsOfWave(const TrainedParams& p, const PairParams& pp, uint32_t* lds)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long first = (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pp.entriesPerWave;
    if (first >= p.n) {
        return;
    }
    const unsigned long long last = min(first + pp.entriesPerWave, p.n);
    const uint32_t pieces = p.dim / 4;   // 1 .. 128
    const uint32_t tileWords = p.wordsPerWave & ~1u;   // >= 2: the launch refuses a geometry of one word per wavefront
    PoolTile tile;

#pragma nounroll
    for (unsigned long long start = first; start < last; start += tileWords) {
        // An odd wordsPerWave (nine lanes per word: 7): the tile ends one word early, at a limit of its own. decodePoolTile
        // prefetches the next tile's row ids for the limit it was given, so there the ids come from a plain load at the
        // start of each tile instead; accepted. An even wordsPerWave keeps the run's limit and the prefetch.
        const unsigned long long limit = tileWords == p.wordsPerWave ? last : min(last, start + tileWords);
        decodePoolTile<HAS_SUB, FAST>(p, mem, lane, start, limit, tile);
        const uint32_t words = static_cast<uint32_t>(tile.end - tile.start);   // even: start, last and tileWords are
        float cosine = 0.f;
        float dot = 0.f;
        float norm = 0.f;
#pragma nounroll
        for (uint32_t w = 0; w < words; w += 2) {
            const uint32_t c0 = min(lane, pieces - 1);
            PairSums sums = pieceSums(gatherPiece<FAST>(p, mem, tile, w, c0), gatherPiece<FAST>(p, mem, tile, w + 1, c0));
            if (lane >= pieces) {
                sums = PairSums{0.f, 0.f, 0.f};
            }
            if (pieces > WAVE) {   // wave-uniform
                const uint32_t c1 = min(lane + WAVE, pieces - 1);
                const PairSums both =
                    addSums(sums, pieceSums(gatherPiece<FAST>(p, mem, tile, w, c1), gatherPiece<FAST>(p, mem, tile, w + 1, c1)));
                // (selected, not added to +0.0: a lane without a second piece keeps the bits of a -0.0 product)
                if (lane + WAVE < pieces) {
                    sums = both;
                }
            }
            const PairResult r = pairOfSums(butterflies(sums, lane));
            cosine = lane == w / 2 ? r.cosine : cosine;
            dot = lane == w / 2 ? r.dot : dot;
            norm = lane == w ? r.na : lane == w + 1 ? r.nb : norm;
        }
        if (pp.cosines && lane < words / 2) {
            pp.cosines[tile.start / 2 + lane] = cosine;
        }
        if (pp.dots && lane < words / 2) {
            pp.dots[tile.start / 2 + lane] = dot;
        }
        if (pp.norms && lane < words) {
            pp.norms[tile.start + lane] = norm;
        }
    }
}

// One wavefront per pair of a dense matrix: denseRowOfWave's loop with two rows and three partials -- lane l adds the
// products and squares of the pieces l, l + 64, .. in that order, starting from piece l's --, the butterflies and the tail.
__device__ __forceinline__ void densePairOfWave(const DensePairParams& p)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const unsigned long long i =
        static_cast<unsigned long long>(blockIdx.x) * (blockDim.x / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    if (i >= p.pairs) {
        return;
    }
    const float* a = p.values + 2 * i * p.ldValues;
    const float* b = a + p.ldValues;
    const bool aligned = p.dim % 4 == 0 && p.ldValues % 4 == 0 && reinterpret_cast<uintptr_t>(p.values) % 16 == 0;
    const uint32_t pieces = p.dim / 4 + (p.dim % 4 != 0);
    PairSums sums{0.f, 0.f, 0.f};
    if (lane < pieces) {
        sums = pieceSums(densePiece(a, p.dim, lane, aligned), densePiece(b, p.dim, lane, aligned));
        for (uint32_t k = lane + WAVE; k < pieces; k += WAVE) {
            sums = addSums(sums, pieceSums(densePiece(a, p.dim, k, aligned), densePiece(b, p.dim, k, aligned)));
        }
    }
    const PairResult r = pairOfSums(butterflies(sums, lane));
    if (lane == 0) {
        if (p.cosines) {
            p.cosines[i] = r.cosine;
        }
        if (p.dots) {
            p.dots[i] = r.dot;
        }
    }
    // (the two norms from two lanes: one 4-byte store, whatever the alignment of norms beyond that of a float)
    if (p.norms && lane < 2) {
        p.norms[2 * i + lane] = lane ? r.nb : r.na;
    }
}
