// Device code of the bag-pair kernel (memb_hip_bag_pairs.hip): the walk of a wavefront over its run of whole pairs of
// bags of a trained model. Included inside the unit's anonymous namespace, behind hip_pooled_kernels.h (bagRange,
// decodePoolTile, accumulatePiece, divide4), hip_norms_kernels.h and hip_pairs_kernels.h, whose pieceSums, addSums,
// butterflies and pairOfSums are used as they are.
#pragma once

using memb_bag_pairs::BagPairParams;

// pool_trained's register form with the cosine of pairsOfWave where pool_trained stores a row: a wavefront owns the bags
// [firstBag, lastBag), an EVEN number of them from an even bag on, so whole pairs; it decodes full tiles across bag
// boundaries (decodePoolTile), adds a bag's entries in order into the pieces l and l + 64 of its row (accumulatePiece) --
// the contract's layout -- and divides them once for the mean. The finished row of an even bag waits in registers; when
// the odd bag behind it is finished, the two rows are multiplied piece by piece, the three partials reduced side by side
// and the pair finished. Lane 0 stores the pair's cosine and dot, the lanes 0 and 1 its two norms. No row is stored.
template <bool HAS_SUB, bool FAST>
__device__ __forceinline__ void bagPairsOfWave(const TrainedParams& p, const PoolParams& pool, const BagPairParams& bp, uint32_t* lds)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wavesPerBlock = blockDim.x / WAVE;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const WaveLds mem = setUpLds<OUT_VEC4>(p, lds);
    const unsigned long long firstBag =
        (static_cast<unsigned long long>(blockIdx.x) * wavesPerBlock + wave) * pool.bagsPerWave;   // even: bagsPerWave is
    if (firstBag >= pool.bags) {
        return;
    }
    const unsigned long long lastBag = min(firstBag + pool.bagsPerWave, pool.bags);   // even: pool.bags is
    // where this wavefront's entries end while the offsets ascend: tiles are not decoded past it
    const unsigned long long runEnd = min(static_cast<unsigned long long>(pool.offsets[lastBag]), p.n);
    const uint32_t pieces = p.dim / 4;   // 1 .. 128
    PoolTile tile;
    float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 even0 = make_float4(0.f, 0.f, 0.f, 0.f);   // the finished row of the pair's first bag
    float4 even1 = make_float4(0.f, 0.f, 0.f, 0.f);

#pragma nounroll
    for (unsigned long long bag = firstBag; bag < lastBag; ++bag) {
        unsigned long long begin, end;
        bagRange(pool, bag, p.n, &begin, &end);
        if (end <= begin) {   // an empty bag is a row of +0.0 and takes part like any other
            acc0 = make_float4(0.f, 0.f, 0.f, 0.f);
            acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const float count = static_cast<float>(static_cast<uint32_t>(end - begin));
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
                acc0 = divide4(acc0, count);
                if (pieces > WAVE) {   // wave-uniform
                    acc1 = divide4(acc1, count);
                }
            }
        }
        if (!(bag & 1)) {
            even0 = acc0;
            even1 = acc1;
            continue;
        }
        PairSums sums = pieceSums(even0, acc0);
        if (lane >= pieces) {
            sums = PairSums{0.f, 0.f, 0.f};
        }
        if (pieces > WAVE) {   // wave-uniform
            const PairSums both = addSums(sums, pieceSums(even1, acc1));
            // (selected, not added to +0.0: a lane without a second piece keeps the bits of a -0.0 product)
            if (lane + WAVE < pieces) {
                sums = both;
            }
        }
        const PairResult r = pairOfSums(butterflies(sums, lane));
        const unsigned long long pair = bag / 2;
        if (lane == 0) {
            if (bp.cosines) {
                bp.cosines[pair] = r.cosine;
            }
            if (bp.dots) {
                bp.dots[pair] = r.dot;
            }
        }
        // (the two norms from two lanes: one 4-byte store each, whatever the alignment of norms beyond that of a float)
        if (bp.norms && lane < 2) {
            bp.norms[2 * pair + lane] = lane ? r.nb : r.na;
        }
    }
}
