// The kernels of memb_hip_pooled.hip (sum / mean of each bag of rows -- include/memb_hip_pooled.h -- or of a bag's KNOWN
// rows -- include/memb_hip_pooled_known.h -- as fp32, bf16 or fp16 elements) as memb_hip.hip launches them (hip_pooled_launch.h: launchPooled):
// host addresses for hipLaunchKernel / hipFuncGetAttributes. Their first parameter is the TrainedParams / UniformParams /
// FullParams of the device headers, which both translation units include -- rows[0 .. n) are the ENTRIES, out / ld /
// colOff describe the bags' rows -- their second the PoolParams below, the third of the known kernels the KnownParams.
#pragma once

#include <cstdint>

#include "hip_kernel_handle.h"

namespace memb_pooled {

struct PoolParams {
    const uint32_t* offsets;     // [bags + 1]: bag b owns the entries [min(offsets[b], n), min(offsets[b + 1], n))
    unsigned long long bags;
    uint32_t bagsPerWave;        // trained kernels: consecutive bags a wavefront owns (launch geometry, never the result)
    uint32_t mean;               // MEMB_HIP_POOL_MEAN: divide each sum by its bag's entry count
};

struct KnownParams {
    uint32_t* counts;   // [bags] or null: the known entries of each bag
};

constexpr uint32_t TRAINED_VEC4_MAX_DIM = 512;   // two pieces per lane
constexpr uint32_t ROWWISE_WAVES = 4;
constexpr uint32_t POOLED_TILES_PER_WAVE = 4;

// PoolParams::bagsPerWave of the trained kernels (this unit's and pool_trained_union), on the host: a wavefront owns a run
// of consecutive bags sized so that it decodes about POOLED_TILES_PER_WAVE tiles of wordsPerWave entries
// (tilesPerWaveSwitch, the option tiles_per_wave: that many where it is not 0), fewer while the grid would not fill the
// cuCount CUs with wavesPerCu wavefronts each, at most 1 << 16. A bag is never split: ONE enormous bag is walked by one
// wavefront, correct and slow.
inline uint32_t pooledBagsPerWave(
    uint32_t tilesPerWaveSwitch, uint32_t wordsPerWave, uint64_t n, uint64_t bags, uint32_t cuCount, uint32_t wavesPerCu)
{
    const uint64_t tilesPerWave = tilesPerWaveSwitch ? tilesPerWaveSwitch : POOLED_TILES_PER_WAVE;
    const uint64_t entriesPerBag = n / (bags ? bags : 1);
    const uint64_t tilesOfEntries = tilesPerWave * wordsPerWave / (entriesPerBag ? entriesPerBag : 1);
    const uint64_t fillsTheCus = bags / (uint64_t(cuCount) * wavesPerCu);
    uint64_t owned = tilesOfEntries < fillsTheCus ? tilesOfEntries : fillsTheCus;
    owned = owned < (1u << 16) ? owned : (1u << 16);
    return static_cast<uint32_t>(owned ? owned : 1);
}

enum class PoolStorage { Trained, Uniform, Full };

// The kernel of a pooled lookup (address null where no instance exists: HAS_SUB with FAST, an outType that is no
// MEMB_HIP_OUT_*; name: the kernel family). known: the family that leaves a bag's unknown entries out and counts the others.
//   Trained   pool_trained<HAS_SUB, FAST, VEC4> (fp32), pool_trained_narrow<HAS_SUB, FAST, VEC4, OUT> (bf16 / fp16),
//             pool_known_trained<HAS_SUB, FAST, VEC4, OUT>. vec4: register accumulators of pieces of four elements (dim a
//             multiple of 4 and at most TRAINED_VEC4_MAX_DIM, out / ld / colOff aligned to a piece), else the column form
//             for any dim -- fp32: partial sums parked in the bag's columns of `out`; bf16 / fp16: register blocks of 512
//             columns, one walk of the bag each. All of them take pool_trained's LDS (an fp32 codebook).
//   Uniform   pool_uniform, pool_uniform_narrow<OUT>, pool_known_uniform<OUT>   } one wavefront per bag, blocks of
//   Full      pool_full, pool_full_narrow<OUT>, pool_known_full<OUT>            } ROWWISE_WAVES wavefronts
// (hasSub, fast, vec4: trained only)
memb::KernelHandle pooledKernel(PoolStorage storage, bool hasSub, bool fast, bool vec4, int outType, bool known);

}  // namespace memb_pooled
