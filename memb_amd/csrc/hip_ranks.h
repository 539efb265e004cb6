// The kernels of memb_hip_ranks.hip (include/memb_hip_ranks.h: per row of a dense fp32 matrix the number of candidates
// that precede a mark in the selection's order) as memb_hip.hip launches them (hip_ranks_launch.h): host addresses for
// hipLaunchKernel, as memb::KernelHandle. Both kernels take ONE parameter, the RankParams below. The device code is
// hip_ranks_kernels.h.
#pragma once

#include <cstdint>

#include "hip_analogies.h"   // (MAX_EXCLUDED, the width of a list of non-candidates, and the slices of the fused call beneath it)

namespace memb_ranks {

struct RankParams {
    const float* matrix;           // row q: matrix[q * ld .. + n)
    const float* thresholds;       // nRows: t_q
    const long long* marks;        // nRows: p_q, a position (base + column)
    const long long* excluded;     // row q: excluded[q * ldExcluded .. + width); null where width == 0
    uint32_t* partials;            // workspace: [nRows * blocksPerRow], block b of rank_count stores partials[b]
    long long* counts;             // nRows
    unsigned long long ld;         // in floats, >= n
    unsigned long long ldExcluded; // in entries, >= width
    long long base;                // a column is the position base + column; >= 0
    uint32_t nRows;
    uint32_t n;                    // columns, at most MAX_COLUMNS
    uint32_t blocksPerRow;         // ceil(n / BLOCK_RUN): block b counts in row b / blocksPerRow; 0 where n == 0
    uint32_t width;                // 0 .. memb_analogies::MAX_EXCLUDED: one entry per lane of rank_fold
    uint32_t accumulate;           // rank_fold adds to counts instead of storing
};

constexpr uint32_t COUNT_THREADS = 256;         // rank_count: four wavefronts inside one row
constexpr uint32_t COLUMNS_PER_THREAD = 8;      // loads issued back to back, COUNT_THREADS columns apart (geometry, never the result)
constexpr uint32_t BLOCK_RUN = COUNT_THREADS * COLUMNS_PER_THREAD;   // the columns of one block and one partial count
constexpr uint32_t FOLD_WAVES = 4;              // rank_fold: wavefronts, that is rows, per block
constexpr uint64_t MAX_ROWS = 1ull << 16;
constexpr uint64_t MAX_COLUMNS = 1ull << 31;    // of one launch: columns travel as 32 bits, and a count fits 32 bits

// rank_count: nRows * blocksPerRow blocks of COUNT_THREADS threads, neighbouring lanes on neighbouring columns of one row.
// 16 bytes of static LDS.
memb::KernelHandle countKernel();
// rank_fold: ceil(nRows / FOLD_WAVES) blocks of FOLD_WAVES wavefronts, one wavefront per row. No LDS.
memb::KernelHandle foldKernel();

}  // namespace memb_ranks
