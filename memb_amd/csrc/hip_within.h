// The kernels of memb_hip_within.hip (include/memb_hip_within.h: per row of a dense fp32 matrix the LIST of the candidates
// that precede a mark in the selection's order, in CSR form) as memb_hip.hip launches them (hip_within_launch.h): host
// addresses for hipLaunchKernel, as memb::KernelHandle. All three kernels take ONE parameter, the WithinParams below. The
// device code is hip_within_kernels.h; the geometry of a block (COUNT_THREADS, COLUMNS_PER_THREAD, BLOCK_RUN) and the
// limits are the rank unit's.
#pragma once

#include <cstdint>

#include "hip_ranks.h"   // (the geometry of a block inside a row, MAX_ROWS, MAX_COLUMNS; MAX_EXCLUDED beneath it)

namespace memb_within {

struct WithinParams {
    const float* matrix;           // row q: matrix[q * ld .. + n)
    const float* thresholds;       // nRows: t_q
    const long long* marks;        // nRows: p_q, a position (base + column)
    const long long* excluded;     // row q: excluded[q * ldExcluded .. + width); null where width == 0
    const long long* offsets;      // nRows + 1: row q's segment of positions / values
    long long* cursors;            // nRows: the entries row q found so far
    long long* positions;          // capacity
    float* values;                 // capacity, or null: not written
    uint32_t* totals;              // workspace: [nRows * blocksPerRow], block b of within_count stores totals[b]
    long long* starts;             // workspace: [nRows * blocksPerRow], within_starts stores block b's first destination
    unsigned long long ld;         // in floats, >= n
    unsigned long long ldExcluded; // in entries, >= width
    long long base;                // a column is the position base + column; >= 0
    long long capacity;            // entries of positions and values; no destination at or beyond it is written
    uint32_t nRows;
    uint32_t n;                    // columns, at most memb_ranks::MAX_COLUMNS
    uint32_t blocksPerRow;         // ceil(n / BLOCK_RUN): block b works in row b / blocksPerRow; 0 where n == 0
    uint32_t width;                // 0 .. memb_analogies::MAX_EXCLUDED: one entry per lane of a block's first wavefront
    uint32_t accumulate;           // row q goes on at offsets[q] + cursors[q], and cursors[q] grows
};

constexpr uint32_t STARTS_WAVES = 4;             // within_starts: wavefronts, that is rows, per block
constexpr uint64_t MAX_CAPACITY = 1ull << 62;    // destinations are int64

// within_count: nRows * blocksPerRow blocks of memb_ranks::COUNT_THREADS threads, neighbouring lanes on neighbouring
// columns of one row. Static LDS: the wavefronts' counts and the row's non-candidates inside the block's run.
memb::KernelHandle countKernel();
// within_starts: ceil(nRows / STARTS_WAVES) blocks of STARTS_WAVES wavefronts, one wavefront per row. No LDS.
memb::KernelHandle startsKernel();
// within_write: within_count's grid. Static LDS: a count per (load step, wavefront) and the non-candidates likewise.
memb::KernelHandle writeKernel();

}  // namespace memb_within
