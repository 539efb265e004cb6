// The kernels of memb_hip_analogies.hip (include/memb_hip_analogies.h: the selection of memb_hip_query_topk.h with a list
// of positions per row that are no candidates, and sums of weighted rows in a fixed order) as memb_hip.hip launches them
// (hip_analogies_launch.h): host addresses for hipLaunchKernel, as memb::KernelHandle.
#pragma once

#include <cstdint>

#include "hip_query_topk.h"   // (TopkParams: topk_select_excluding takes topk_select's parameters first)

namespace memb_analogies {

// topk_select_excluding's SECOND parameter, behind the TopkParams of the launch: the same for every slice of a call, since
// its entries are positions (base + column) and the slice's base travels in TopkParams.
struct ExcludedList {
    const long long* excluded;   // row r: excluded[r * ld .. + width); null where width == 0
    unsigned long long ld;       // in entries, >= width
    uint32_t width;              // 0 .. MAX_EXCLUDED: one entry per lane
};

struct WeightedSumParams {
    const float* matrix;         // entry e: matrix[e * ld .. + dim)
    const float* weights;        // one per entry; null: all +1
    const uint32_t* offsets;     // nSums + 1: sum q takes the entries offsets[q] .. offsets[q + 1]
    float* out;                  // sum q: out[q * ldOut .. + dim)
    unsigned long long ld;       // in floats, >= dim
    unsigned long long ldOut;    // in floats, >= dim
    uint32_t nSums;
    uint32_t dim;
};

constexpr uint32_t MAX_EXCLUDED = 64;        // one entry per lane
constexpr uint32_t SUM_THREADS = 256;        // weighted_rows_sum: one thread per output element
constexpr uint64_t MAX_SUMS = 1ull << 24;
constexpr uint64_t MAX_SUM_DIM = 1ull << 16;

// topk_select_excluding: topk_select's grid and block (hip_query_topk.h); a survivor whose column the row's list names is
// not inserted. Parameters: TopkParams, ExcludedList. No LDS.
memb::KernelHandle selectExcludingKernel();
// weighted_rows_sum: ceil(nSums * dim / SUM_THREADS) blocks of SUM_THREADS threads, one thread per output element. No LDS.
memb::KernelHandle weightedRowsSumKernel();

}  // namespace memb_analogies
