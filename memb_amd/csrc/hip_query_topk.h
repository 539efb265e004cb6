// The kernels of memb_hip_query_topk.hip (include/memb_hip_query_topk.h: the k best columns of every row of a dense fp32
// matrix, by the total order of that header) as memb_hip.hip launches them (hip_query_topk_launch.h): host addresses for
// hipLaunchKernel, as memb::KernelHandle. Both kernels take ONE parameter, the TopkParams below.
#pragma once

#include <cstdint>

#include "hip_query_matrix.h"   // (MAX_QUERIES: the workspace of memb_hip_query_topk_device, hip_query_topk_launch.h)

namespace memb_query_topk {

struct TopkParams {
    const float* matrix;         // row q: matrix[q * ld .. + n)
    uint32_t* listValues;        // workspace: [nRows * segments * k] the bits of each segment's k best, best first
    uint32_t* listColumns;       // workspace: likewise, their columns; EMPTY_COLUMN where a segment held fewer than k
    float* values;               // output: row q is values[q * ldOut .. + k)
    long long* positions;        // output: likewise
    unsigned long long ld;       // in floats
    unsigned long long ldOut;    // in elements, >= k
    long long base;              // a column is reported as base + column
    uint32_t nRows;
    uint32_t n;                  // columns, at most MAX_COLUMNS
    uint32_t k;                  // 1 .. MAX_K
    uint32_t segments;           // per row; 0: no column at all (topk_merge alone fills the output)
    uint32_t segmentLength;      // columns per segment, a multiple of BATCH * UNROLL (launch geometry, never the result)
    uint32_t merge;              // topk_merge: the k entries the output holds take part as candidates
};

constexpr uint32_t MAX_K = 64;                  // one rank per lane
constexpr uint32_t BATCH = 64;                  // columns tested with one ballot
constexpr uint32_t UNROLL = 4;                  // batches loaded before the first is tested
constexpr uint32_t WAVES_PER_BLOCK = 4;
constexpr uint32_t EMPTY_COLUMN = 0xFFFFFFFFu;
constexpr uint64_t MAX_COLUMNS = 1ull << 31;    // of one selection: columns travel as 32 bits
constexpr uint64_t MAX_ROWS = 1ull << 24;
// A segment is never shorter than this (a shorter one leaves more lists to merge than columns to skip), and a row is cut
// into segments only until TARGET_WAVES wavefronts exist or MAX_SEGMENTS lists per row would have to be merged by the one
// wavefront of topk_merge. Launch geometry: never the result. tests/test_gpu_query_topk.py sizes its matrices by these.
constexpr uint32_t MIN_SEGMENT = 1024;
constexpr uint32_t TARGET_WAVES = 8192;
constexpr uint32_t MAX_SEGMENTS = 256;
// memb_hip_query_topk_device: the recommended workspace holds a (n_queries, slice) matrix of about this many bytes
// (DESIGN.md section 5.12 has the values that were tried), and no slice is narrower than MIN_SLICE columns or, so that a
// slice's columns fit 32 bits, wider than MAX_SLICE.
constexpr uint64_t SLICE_MATRIX_BYTES = 32ull << 20;
constexpr uint64_t MIN_SLICE = 64;
constexpr uint64_t MAX_SLICE = 1ull << 30;

// topk_select: one wavefront per (row, segment) writes its sorted list to the workspace. Grid: ceil(nRows * segments /
// WAVES_PER_BLOCK) blocks of WAVES_PER_BLOCK wavefronts. No LDS.
memb::KernelHandle selectKernel();
// topk_merge: one wavefront per row merges the row's lists and, with `merge`, what the output holds, and writes the
// output. Grid: ceil(nRows / WAVES_PER_BLOCK) blocks. No LDS.
memb::KernelHandle mergeKernel();

}  // namespace memb_query_topk
