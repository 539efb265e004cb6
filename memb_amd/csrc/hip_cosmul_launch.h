// 3CosMul scores and the k best candidates by them, host side (include/memb_hip_cosmul.h): the argument checks, how the
// workspace is cut into lists, cosines and scores and the candidates into slices, the launch of cosmul_scores, and the
// implementations of the entry points. The kernel is memb_hip_cosmul.hip's, handed over as an address (hip_cosmul.h).
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after
// hip_analogies_launch.h (excludedListRefusal, excludingTopkSelection) and hip_query_topk_launch.h (launchTopk, the lists
// and slices). The first part needs neither a context nor the HIP runtime: tests/cpp/cosmul_planning_main.cpp includes this
// file behind hip_analogies_launch.h with MEMB_HIP_QUERIES_PLANNING_ONLY defined and runs that part alone under the host
// sanitizers.
#pragma once

// What memb_hip_cosmul_scores_device refuses, or null.
inline const char* cosmulScoresRefusal(
    int device, const float* cosines, size_t ld, const uint32_t* offsets, const uint32_t* negativesFrom, size_t nQuestions,
    size_t n, const float* scores, size_t ldScores)
{
    if (device < 0) {
        return "device must be a HIP device";
    }
    if (nQuestions > memb_cosmul::MAX_QUESTIONS || n > memb_cosmul::MAX_COLUMNS) {
        return "batch too large";
    }
    if (!offsets || !negativesFrom || !scores) {
        return "null argument: offsets, negatives_from and scores are needed";
    }
    if (n && !cosines) {
        return "null argument: cosines is needed where n > 0";
    }
    if (ld < n || ldScores < n) {
        return "ld and ld_scores must be at least n";
    }
    if (reinterpret_cast<uintptr_t>(cosines) % 4 != 0 || reinterpret_cast<uintptr_t>(offsets) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(negativesFrom) % 4 != 0 || reinterpret_cast<uintptr_t>(scores) % 4 != 0) {
        return "cosines, offsets, negatives_from and scores must be aligned to 4 bytes";
    }
    return nullptr;
}

// Blocks of cosmul_scores per question over n >= 1 columns.
inline uint32_t cosmulBlocksPerQuestion(uint64_t n)
{
    return static_cast<uint32_t>((n + memb_cosmul::SCORE_THREADS - 1) / memb_cosmul::SCORE_THREADS);
}

// The slice of the recommended workspace: planTopkSlice's rule with a row per term and a row per question, so that the
// cosines and the scores of a slice together take about SLICE_MATRIX_BYTES.
inline uint64_t cosmulRecommendedSlice(uint64_t nTerms, uint64_t nQuestions)
{
    return topkRecommendedSlice(nTerms + nQuestions);
}

// memb_hip_query_cosmul_workspace_bytes without the context: the lists of the selection over nQuestions rows, then the
// (nTerms, slice) cosines, then the (nQuestions, slice) scores; 0 where nothing is needed or the sizes are refused
inline uint64_t cosmulWorkspaceBytes(uint64_t nTerms, uint64_t nQuestions, uint64_t n, uint64_t k, bool minimal)
{
    if (k == 0 || k > memb_query_topk::MAX_K || n > (uint64_t(1) << 36) || nTerms > memb_cosmul::MAX_TERM_ROWS ||
        nQuestions > memb_cosmul::MAX_QUESTIONS || !n || !nQuestions) {
        return 0;
    }
    const uint64_t slice = std::min(n, minimal ? memb_query_topk::MIN_SLICE : cosmulRecommendedSlice(nTerms, nQuestions));
    return queryTopkListBytes(nQuestions, k) + 4 * (nTerms + nQuestions) * slice;
}

// The candidates of one slice under a workspace of workspaceBytes, by planTopkSlice's rule from nTerms + nQuestions rows:
// all n where they fit, otherwise the largest multiple of MIN_SLICE that does, at most MAX_SLICE; 0: too small.
inline uint64_t planCosmulSlice(uint64_t nTerms, uint64_t nQuestions, uint64_t n, uint64_t k, uint64_t workspaceBytes)
{
    const uint64_t lists = queryTopkListBytes(nQuestions, k);
    if (!nQuestions || !n || workspaceBytes < lists) {
        return 0;
    }
    const uint64_t fits = (workspaceBytes - lists) / (4 * (nTerms + nQuestions));
    const uint64_t slice = fits >= n ? n : fits / memb_query_topk::MIN_SLICE * memb_query_topk::MIN_SLICE;
    return std::min(slice, memb_query_topk::MAX_SLICE);
}

// What memb_hip_query_cosmul_nearest_device refuses before it looks at the model, or null. dim: the model's. The limits
// of the matrix call over the terms are asked of queryMatrixArgumentsRefusal, with the workspace standing for the matrix.
inline const char* cosmulNearestArgumentsRefusal(
    const float* terms, size_t nTerms, size_t ldTerms, size_t dim, const uint32_t* offsets, const uint32_t* negativesFrom,
    size_t nQuestions, const uint32_t* rows, size_t n, uint32_t k, const int64_t* excluded, size_t width, size_t ldExcluded,
    const float* values, const int64_t* positions, size_t ldOut, const void* workspace, size_t workspaceBytes)
{
    if (k == 0 || k > memb_query_topk::MAX_K) {
        return "k must be 1 .. 64";
    }
    if (!values || !positions) {
        return "null argument: values and positions are needed";
    }
    if (ldOut < k) {
        return "ld_out must be at least k";
    }
    if (nTerms > memb_cosmul::MAX_TERM_ROWS || nQuestions > memb_cosmul::MAX_QUESTIONS) {
        return "batch too large: at most 2^16 terms and 2^16 questions";
    }
    if (!offsets || !negativesFrom) {
        return "null argument: offsets and negatives_from are needed";
    }
    if (reinterpret_cast<uintptr_t>(offsets) % 4 != 0 || reinterpret_cast<uintptr_t>(negativesFrom) % 4 != 0) {
        return "offsets and negatives_from must be aligned to 4 bytes";
    }
    if (const char* refusal = queryMatrixArgumentsRefusal(terms, nTerms, ldTerms, dim, rows, n, values, nullptr, n, nullptr)) {
        return refusal;
    }
    if (const char* refusal = excludedListRefusal(excluded, width, ldExcluded)) {
        return refusal;
    }
    if (reinterpret_cast<uintptr_t>(positions) % 8 != 0 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) {
        return "positions and workspace must be aligned to 8 bytes";
    }
    if (n && nQuestions && (!workspace || !planCosmulSlice(nTerms, nQuestions, n, k, workspaceBytes))) {
        return "workspace too small: memb_hip_query_cosmul_workspace_bytes(.., minimal) says how large";
    }
    return nullptr;
}

#ifndef MEMB_HIP_QUERIES_PLANNING_ONLY

// cosmul_scores over n >= 1 columns and nQuestions >= 1 questions. The current device is the matrix's. Arguments as
// cosmulScoresRefusal lets them through.
int launchCosmulScores(
    const float* cosines, size_t ld, const uint32_t* offsets, const uint32_t* negativesFrom, size_t nQuestions, size_t n,
    float* scores, size_t ldScores, hipStream_t stream)
{
    memb_cosmul::CosmulParams params{};
    params.cosines = cosines;
    params.offsets = offsets;
    params.negativesFrom = negativesFrom;
    params.scores = scores;
    params.ld = ld;
    params.ldScores = ldScores;
    params.nQuestions = static_cast<uint32_t>(nQuestions);
    params.n = static_cast<uint32_t>(n);
    params.blocksPerQuestion = cosmulBlocksPerQuestion(n);
    void* arguments[1] = {&params};
    // (blocks == 0 where the elements do not fit one launch: launchWithoutLds refuses)
    return launchWithoutLds(
        memb_cosmul::scoresKernel(), memb::gridBlocks(1, 1, uint64_t(nQuestions) * params.blocksPerQuestion),
        memb_cosmul::SCORE_THREADS, arguments, stream);
}

// memb_hip_cosmul_scores_device
int cosmul_scores_device_checked(
    int device, const float* cosines, size_t ld, const uint32_t* offsets, const uint32_t* negativesFrom, size_t nQuestions,
    size_t n, float* scores, size_t ldScores, void* stream)
{
    if (const char* refusal = cosmulScoresRefusal(device, cosines, ld, offsets, negativesFrom, nQuestions, n, scores, ldScores)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQuestions == 0 || n == 0) {
        return MEMB_HIP_OK;
    }
    DeviceScope deviceScope(device);
    HIP_TRY(deviceScope.status());
    return launchCosmulScores(cosines, ld, offsets, negativesFrom, nQuestions, n, scores, ldScores, static_cast<hipStream_t>(stream));
}

// memb_hip_query_cosmul_nearest_device: query_topk_device_checked's loop over the slices with the scores between the
// matrix and the selection
int query_cosmul_nearest_device_checked(
    memb_hip_ctx* ctx, const float* terms, size_t nTerms, size_t ldTerms, const uint32_t* offsets, const uint32_t* negativesFrom,
    size_t nQuestions, const uint32_t* rows, size_t n, uint32_t k, const int64_t* excluded, size_t width, size_t ldExcluded,
    float* values, int64_t* positions, size_t ldOut, void* workspace, size_t workspaceBytes, void* stream)
{
    if (!ctx) {
        return fail(MEMB_HIP_ERR_INVALID, "null argument: ctx");
    }
    if (const char* refusal = cosmulNearestArgumentsRefusal(
            terms, nTerms, ldTerms, ctx->dim, offsets, negativesFrom, nQuestions, rows, n, k, excluded, width, ldExcluded, values,
            positions, ldOut, workspace, workspaceBytes)) {
        return fail(MEMB_HIP_ERR_INVALID, refusal);
    }
    if (nQuestions == 0) {
        return MEMB_HIP_OK;
    }
    const char* reason = n ? fusedRefusal(ctx, FUSED_QUERIES) : nullptr;   // (n == 0 fills the empty slots for every model)
    if (reason) {
        return failFused(FUSED_QUERIES, reason);
    }
    DeviceScope deviceScope(ctx->device);
    HIP_TRY(deviceScope.status());
    memb_analogies::ExcludedList list{};
    const TopkSelection selection = excludingTopkSelection(&list, excluded, width, ldExcluded);
    const hipStream_t hipStream = static_cast<hipStream_t>(stream);
    if (n == 0) {
        return launchTopk(selection, nullptr, nQuestions, 0, 0, 0, k, false, values, positions, ldOut, nullptr, hipStream);
    }
    const size_t slice = planCosmulSlice(nTerms, nQuestions, n, k, workspaceBytes);
    float* cosines = reinterpret_cast<float*>(static_cast<char*>(workspace) + queryTopkListBytes(nQuestions, k));
    float* scores = cosines + nTerms * slice;
    for (size_t start = 0; start < n; start += slice) {
        const size_t count = std::min(slice, n - start);
        // (no term at all: no matrix, and cosmul_scores reads none)
        int code = query_matrix_device_checked(ctx, terms, nTerms, ldTerms, rows + start, count, cosines, nullptr, slice, nullptr, stream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchCosmulScores(cosines, slice, offsets, negativesFrom, nQuestions, count, scores, slice, hipStream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
        code = launchTopk(
            selection, scores, nQuestions, count, slice, static_cast<int64_t>(start), k, start != 0, values, positions, ldOut,
            workspace, hipStream);
        if (code != MEMB_HIP_OK) {
            return code;
        }
    }
    return MEMB_HIP_OK;
}

// memb_hip_query_cosmul_workspace_bytes
size_t query_cosmul_workspace_bytes(const memb_hip_ctx* ctx, size_t nTerms, size_t nQuestions, size_t n, uint32_t k, bool minimal)
{
    return ctx ? static_cast<size_t>(cosmulWorkspaceBytes(nTerms, nQuestions, n, k, minimal)) : 0;
}

// memb_hip_query_cosmul_kernel_name
const char* query_cosmul_kernel_name(const memb_hip_ctx* ctx)
{
    if (!ctx) {
        return "cosmul_scores";
    }
    return fusedRefusal(ctx, FUSED_QUERIES) ? "" : "query_matrix_trained+cosmul_scores+topk_select_excluding+topk_merge";
}

#endif  // MEMB_HIP_QUERIES_PLANNING_ONLY
