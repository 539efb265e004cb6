// What the decode-fused kernel families share on the host: pool_trained, norms_trained / unit_trained, pairs_trained,
// bag_pairs_trained, query_trained, query_matrix_trained and query_bags_trained are the one-tile decode up to the symbol
// tile, so they run on its plan, its LDS and its block size. Here: which models they take (fusedRefusal), the plan of a
// launch (planFused), and the end of every launch of a kernel that another translation unit hands over as a
// memb::KernelHandle -- launchOwnedRuns for grids of wavefronts that own a run of items each, launchWithoutLds for the
// kernels without dynamic LDS. A family's own launch keeps its selector, the items a wavefront owns and its parameters.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the plans
// (hip_decode_plan.h) and before the launches that use it; see that file for the overview.
#pragma once

// How a family words its refusal of a model, and what it asks beyond the shared conditions.
struct FusedFamily {
    const char* prefix;         // "fused pair kernel"
    const char* advice;         // what the caller can do instead
    uint32_t minWordsPerWave;   // 2: pairs_trained, whose tiles hold whole pairs; 1 otherwise
};

constexpr FusedFamily FUSED_NORMS{"fused norm kernels", "decode the rows and use the dense entry points", 1};
constexpr FusedFamily FUSED_PAIRS{"fused pair kernel", "decode the rows and use the dense entry point", 2};
constexpr FusedFamily FUSED_BAG_PAIRS{"fused bag-pair kernel", "pool the bags and use the dense pair entry point", 1};
constexpr FusedFamily FUSED_QUERIES{"fused query kernel", "decode the candidates and use the dense pair entry point", 1};
constexpr FusedFamily FUSED_QUERY_BAGS{"fused query-bags kernel", "pool the bags and use the dense pair entry point", 1};

// Why the fused kernels of a family (other than pool_trained, which has a form for every model) do not take this model, or
// null: trained storage, and pool_trained's register form of two 16-byte pieces per lane.
const char* fusedRefusal(const memb_hip_ctx* ctx, const FusedFamily& family)
{
    static_assert(memb_pooled::TRAINED_VEC4_MAX_DIM == 512, "the refusal names the limit");
    if (ctx->storage != memb::wire::Storage_Trained) {
        return "trained storage only";
    }
    if (ctx->dim % 4 != 0 || ctx->dim > memb_pooled::TRAINED_VEC4_MAX_DIM) {
        return "dim must be a multiple of 4 and at most 512";
    }
    if (WAVE / ctx->lanesPerWord < family.minWordsPerWave) {
        return "a wavefront of this geometry holds fewer than two words";
    }
    return nullptr;
}

// MEMB_HIP_UNSUPPORTED with the family's words for fusedRefusal's reason.
int failFused(const FusedFamily& family, const char* reason)
{
    return fail(MEMB_HIP_UNSUPPORTED, std::string(family.prefix) + ": " + reason + " (" + family.advice + ")");
}

// The plan of a fused launch: the decode's parameters and the block the kernel shares with the one-tile decode.
struct FusedPlan {
    TrainedParams trained;
    uint32_t waves;      // wavefronts per block
    uint32_t ldsBytes;   // dynamic LDS per block
};

int inconsistentGeometry()
{
    return fail(MEMB_HIP_ERR_INVALID, "internal error: inconsistent decode geometry");
}

// Plans a fused launch over lookup.rows[0 .. lookup.n): a decode of max(n, 1) fp32 rows (the kernels add fp32 centroids
// whatever they store, so LDS holds an fp32 codebook) by the one-tile kernel with the usual index (planTrained, force = 0),
// while the kernel is told the true n -- a pooled call may have bags and no entry. lookup.out / ld / colOff describe the
// rows a kernel stores (null / dim / 0 where it stores none); they reach the kernel as they are.
int planFused(const memb_hip_ctx* ctx, const Lookup& lookup, FusedPlan* plan)
{
    Lookup planned = lookup;
    planned.n = std::max<size_t>(lookup.n, 1);
    planned.outType = MEMB_HIP_OUT_F32;
    TrainedPlan decode;
    const int code = planTrained(ctx, planned, 0, false, rowsUnordered(ctx, false), &decode);
    if (code != MEMB_HIP_OK) {
        return code;
    }
    if (!decode.geometry.waves) {
        return fail(MEMB_HIP_ERR_INVALID, "decode tables and bitstream slots do not fit into LDS");
    }
    TrainedParams& trained = plan->trained;
    trained = lookupParams(ctx);
    trained.rows = lookup.rows;
    trained.out = static_cast<float*>(lookup.out);
    trained.n = lookup.n;
    trained.ld = lookup.ld;
    trained.colOff = lookup.colOff;
    if (!lookupParamsConsistent(ctx, trained, decode.geometry) || lookup.ld < lookup.colOff + trained.dim) {
        return inconsistentGeometry();
    }
    plan->waves = decode.geometry.waves;
    plan->ldsBytes = decode.geometry.ldsBytes;
    return MEMB_HIP_OK;
}

// blocks == 0: memb::gridBlocks' "too many". dynamicLds: through launchKernelAddress, which raises the kernel's dynamic
// LDS limit on first use; else launched as it is -- that call is refused for a kernel with static LDS of its own, as the
// scan kernels have, and the others without dynamic LDS have no use for it.
int launchBlocks(
    const memb::KernelHandle& kernel, uint32_t blocks, uint32_t threads, bool dynamicLds, uint32_t ldsBytes, void** arguments,
    hipStream_t stream)
{
    if (!blocks) {
        return fail(MEMB_HIP_ERR_INVALID, "batches too large for one launch");
    }
    hipError_t status;
    if (dynamicLds) {
        status = launchKernelAddress(kernel.address, dim3(blocks), dim3(threads), ldsBytes, stream, arguments);
    } else {
        status = !kernel.address ? hipErrorInvalidDeviceFunction
                                 : hipLaunchKernel(kernel.address, dim3(blocks), dim3(threads), arguments, 0, stream);
        status = status != hipSuccess ? status : hipGetLastError();
    }
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string(kernel.name) + " launch: " + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// The end of every launch whose wavefronts own a run of consecutive items (bags, rows, entries, candidates): blocks of
// `waves` wavefronts with ldsBytes of dynamic LDS (0 for the row-wise pooled kernels) over count >= 1 items, perWave per
// wavefront -- which the kernel reads from its parameters, set by the caller.
int launchOwnedRuns(
    const memb::KernelHandle& kernel, uint32_t waves, uint32_t ldsBytes, uint32_t perWave, uint64_t count, void** arguments,
    hipStream_t stream)
{
    return launchBlocks(kernel, memb::gridBlocks(waves, perWave, count), waves * WAVE, true, ldsBytes, arguments, stream);
}

// The kernels without dynamic LDS (norms_dense, unit_dense, pairs_dense, the chunk plan, pool_chunks, topk_select,
// topk_merge): `blocks` blocks of `threads` threads; blocks == 0 where memb::gridBlocks found too many.
int launchWithoutLds(const memb::KernelHandle& kernel, uint32_t blocks, uint32_t threads, void** arguments, hipStream_t stream)
{
    return launchBlocks(kernel, blocks, threads, false, 0, arguments, stream);
}
