// The decode kernel table -- every instance of the decode kernel templates, by template arguments -- , what the
// runtime knows about a kernel on a device, and the one helper that launches a kernel with dynamic LDS.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, inside its anonymous namespace, after the device
// code and the context (hip_context.h); see that file for the overview.
#pragma once

// One instance of a kernel template: the function and its name as in the symbol, e.g. decode_trained<false, 2, true>
// (what info() reports as `kernel` and `union_kernel`).
template <typename... A>
struct KernelInstance {
    void (*fn)(A...) = nullptr;
    std::string name;
};

std::string templateArgument(bool value)
{
    return value ? "true" : "false";
}

std::string templateArgument(int value)
{
    return std::to_string(value);
}

template <typename... T>
std::string instanceName(const char* family, T... arguments)
{
    std::string name = family;
    const char* separator = "<";
    ((name += separator + templateArgument(arguments), separator = ", "), ...);
    return name + ">";
}

// The kernel table: every instance of the five decode kernel templates, indexed by its template arguments, empty where
// no instance exists (tests/test_isa.py counts them). Key forms <HAS_SUB, FAST>: <false, true> nibble keys (a one-level
// table), <false, false> and <true, false> byte keys with a one- or a two-level table.
struct KernelTable {
    KernelInstance<TrainedParams> trained[2][5][2];              // decode_trained<HAS_SUB, MODE, FAST>
    KernelInstance<TrainedParams> persistent[2][5][2];           // decode_records_persistent<HAS_SUB, MODE, FAST>: not OUT_INDEX
    KernelInstance<TrainedParams, BatchList> batches[2][3][2];   // decode_trained_batches<HAS_SUB, MODE, FAST>: OUT_SCALAR .. OUT_FLAT
    KernelInstance<UnionParams> unions[2][2][5][2];              // decode_trained_union<HAS_SUB, FAST, COUNT, AVERAGE>: COUNT 2 .. 4
    KernelInstance<UnionParams> split[2][2][2][2];               // decode_union_split<HAS_SUB, FAST, AVERAGE, COMPACT>: COMPACT
                                                                 // with nibble keys only

    KernelTable()
    {
        addKeyForm<false, true>();
        addKeyForm<false, false>();
        addKeyForm<true, false>();
    }

private:
    template <bool HAS_SUB, bool FAST>
    void addKeyForm()
    {
        addMode<HAS_SUB, FAST, OUT_SCALAR>();
        addMode<HAS_SUB, FAST, OUT_VEC4>();
        addMode<HAS_SUB, FAST, OUT_FLAT>();
        addMode<HAS_SUB, FAST, OUT_INDEX>();
        addMode<HAS_SUB, FAST, OUT_KEYS>();
        addUnion<HAS_SUB, FAST, 2, false>();
        addUnion<HAS_SUB, FAST, 2, true>();
        addUnion<HAS_SUB, FAST, 3, false>();
        addUnion<HAS_SUB, FAST, 3, true>();
        addUnion<HAS_SUB, FAST, 4, false>();
        addUnion<HAS_SUB, FAST, 4, true>();
    }

    template <bool HAS_SUB, bool FAST, int MODE>
    void addMode()
    {
        trained[HAS_SUB][MODE][FAST] = {&decode_trained<HAS_SUB, MODE, FAST>, instanceName("decode_trained", HAS_SUB, MODE, FAST)};
        if constexpr (MODE != OUT_INDEX) {
            persistent[HAS_SUB][MODE][FAST] = {
                &decode_records_persistent<HAS_SUB, MODE, FAST>, instanceName("decode_records_persistent", HAS_SUB, MODE, FAST)};
        }
        if constexpr (MODE <= OUT_FLAT) {
            batches[HAS_SUB][MODE][FAST] = {
                &decode_trained_batches<HAS_SUB, MODE, FAST>, instanceName("decode_trained_batches", HAS_SUB, MODE, FAST)};
        }
    }

    template <bool HAS_SUB, bool FAST, int COUNT, bool AVERAGE>
    void addUnion()
    {
        unions[HAS_SUB][FAST][COUNT][AVERAGE] = {
            &decode_trained_union<HAS_SUB, FAST, COUNT, AVERAGE>, instanceName("decode_trained_union", HAS_SUB, FAST, COUNT, AVERAGE)};
        if constexpr (COUNT == 2) {
            split[HAS_SUB][FAST][AVERAGE][false] = {
                &decode_union_split<HAS_SUB, FAST, AVERAGE, false>, instanceName("decode_union_split", HAS_SUB, FAST, AVERAGE, false)};
        }
        if constexpr (COUNT == 2 && FAST) {
            split[HAS_SUB][FAST][AVERAGE][true] = {
                &decode_union_split<HAS_SUB, FAST, AVERAGE, true>, instanceName("decode_union_split", HAS_SUB, FAST, AVERAGE, true)};
        }
    }
};

const KernelTable& kernelTable()
{
    static const KernelTable table;
    return table;
}

// HAS_SUB of a model's lookup kernels: byte keys decode through the 4-byte PACKED table (the index pass reads the 8-byte
// one: buildSegmentIndex), nibble keys have a one-level table.
bool lookupHasSub(const memb_hip_ctx* ctx)
{
    return !ctx->fast && ctx->byteTable.hasSubTables;
}

// decode_trained (persistent: decode_records_persistent) for a model's lookups in this output mode
const KernelInstance<TrainedParams>& lookupKernel(const memb_hip_ctx* ctx, bool persistent, int mode)
{
    return (persistent ? kernelTable().persistent : kernelTable().trained)[lookupHasSub(ctx)][mode][ctx->fast];
}

// What the runtime knows about a kernel on the current device, looked up once per (kernel, device) -- which is also when
// the kernel's dynamic-LDS limit is raised to the 160 KiB of a CU: its registers (-> wavefronts a CU can hold) and, for
// blocks of `threads` (non-zero) with ldsBytes of LDS, how many such blocks a CU holds.
struct KernelFacts {
    int numRegs = 0;
    uint32_t registerWavesPerCu = 32;
    int blocksPerCu = 0;
};

hipError_t kernelFacts(const void* kernel, KernelFacts* out, uint32_t threads = 0, uint32_t ldsBytes = 0)
{
    struct Known {
        const void* kernel;
        int device;
        KernelFacts facts;
        std::vector<std::pair<std::pair<uint32_t, uint32_t>, int>> blocksPerCu;   // (threads, ldsBytes) -> blocks
    };
    static std::mutex mutex;
    static std::vector<Known> known;
    int device = 0;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> lock(mutex);
    auto entry = std::find_if(known.begin(), known.end(), [&](const Known& k) { return k.kernel == kernel && k.device == device; });
    if (entry == known.end()) {
        hipFuncAttributes attributes;
        hipError_t status = hipFuncGetAttributes(&attributes, kernel);
        if (status != hipSuccess) {
            return status;
        }
        KernelFacts facts;
        facts.numRegs = attributes.numRegs;
        // allocation granule 8 registers, 512 per lane per SIMD, 4 SIMDs, at most 8 wavefronts each
        const int allocated = std::max(8, (attributes.numRegs + 7) / 8 * 8);
        facts.registerWavesPerCu = 4u * static_cast<uint32_t>(std::min(8, 512 / allocated));
        status = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (status != hipSuccess) {
            return status;
        }
        entry = known.insert(known.end(), Known{kernel, device, facts, {}});
    }
    *out = entry->facts;
    if (threads) {
        for (const auto& blocks : entry->blocksPerCu) {
            if (blocks.first.first == threads && blocks.first.second == ldsBytes) {
                out->blocksPerCu = blocks.second;
            }
        }
        if (!out->blocksPerCu) {
            hipError_t status = hipOccupancyMaxActiveBlocksPerMultiprocessor(&out->blocksPerCu, kernel, static_cast<int>(threads), ldsBytes);
            if (status != hipSuccess) {
                return status;
            }
            out->blocksPerCu = std::max(out->blocksPerCu, 1);
            entry->blocksPerCu.push_back({{threads, ldsBytes}, out->blocksPerCu});
        }
    }
    return hipSuccess;
}

template <typename... A>
hipError_t kernelFacts(void (*kernel)(A...), KernelFacts* out, uint32_t threads = 0, uint32_t ldsBytes = 0)
{
    return kernelFacts(reinterpret_cast<const void*>(kernel), out, threads, ldsBytes);
}

// Enqueues kernel<<<grid, block, ldsBytes, stream>>>(*arguments[0], ...) -- every kernel with dynamic LDS is launched here,
// the narrow ones of memb_hip_narrow.hip, known by their addresses, included. The first launch of a kernel on a device in a
// thread goes through kernelFacts, which raises its LDS limit; after that the check is one lookup in this thread's own
// table, no lock: the latency of a single word is on this path.
hipError_t launchKernelAddress(const void* kernel, dim3 grid, dim3 block, uint32_t ldsBytes, hipStream_t stream, void** arguments)
{
    static thread_local std::unordered_map<const void*, int> configuredDevice;
    if (!kernel) {
        return hipErrorInvalidDeviceFunction;
    }
    int device = 0;
    (void)hipGetDevice(&device);
    int& configured = configuredDevice.try_emplace(kernel, -1).first->second;
    if (configured != device) {
        KernelFacts facts;
        hipError_t status = kernelFacts(kernel, &facts);
        if (status != hipSuccess) {
            return status;
        }
        configured = device;
    }
    const hipError_t status = hipLaunchKernel(kernel, grid, block, arguments, ldsBytes, stream);
    return status != hipSuccess ? status : hipGetLastError();
}

// The kernels of this translation unit: argument types checked against the kernel's.
template <typename... A>
hipError_t launchKernel(void (*kernel)(A...), dim3 grid, dim3 block, uint32_t ldsBytes, hipStream_t stream, A... args)
{
    void* arguments[] = {&args...};
    return launchKernelAddress(reinterpret_cast<const void*>(kernel), grid, block, ldsBytes, stream, arguments);
}
