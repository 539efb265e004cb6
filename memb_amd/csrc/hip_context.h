// The context behind the C ABI's opaque pointer: its measurement / test switches, device allocation and
// teardown, the current-device guards of the entry points.
//
// Host code of libmemb_hip.so. Included by memb_hip.hip only, at global scope (memb_hip_ctx and Switches are
// global types; the rest is in an anonymous namespace of its own), after fail and HIP_TRY; see that file for
// the overview.
#pragma once

// ---------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------

// Measurement / test switches: options of a live context (memb_hip_ctx_set_option) and a few environment variables read once
// when a context is created (tools/perf/README.md has the list).
struct Switches {
    uint32_t waves = 0;            // MEMB_HIP_WAVES / option waves_per_block: force the wavefronts per block (0 = choose)
    uint32_t debugFlags = 0;       // MEMB_HIP_DEBUG, builds with -DMEMB_HIP_MEASURE only (hip_trained_kernels.h: measureFlags)
    uint32_t persistent = 1;       // option persistent: 1 = the kernel by batch size (planTrained); 0 = one tile per wavefront
                                   // always, 2 = decode_records_persistent whenever the layout allows (tests, measurements)
    uint32_t unionSplit = 1;       // option union_split: decode_union_split for pairs of models with row records:
                                   // 0 = never, 1 = whenever the pair qualifies
    uint32_t unionFused = 1;       // option union_fused (of the FIRST model's context): 0 = no union kernel, the caller launches per model (tests)
    uint32_t tilesPerWave = 0;     // option tiles_per_wave: tiles a wavefront of the one-tile kernels decodes one after the
                                   // other: 0 = by rule (oneTileSteps), K = K (measurements)
    uint32_t fineLanes = 0;        // option fine_lanes: the finer index of small batches: 0 = by rule (planTrained), 1 = never,
                                   // 2 = every batch of a model that has one (tests, measurements)
    uint32_t ldsPad = 0;           // option lds_pad, builds with -DMEMB_HIP_MEASURE only: unused LDS bytes added to every block of
                                   // decode_trained (fewer resident wavefronts per CU from the same code: round 5's residency table, profiles/r05_experiments.txt)
    bool hostExpand = true;        // option host_expand: centroid indices over PCIe for host buffers
    uint32_t sliceWords = ~0u;     // MEMB_HIP_SLICE_WORDS: staging slice (tests)
    uint32_t copyChunkRows = 0;    // MEMB_HIP_COPY_CHUNK_ROWS: rows per ring chunk (tests; 0 = by size)
    uint32_t hostStreaming = 1;    // MEMB_HIP_HOST_STREAMING: non-temporal stores when host threads expand results: 0 = never,
                                   // 1 = results of 64 MB and more (default), 2 = always (tests)
    uint32_t copyThreads = 16;     // MEMB_HIP_COPY_THREADS
    bool verbose = false;          // MEMB_HIP_VERBOSE
};

struct memb_hip_ctx {
    Switches switches;
    int device = 0;
    uint32_t storage = 0;
    uint32_t dim = 0;
    uint64_t nRows = 0;
    uint64_t deviceBytes = 0;
    hipStream_t stream = nullptr;
    std::vector<void*> allocations;

    // trained
    uint4* streams = nullptr;            // re-packed bitstreams
    uint32_t* streamStarts = nullptr;    // [nRows + 1]
    uint32_t* table = nullptr;
    float* codebook = nullptr;
    bool fast = false;                   // <= 16 centroids, codes <= 8 bits, one-level table
    memb::DecodeTable hostTable;         // 8-byte device entries: nibble keys, the index pass, the union kernel
    uint32_t tableDwords = 0;
    // byte keys (!fast): the table of the PACKED kernels -- 4-byte entries, a first level that covers
    // the longest code where 32 KiB hold it (hip_trained_kernels.h: decodeSegment)
    memb::DecodeTable byteTable;
    std::vector<memb::CodeInfo> codeLengths;   // kept to rebuild byteTable narrower when LDS is short
    uint32_t* table32 = nullptr;
    // nibble-key models only: the codebook in its BYTE-key form as well (256 plain centroids) -- with table32, which every
    // model has, a union with a byte-key model can then run as one kernel
    float* codebookBytes = nullptr;
    uint32_t maxStreamBytes = 0;
    uint32_t slotDwords = 0;
    uint16_t* segmentIndex = nullptr;    // [nRows][lanesPerWord - 1]; uint32_t entries when indexWide
    bool indexWide = false;              // some row is longer than 65535 bits
    uint32_t* rowMeta = nullptr;         // 16-byte records {start, 13-bit segment offsets}: what lookups read (or null)
    // The finer index of small batches (row-record models): [nRows][fineLanes - 1] uint16_t offsets at which symbols
    // fineSymbols, 2 fineSymbols, ... of each row start -- about sixteen lanes decode a word side by side where the records
    // have offsets for eight, which shortens the one chain of dependent LDS lookups a small batch has nothing to hide behind
    uint16_t* fineIndex = nullptr;
    uint32_t fineLanes = 0;
    uint32_t fineSymbols = 0;
    uint32_t recordPieces = 0;           // non-zero: row records (TrainedParams::recordPieces); `streams` is that array
    const char* unionKernel = "";        // what the last union launch with this context as its first model ran (kernelTable)
    const char* pooledUnionKernel = "";  // ... and the last pooled union launch (memb_hip_pool_union_kernel_name)
    uint32_t lanesPerWord = 1;           // G: lanes that share one word
    uint32_t segmentSymbols = 0;         // S: symbols per lane, multiple of 4
    std::vector<uint32_t> streamBytes;   // per row, host side (reporting only)
    uint32_t ldsLimit = 0;
    uint32_t cuCount = 0;

    // uniform / full
    uint4* uniformRecords = nullptr;     // row records: {min, max, 0, 0} + the weights, regionPieces 16-byte pieces per row
    uint32_t regionPieces = 0;
    float levels = 0.f;
    float* fullValues = nullptr;

    // word -> row on the device (memb_hip_ctx_stage_words; hip_words.h): the keys and a hash table over them
    uint8_t* wordKeyBytes = nullptr;
    void* wordSlots = nullptr;           // WordSlot [wordSlotMask + 1]; non-null = staged
    uint32_t wordSlotMask = 0;
    uint32_t wordIndexKeys = 0;
    uint64_t wordIndexBytes = 0;

    // staging for the host-buffer entry point
    uint32_t* stagedRows = nullptr;
    float* stagedOut = nullptr;   // fp32 rows, or rows of centroid indices (trained: see decodeRowsAsKeys)
    size_t stagedCapacity = 0;    // words
    size_t stagedRowBytes = 0;
    std::vector<float> hostCodebook;   // the device codebook's host copy (256 centroids or 256 pairs)
    uint32_t* hostRowsPinned = nullptr;   // memb_hip_decode_words: the row ids the device looked up, for the host threads
    size_t hostRowsCapacity = 0;
    // What the last very large batch looked like to the kernel that decoded it (hip_trained_kernels.h: noteBatchOrder):
    // one word of pinned host memory, 1 = rows mostly consecutive, 0 = no particular order, ORDER_UNKNOWN before the first
    uint32_t* orderSeen = nullptr;
    uint32_t* orderSeenDevice = nullptr;
    // small batches: pinned host memory the kernel reads row ids from and writes rows to directly
    void* smallHost = nullptr;
    void* smallDevice = nullptr;
    bool smallUnavailable = false;
    // pinned ring the DMA engine fills while host threads copy earlier chunks to the caller's rows
    static constexpr int RING = 4;
    void* ring[RING] = {};
    hipEvent_t ringEvents[RING] = {};
    bool ringUnavailable = false;
    std::unique_ptr<memb::WorkerPool> copyPool;   // the host threads that empty the ring
    std::mutex mutex;
};

namespace {

constexpr uint32_t ORDER_UNKNOWN = 2;   // memb_hip_ctx::orderSeen before any very large batch

uint32_t envUint(const char* name, uint32_t fallback)
{
    const char* text = std::getenv(name);
    if (!text || !*text) {
        return fallback;
    }
    return static_cast<uint32_t>(std::strtoul(text, nullptr, 10));
}

template <typename T>
int deviceAlloc(memb_hip_ctx* ctx, T** pointer, size_t bytes)
{
    void* raw = nullptr;
    HIP_TRY(hipMalloc(&raw, std::max<size_t>(bytes, 16)));
    ctx->allocations.push_back(raw);
    ctx->deviceBytes += std::max<size_t>(bytes, 16);
    *pointer = static_cast<T*>(raw);
    return MEMB_HIP_OK;
}

// Gives an allocation of deviceAlloc back before the context goes (optional structures whose build failed).
template <typename T>
void deviceRelease(memb_hip_ctx* ctx, T** pointer, size_t bytes)
{
    if (!*pointer) {
        return;
    }
    auto found = std::find(ctx->allocations.begin(), ctx->allocations.end(), static_cast<void*>(*pointer));
    if (found != ctx->allocations.end()) {
        ctx->allocations.erase(found);
        ctx->deviceBytes -= std::max<size_t>(bytes, 16);
    }
    (void)hipFree(*pointer);
    *pointer = nullptr;
}

// Host -> device copy of a (possibly file-mapped) range. Pinning the mapped
// pages first lets the copy run at the PCIe rate; registration of a read-only
// mapping can be refused, in which case the plain copy is used.
int copyToDevice(void* dst, const void* src, size_t bytes)
{
    if (!bytes) {
        return MEMB_HIP_OK;
    }
    bool registered = false;
    if (bytes >= (8u << 20)) {
        hipError_t status = hipHostRegister(const_cast<void*>(src), bytes, hipHostRegisterReadOnly);
        if (status == hipSuccess) {
            registered = true;
        } else {
            (void)hipGetLastError();
        }
    }
    hipError_t status = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    if (registered) {
        (void)hipHostUnregister(const_cast<void*>(src));
    }
    if (status != hipSuccess) {
        return fail(MEMB_HIP_ERR_DEVICE, std::string("hipMemcpy to device: ") + hipGetErrorString(status));
    }
    return MEMB_HIP_OK;
}

// Makes the context's device current for the duration of an entry point and puts the caller's
// device back afterwards (the calling thread may belong to PyTorch, whose current device must not
// change under it).
class DeviceScope {
public:
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&previous_) != hipSuccess) {
            (void)hipGetLastError();
            previous_ = -1;
        }
        status_ = previous_ == device ? hipSuccess : hipSetDevice(device);
        changed_ = status_ == hipSuccess && previous_ != device;
    }
    ~DeviceScope()
    {
        if (changed_ && previous_ >= 0) {
            (void)hipSetDevice(previous_);
        }
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    hipError_t status() const { return status_; }

private:
    int previous_ = -1;
    hipError_t status_ = hipSuccess;
    bool changed_ = false;
};

// Puts the calling thread's current device back when it goes out of scope (context creation and
// destruction switch devices as they go).
class DeviceRestore {
public:
    DeviceRestore()
    {
        if (hipGetDevice(&previous_) != hipSuccess) {
            (void)hipGetLastError();
            previous_ = -1;
        }
    }
    ~DeviceRestore()
    {
        if (previous_ >= 0) {
            (void)hipSetDevice(previous_);
        }
    }
    DeviceRestore(const DeviceRestore&) = delete;
    DeviceRestore& operator=(const DeviceRestore&) = delete;

private:
    int previous_ = -1;
};

// (callers hold a DeviceRestore: the context's device stays current for the staging that follows)
int openDevice(memb_hip_ctx* ctx, int device)
{
    int count = 0;
    hipError_t status = hipGetDeviceCount(&count);
    if (status != hipSuccess || count == 0) {
        (void)hipGetLastError();
        return fail(MEMB_HIP_ERR_DEVICE, "no HIP device available");
    }
    if (device < 0 || device >= count) {
        return fail(MEMB_HIP_ERR_INVALID, "device index out of range");
    }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t properties;
    HIP_TRY(hipGetDeviceProperties(&properties, device));
    ctx->device = device;
    ctx->cuCount = properties.multiProcessorCount;
    ctx->ldsLimit = static_cast<uint32_t>(std::min<size_t>(properties.sharedMemPerBlock, 160 * 1024));
    if (properties.maxSharedMemoryPerMultiProcessor >= 160 * 1024) {
        ctx->ldsLimit = 160 * 1024;
    }
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    // the word the kernels of very large batches leave about their rows' order (noteBatchOrder); a context that cannot have
    // it runs the block size of key order whatever comes
    void* seen = nullptr;
    if (hipHostMalloc(&seen, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
        void* device = nullptr;
        if (hipHostGetDevicePointer(&device, seen, 0) == hipSuccess) {
            ctx->orderSeen = static_cast<uint32_t*>(seen);
            ctx->orderSeenDevice = static_cast<uint32_t*>(device);
            *ctx->orderSeen = ORDER_UNKNOWN;
        } else {
            (void)hipHostFree(seen);
        }
    }
    (void)hipGetLastError();
    return MEMB_HIP_OK;
}

Switches readSwitches()
{
    Switches switches;
    switches.waves = envUint("MEMB_HIP_WAVES", 0);   // (also an option; as a variable it is known when the tables are sized: chooseLanes)
#ifdef MEMB_HIP_MEASURE
    switches.debugFlags = envUint("MEMB_HIP_DEBUG", 0);
#endif
    switches.sliceWords = envUint("MEMB_HIP_SLICE_WORDS", ~0u);
    switches.copyChunkRows = envUint("MEMB_HIP_COPY_CHUNK_ROWS", 0);
    switches.copyThreads = std::min<uint32_t>(envUint("MEMB_HIP_COPY_THREADS", 16), 64);
    switches.hostStreaming = std::min<uint32_t>(envUint("MEMB_HIP_HOST_STREAMING", 1), 2);
    switches.verbose = envUint("MEMB_HIP_VERBOSE", 0) != 0;
    return switches;
}

void destroy(memb_hip_ctx* ctx)
{
    if (!ctx) {
        return;
    }
    DeviceRestore restore;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
    }
    for (void* allocation : ctx->allocations) {
        (void)hipFree(allocation);
    }
    if (ctx->orderSeen) {
        (void)hipHostFree(ctx->orderSeen);
    }
    if (ctx->smallHost) {
        (void)hipHostFree(ctx->smallHost);
    }
    if (ctx->hostRowsPinned) {
        (void)hipHostFree(ctx->hostRowsPinned);
    }
    for (int i = 0; i < memb_hip_ctx::RING; ++i) {
        if (ctx->ring[i]) {
            (void)hipHostFree(ctx->ring[i]);
        }
        if (ctx->ringEvents[i]) {
            (void)hipEventDestroy(ctx->ringEvents[i]);
        }
    }
    if (ctx->stagedRows) {
        (void)hipFree(ctx->stagedRows);
    }
    if (ctx->stagedOut) {
        (void)hipFree(ctx->stagedOut);
    }
    if (ctx->stream) {
        (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

struct ContextGuard {
    explicit ContextGuard(memb_hip_ctx* ctx): ctx_(ctx) {}
    ~ContextGuard() { destroy(ctx_); }
    ContextGuard(const ContextGuard&) = delete;
    ContextGuard& operator=(const ContextGuard&) = delete;
    memb_hip_ctx* release()
    {
        memb_hip_ctx* ctx = ctx_;
        ctx_ = nullptr;
        return ctx;
    }

private:
    memb_hip_ctx* ctx_;
};

}  // namespace
