// pybind11 module `_memb`: the reference's binding surface
// (python/memb_bindings.cpp:11-72) -- Reader(filename, num_threads) with
// dim / word_embedding / batch_embedding / keys, Builder(dim, storage, bits)
// with add_word / save, available_compression_strategies() -- plus additions
// for device-resident results and strided (concatenated) outputs.
#include "builder.h"
#include "reader.h"
#include "compression_strategy.h"
#include "codec.h"
#include "../../include/memb_hip_pooled_union.h"
#include "../../include/memb_hip_norms.h"
#include "../../include/memb_hip_pairs.h"
#include "../../include/memb_hip_bag_pairs.h"
#include "../../include/memb_hip_queries.h"
#include "../../include/memb_hip_query_matrix.h"
#include "hip_query_matrix.h"
#include "../../include/memb_hip_query_topk.h"
#include "../../include/memb_hip_analogies.h"
#include "hip_query_topk.h"
#include "../../include/memb_hip_query_bags.h"
#include "hip_query_bags.h"

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <pybind11/numpy.h>

#include <sys/mman.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

namespace py = pybind11;

namespace {

std::shared_ptr<memb::Reader> makeReader(
    const std::string& filename, size_t numThreads, int device, size_t maxDirectDecodeBits)
{
    if (maxDirectDecodeBits == 0) {
        return std::make_shared<memb::Reader>(filename, numThreads, device);
    }
    // the reference's test hook: a trained strategy with a short first-level
    // table, injected through the second Reader constructor (src/tests.cpp:76-88)
    return std::make_shared<memb::Reader>(
        filename, std::make_shared<memb::TrainedCompressionStrategy>(maxDirectDecodeBits), numThreads, device);
}

// UTF-8 pointers of a sequence of str, without copying the words (pybind11's
// vector<string> caster copies every one). The pointers stay valid while the
// sequence is alive; a word with an embedded NUL ends there, as it does for the
// reference's strcmp.
// A large result array is filled once, right after numpy allocated it: ask for
// transparent huge pages on it (hosts run THP in "madvise" mode), so that filling
// 2.6 GB takes ~1300 page faults instead of ~640,000. Advice only; ignored where
// THP is off.
void adviseHugePages(void* data, size_t bytes)
{
    const size_t huge = size_t(2) << 20;
    if (bytes < 16 * huge) {
        return;
    }
    const uintptr_t first = (reinterpret_cast<uintptr_t>(data) + huge - 1) / huge * huge;
    const uintptr_t last = (reinterpret_cast<uintptr_t>(data) + bytes) / huge * huge;
    if (last > first) {
        (void)::madvise(reinterpret_cast<void*>(first), last - first, MADV_HUGEPAGE);
    }
}

struct WordPointers {
    py::object fast;   // keeps the items alive
    std::vector<const char*> pointers;

    explicit WordPointers(const py::handle& words)
    {
        fast = py::reinterpret_steal<py::object>(PySequence_Fast(words.ptr(), "expected a list of str"));
        if (!fast) {
            throw py::error_already_set();
        }
        const Py_ssize_t count = PySequence_Fast_GET_SIZE(fast.ptr());
        PyObject** items = PySequence_Fast_ITEMS(fast.ptr());
        pointers.resize(static_cast<size_t>(count));
        for (Py_ssize_t i = 0; i < count; ++i) {
            if (!PyUnicode_Check(items[i])) {
                throw py::type_error("words must be str");
            }
            const char* text = PyUnicode_AsUTF8(items[i]);
            if (!text) {
                throw py::error_already_set();
            }
            pointers[static_cast<size_t>(i)] = text;
        }
    }

    size_t size() const { return pointers.size(); }
    const char* const* data() const { return pointers.data(); }
};

// Every binding that fills or looks up through a WordBatch holds its claim for the whole call: a batch shared by two calls
// in flight (one's begin would reset, even free, what the other's threads and lookups still use) is a RuntimeError.
// Taken while the GIL is held and never waited for.
struct BatchClaim {
    memb::WordBatch& batch;

    explicit BatchClaim(memb::WordBatch& claimed): batch(claimed)
    {
        if (!batch.tryClaim()) {
            throw std::runtime_error("word batch is in use by another call");
        }
    }
    ~BatchClaim() { batch.releaseClaim(); }
    BatchClaim(const BatchClaim&) = delete;
    BatchClaim& operator=(const BatchClaim&) = delete;
};

// packed_to_rows_device / _packed_fill_seconds: one buffer of bytes and n + 1 uint32 offsets, as plain memory
struct PackedWords {
    const uint8_t* data;
    size_t dataBytes;
    const uint32_t* offsets;
    size_t count;
};

PackedWords packedWords(const py::buffer_info& blob, const py::array& offsets)
{
    if (blob.ndim != 1 || blob.itemsize != 1 || (blob.size > 1 && blob.strides[0] != 1)) {
        throw py::type_error("bytes must be a contiguous one-dimensional buffer of bytes");
    }
    if (!py::isinstance<py::array_t<uint32_t>>(offsets) || offsets.ndim() != 1 || offsets.shape(0) < 1 ||
        !(offsets.flags() & py::array::c_style)) {
        throw py::type_error("offsets must be a contiguous numpy.uint32 array of n + 1 entries");
    }
    return PackedWords{
        static_cast<const uint8_t*>(blob.ptr), static_cast<size_t>(blob.size), static_cast<const uint32_t*>(offsets.data()),
        static_cast<size_t>(offsets.shape(0)) - 1};
}

// A list of str into a word batch on the device (memb::WordBatch, include/memb_hip.h: memb_hip_words_plan) -- the part
// of a device word search that is host work, and at 2.2 M words the longest part of a lookup, so every word is touched
// ONCE: pooled threads read the str objects and write their UTF-8 bytes (up to the first NUL, where the reference's
// strcmp stops) straight into the batch's pinned job regions, which the lookup kernel reads over PCIe. The calling
// thread holds the GIL throughout, so no Python code runs meanwhile; the pool reads the objects' memory only: a compact
// ASCII str (nearly every token) has its bytes behind its header, a str with a cached UTF-8 form has pointer and length
// in its header. A job that meets anything else (non-ASCII without the cache, not a str at all) is redone after the
// calling thread has gone over its words through the API, which may allocate and raise. The walk is a cache miss per
// word and little else: every thread prefetches the objects a few words ahead.
// onChunk(firstWord, words) is called on the calling thread for consecutive runs of finished jobs, in order, while
// later jobs are still being filled: the lookups of a run overlap the filling of the next.
// The pool threads read str objects WITHOUT the GIL, relying on the calling thread's hold of it to keep the list and its
// strings from changing, and on the object layout of the CPython versions this was written against. Where either does
// not hold -- a free-threaded build, another interpreter, a CPython newer than the layouts known here -- every word goes
// through PyUnicode_AsUTF8AndSize on the calling thread instead (fillJobWithApi).
#if defined(Py_GIL_DISABLED) || defined(PYPY_VERSION) || defined(GRAALVM_PYTHON) || PY_VERSION_HEX < 0x03080000 || PY_VERSION_HEX >= 0x030E0000
constexpr bool DIRECT_STR_ACCESS = false;
#else
constexpr bool DIRECT_STR_ACCESS = true;
static_assert(sizeof(PyASCIIObject) <= sizeof(PyCompactUnicodeObject), "str layout: ASCII header inside the compact one");
#endif

struct WordFiller {
    static size_t poolThreads()
    {
        const char* text = std::getenv("MEMB_PACK_THREADS");
        const unsigned wanted = text && *text ? static_cast<unsigned>(std::strtoul(text, nullptr, 10)) : 64u;
        return std::max(2u, std::min(std::min(wanted, 128u), std::thread::hardware_concurrency()));
    }

    // Threads for a batch of `count` words: the walk is a cache miss per word, so large batches want many (2.2 M shuffled
    // words: 2.1 / 1.5 / 0.87 ms with 16 / 32 / 64 threads) and small ones few (100 000 words: 0.068 / 0.079 / 0.109 ms):
    // one per 32 768 words, at least sixteen (eight: 100 000 words 0.16-0.22 ms against 0.14-0.15), at most the pool
    // (MEMB_PACK_THREADS, default 64).
    static size_t threadsFor(size_t count)
    {
        return std::min<size_t>(pool().size(), std::max<size_t>(16, count / 32768));
    }

    static memb::WorkerPool& pool()
    {
        static memb::WorkerPool workers(poolThreads() - 1);
        return workers;
    }

    // The pool serves one batch at a time (start .. wait): whoever fills through it -- this filler or PackedFiller, which
    // runs without the GIL -- holds this mutex meanwhile, and fills on its own thread when it cannot get it.
    static std::mutex& poolMutex()
    {
        static std::mutex mutex;
        return mutex;
    }

    enum JobState : int { FILLED = 0, NEEDS_API = 1, TOO_LONG = 2 };

    // One job of the plan; returns its state (and, for TOO_LONG, the bytes it needs in *needed).
    static JobState fillJob(const memb_hip_words_plan& plan, PyObject** items, size_t job, uint64_t* needed)
    {
        constexpr size_t AHEAD = 12;
        const size_t first = job * plan.job_words, last = std::min(plan.n, first + plan.job_words);
        uint32_t* offsets = plan.offsets + job * (plan.job_words + 1);
        const uint64_t base = uint64_t(job) * plan.job_bytes;
        uint64_t at = 0;
        bool fits = true;
        for (size_t i = first; i < last; ++i) {
            if (i + AHEAD < last) {
                __builtin_prefetch(items[i + AHEAD]);
                __builtin_prefetch(reinterpret_cast<const char*>(items[i + AHEAD]) + 64);
            }
            PyObject* item = items[i];
            const char* text = nullptr;
            Py_ssize_t size = 0;
            bool ready = PyUnicode_Check(item);
#if PY_VERSION_HEX < 0x030C0000
            ready = ready && PyUnicode_IS_READY(item);
#endif
            if (ready && PyUnicode_IS_COMPACT_ASCII(item)) {
                text = reinterpret_cast<const char*>(reinterpret_cast<PyASCIIObject*>(item) + 1);
                size = PyUnicode_GET_LENGTH(item);
            } else if (ready && reinterpret_cast<PyCompactUnicodeObject*>(item)->utf8) {
                // (every str that is not compact ASCII -- compact or not -- begins with a PyCompactUnicodeObject, whose
                // utf8 / utf8_length hold the cached UTF-8 form once PyUnicode_AsUTF8AndSize has been asked for it)
                text = reinterpret_cast<PyCompactUnicodeObject*>(item)->utf8;
                size = reinterpret_cast<PyCompactUnicodeObject*>(item)->utf8_length;
            }
            if (!text || size < 0) {
                return NEEDS_API;
            }
            const size_t length = ::strnlen(text, static_cast<size_t>(size));
            if (fits && at + length <= plan.job_bytes) {
                offsets[i - first] = static_cast<uint32_t>(base + at);
                std::memcpy(plan.bytes + base + at, text, length);
            } else {
                fits = false;
            }
            at += length;
        }
        if (!fits) {
            *needed = at;
            return TOO_LONG;
        }
        offsets[last - first] = static_cast<uint32_t>(base + at);
        return FILLED;
    }

    // The same job through the C API alone, on the calling thread (GIL held): interpreters whose str layout is not known here.
    static JobState fillJobWithApi(const memb_hip_words_plan& plan, PyObject** items, size_t job, uint64_t* needed)
    {
        const size_t first = job * plan.job_words, last = std::min(plan.n, first + plan.job_words);
        uint32_t* offsets = plan.offsets + job * (plan.job_words + 1);
        const uint64_t base = uint64_t(job) * plan.job_bytes;
        uint64_t at = 0;
        bool fits = true;
        for (size_t i = first; i < last; ++i) {
            if (!PyUnicode_Check(items[i])) {
                throw py::type_error("words must be str");
            }
            Py_ssize_t size = 0;
            const char* text = PyUnicode_AsUTF8AndSize(items[i], &size);
            if (!text) {
                throw py::error_already_set();
            }
            const size_t length = ::strnlen(text, static_cast<size_t>(size));
            if (fits && at + length <= plan.job_bytes) {
                offsets[i - first] = static_cast<uint32_t>(base + at);
                std::memcpy(plan.bytes + base + at, text, length);
            } else {
                fits = false;
            }
            at += length;
        }
        if (!fits) {
            *needed = at;
            return TOO_LONG;
        }
        offsets[last - first] = static_cast<uint32_t>(base + at);
        return FILLED;
    }

    // The words a job could not read without the API: the calling thread (GIL held) makes their UTF-8 form
    // available, or raises for what is not a str.
    static void prepareWithApi(PyObject** items, size_t first, size_t last)
    {
        for (size_t i = first; i < last; ++i) {
            if (!PyUnicode_Check(items[i])) {
                throw py::type_error("words must be str");
            }
            Py_ssize_t size = 0;
            if (!PyUnicode_AsUTF8AndSize(items[i], &size)) {   // (caches the UTF-8 form in the object)
                throw py::error_already_set();
            }
        }
    }

    // expected: the number of words the caller has room for (rows it writes); a list whose size differs from it when the
    // words are read is refused. SIZE_MAX: any size.
    template <typename OnChunk>
    static size_t fill(memb::WordBatch& batch, const py::handle& words, OnChunk onChunk, size_t expected = SIZE_MAX)
    {
        py::object fast = py::reinterpret_steal<py::object>(PySequence_Fast(words.ptr(), "expected a list of str"));
        if (!fast) {
            throw py::error_already_set();
        }
        size_t bytesPerWord = 0;
        for (int attempt = 0; attempt < 48; ++attempt) {
            size_t count = static_cast<size_t>(PySequence_Fast_GET_SIZE(fast.ptr()));
            memb_hip_words_plan plan;
            {
                py::gil_scoped_release release;   // (begin waits for the lookups that still read the previous batch)
                plan = batch.begin(count, bytesPerWord);
            }
            // Other Python threads ran while the GIL was released: a list may have been resized meanwhile (its item array
            // moved, its size changed). Read both again; a batch begun for another size starts over.
            const size_t now = static_cast<size_t>(PySequence_Fast_GET_SIZE(fast.ptr()));
            if (expected != SIZE_MAX && now != expected) {
                throw std::runtime_error("the list of words changed size during the call");
            }
            if (now != count) {
                continue;
            }
            PyObject** items = PySequence_Fast_ITEMS(fast.ptr());
            std::vector<int> state(plan.jobs, FILLED);
            std::vector<uint64_t> needed(plan.jobs, 0);
            if (count == 0) {
                plan.offsets[0] = 0;
                batch.commit();
                return 0;
            }
            std::unique_lock<std::mutex> lock(WordFiller::poolMutex(), std::try_to_lock);
            const bool pooled = DIRECT_STR_ACCESS && count >= 8192 && lock.owns_lock();
            bool clean = true;
            if (!pooled) {
                for (size_t job = 0; job < plan.jobs; ++job) {
                    state[job] = DIRECT_STR_ACCESS ? fillJob(plan, items, job, &needed[job]) : fillJobWithApi(plan, items, job, &needed[job]);
                    clean = clean && state[job] == FILLED;
                }
                if (clean) {
                    onChunk(size_t(0), count);
                }
            } else {
                // chunks of consecutive jobs; the pool hands jobs out in order, so chunks complete roughly in order
                // (at most eight, of at least 65 536 words: a lookup launch is a few microseconds of this thread's time)
                const size_t chunkJobs = std::max((plan.jobs + 7) / 8, (size_t(65536) + plan.job_words - 1) / plan.job_words);
                const size_t chunks = (plan.jobs + chunkJobs - 1) / chunkJobs;
                std::vector<std::atomic<size_t>> done(chunks);
                for (auto& counter : done) {
                    counter.store(0, std::memory_order_relaxed);
                }
                pool().start(plan.jobs, [&](size_t job) {
                    state[job] = fillJob(plan, items, job, &needed[job]);
                    done[job / chunkJobs].fetch_add(1, std::memory_order_release);
                }, threadsFor(count));
                std::exception_ptr failure;
                for (size_t chunk = 0; chunk < chunks; ++chunk) {
                    const size_t firstJob = chunk * chunkJobs, lastJob = std::min(plan.jobs, firstJob + chunkJobs);
                    // (the GIL stays with this thread while the pool reads the list and its strings: it is what keeps them
                    // from changing under the pool -- as the reference holds it for a whole batch_embedding call,
                    // python/memb_bindings.cpp:54-63. A 2.2 M-word fill is about a millisecond)
                    while (done[chunk].load(std::memory_order_acquire) < lastJob - firstJob) {
                        std::this_thread::yield();
                    }
                    for (size_t job = firstJob; job < lastJob; ++job) {
                        clean = clean && state[job] == FILLED;
                    }
                    if (clean && !failure) {
                        try {
                            const size_t firstWord = firstJob * plan.job_words;
                            onChunk(firstWord, std::min(count, lastJob * plan.job_words) - firstWord);
                        } catch (...) {
                            failure = std::current_exception();   // (the pool still works on this thread's stack)
                        }
                    }
                }
                pool().wait();
                if (failure) {
                    std::rethrow_exception(failure);
                }
            }
            if (clean) {
                batch.commit();
                return count;
            }
            // the rare paths: make the words of the jobs that need it readable, size the regions for the longest job
            uint64_t longest = 0;
            for (size_t job = 0; job < plan.jobs; ++job) {
                if (state[job] == NEEDS_API) {
                    prepareWithApi(items, job * plan.job_words, std::min(count, (job + 1) * plan.job_words));
                }
                longest = std::max(longest, needed[job]);
            }
            if (longest) {
                bytesPerWord = std::max<size_t>(
                    2 * (plan.job_bytes / plan.job_words), (longest + plan.job_words - 1) / plan.job_words * 5 / 4 + 1);
            } else {
                bytesPerWord = plan.job_bytes / plan.job_words;
            }
        }
        throw std::runtime_error("internal error: the word batch does not converge");
    }
};

// Words that are packed already -- a tokenizer's output: one blob of UTF-8 bytes and n + 1 ascending offsets -- into a word
// batch's pinned job regions: per job one memcpy and a run of rebased offsets, on the pool, no str object in sight (the
// walk over 2.2 M str objects is a cache miss per word: 0.8-1.2 ms; this is 0.1-0.2 ms of memcpy). The caller holds no GIL.
// onChunk as in WordFiller::fill. Offsets that are not ascending or leave the blob are refused before anything is written.
struct PackedFiller {
    template <typename OnChunk>
    static size_t fill(memb::WordBatch& batch, const uint8_t* blob, size_t blobBytes, const uint32_t* offsets, size_t count, OnChunk onChunk)
    {
        if (count == 0) {
            const memb_hip_words_plan plan = batch.begin(0, 0);
            plan.offsets[0] = 0;
            batch.commit();
            return 0;
        }
        if (offsets[count] > blobBytes) {
            throw std::invalid_argument("offsets[n] lies beyond the end of the bytes");
        }
        size_t bytesPerWord = std::max<size_t>(1, (size_t(offsets[count]) - offsets[0] + count - 1) / count + 1);
        for (int attempt = 0; attempt < 3; ++attempt) {
            const memb_hip_words_plan plan = batch.begin(count, bytesPerWord);
            // the longest job decides the region size (jobs are runs of job_words consecutive words)
            uint64_t longest = 0;
            for (size_t job = 0; job < plan.jobs; ++job) {
                const size_t first = job * plan.job_words, last = std::min(count, first + plan.job_words);
                if (offsets[last] < offsets[first]) {
                    throw std::invalid_argument("offsets must ascend");
                }
                longest = std::max<uint64_t>(longest, offsets[last] - offsets[first]);
            }
            if (longest > plan.job_bytes) {
                bytesPerWord = (longest + plan.job_words - 1) / plan.job_words + 1;
                continue;
            }
            std::atomic<bool> descending{false};
            auto fillJob = [&](size_t job) {
                const size_t first = job * plan.job_words, last = std::min(count, first + plan.job_words);
                uint32_t* target = plan.offsets + job * (plan.job_words + 1);
                const uint32_t base = static_cast<uint32_t>(job * plan.job_bytes);
                const uint32_t origin = offsets[first];
                bool ordered = true;
                for (size_t i = first; i <= last; ++i) {
                    ordered = ordered && (i == first || offsets[i] >= offsets[i - 1]);
                    target[i - first] = base + (offsets[i] - origin);
                }
                if (!ordered) {
                    descending.store(true, std::memory_order_relaxed);
                    return;
                }
                std::memcpy(plan.bytes + size_t(job) * plan.job_bytes, blob + origin, offsets[last] - origin);
            };
            std::unique_lock<std::mutex> lock(WordFiller::poolMutex(), std::try_to_lock);
            if (count < 8192 || !lock.owns_lock()) {
                for (size_t job = 0; job < plan.jobs; ++job) {
                    fillJob(job);
                }
                if (!descending.load()) {
                    onChunk(size_t(0), count);
                }
            } else {
                // Runs of jobs whose lookups are launched as they finish: a sixteenth of the batch, then up to a quarter, a half,
                // the rest. The lookup reads the words over PCIe (2.2 M words: 0.68 ms at 51 GB/s) and every launch costs it a
                // ramp of ~15 us, so few launches, the first one early (round 6, tools/perf/r6/packed.sh: eight equal runs
                // 0.87-0.98 ms, sixteen 0.92-0.98, thirty-two 1.07-1.12, sixty-four 1.29-1.36).
                std::vector<size_t> ends;
                for (size_t fraction : {16u, 4u, 2u, 1u}) {
                    const size_t end = fraction == 1 ? plan.jobs : std::max<size_t>(1, plan.jobs / fraction);
                    if ((ends.empty() || end > ends.back()) && (fraction == 1 || end * plan.job_words >= 65536)) {
                        ends.push_back(end);
                    }
                }
                const size_t chunks = ends.size();
                auto chunkOf = [&](size_t job) {
                    size_t chunk = 0;
                    while (job >= ends[chunk]) {
                        ++chunk;
                    }
                    return chunk;
                };
                std::vector<std::atomic<size_t>> done(chunks);
                for (auto& counter : done) {
                    counter.store(0, std::memory_order_relaxed);
                }
                WordFiller::pool().start(plan.jobs, [&](size_t job) {
                    fillJob(job);
                    done[chunkOf(job)].fetch_add(1, std::memory_order_release);
                }, WordFiller::threadsFor(count));
                std::exception_ptr failure;
                for (size_t chunk = 0; chunk < chunks; ++chunk) {
                    const size_t firstJob = chunk ? ends[chunk - 1] : 0, lastJob = ends[chunk];
                    while (done[chunk].load(std::memory_order_acquire) < lastJob - firstJob) {
                        std::this_thread::yield();
                    }
                    if (!failure && !descending.load(std::memory_order_relaxed)) {
                        try {
                            const size_t firstWord = firstJob * plan.job_words;
                            onChunk(firstWord, std::min(count, lastJob * plan.job_words) - firstWord);
                        } catch (...) {
                            failure = std::current_exception();
                        }
                    }
                }
                WordFiller::pool().wait();
                if (failure) {
                    std::rethrow_exception(failure);
                }
            }
            if (descending.load()) {
                throw std::invalid_argument("offsets must ascend");
            }
            batch.commit();
            return count;
        }
        throw std::runtime_error("internal error: the word batch does not converge");
    }
};

// batch_embedding / batch_embedding_into: a list of str -> rows in host memory. From a few thousand words on (and when no
// other call of this Reader holds its word batch) the str objects are written straight into the reader's pinned word
// batch by pooled threads and BOTH the word search and the decode run on the device (memb_hip_decode_words); otherwise the
// host search on UTF-8 pointers, as before. The GIL is held while the str objects are read, released for the device work.
void wordsToHostRows(memb::Reader& reader, const py::sequence& wordList, size_t count, float* destination, size_t ld, size_t colOff)
{
    memb::Reader::WordBatchLease lease = reader.leaseWordBatch(count);
    if (lease.batch) {
        WordFiller::fill(*lease.batch, wordList, [](size_t, size_t) {});
        bool done;
        {
            py::gil_scoped_release release;
            done = reader.leasedWordsToBuffer(lease, destination, ld, colOff);
        }
        if (done) {
            return;
        }
    }
    lease = memb::Reader::WordBatchLease();
    WordPointers words(wordList);
    py::gil_scoped_release release;
    reader.batchEmbeddingToStridedBuffer(words.data(), words.size(), destination, ld, colOff);
}

py::dict contextInfo(memb::Reader& reader, uint64_t batchWords)
{
    if (reader.device() == memb::CompressedStorage::HOST_DEVICE) {
        py::dict result;
        result["device"] = "cpu";
        result["dim"] = reader.dim();
        result["n_rows"] = reader.size();
        result["kernel"] = "host decode (" + reader.storageName() + ")";
        return result;
    }
    memb_hip_ctx_info info{};
    info.struct_size = sizeof(info);
    info.batch_words = batchWords;
    if (memb_hip_ctx_get_info(reader.deviceContext(), &info) != MEMB_HIP_OK) {
        throw std::runtime_error(memb_hip_last_error());
    }
    py::dict result;
    result["device"] = info.device;
    result["storage"] = info.storage;
    result["dim"] = info.dim;
    result["n_rows"] = info.n_rows;
    result["device_bytes"] = info.device_bytes;
    result["root_bits"] = info.root_bits;
    result["max_code_bits"] = info.max_code_bits;
    result["table_entries"] = info.table_entries;
    result["max_stream_bytes"] = info.max_stream_bytes;
    result["waves_per_block"] = info.waves_per_block;
    result["lanes_per_word"] = info.lanes_per_word;
    result["segment_symbols"] = info.segment_symbols;
    result["lds_bytes_per_block"] = info.lds_bytes_per_block;
    result["kernel"] = std::string(info.kernel);
    result["row_layout"] = info.row_layout;
    result["row_bytes"] = info.row_bytes;
    result["kernel_registers"] = info.kernel_registers;
    result["register_waves_per_cu"] = info.register_waves_per_cu;
    result["tiles_per_wavefront"] = info.tiles_per_wavefront;
    result["union_kernel"] = std::string(info.union_kernel);
    result["word_index_bytes"] = info.word_index_bytes;
    result["word_index_slots"] = info.word_index_slots;
    result["word_index_keys"] = info.word_index_keys;
    return result;
}

// What every pool_*_to_device method passes on: the sequential lookup over every entry, to which the method adds its own
memb::PooledLookup pooledLookup(
    uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, int outType, size_t ld, size_t colOff, int mode,
    uintptr_t stream)
{
    memb::PooledLookup lookup{
        reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<const uint32_t*>(offsets), bags, reinterpret_cast<void*>(out),
        outType, ld, colOff, mode};
    lookup.stream = reinterpret_cast<void*>(stream);
    return lookup;
}

}  // namespace

// The caller's output matrix for the *_into calls, used in place: float32, writeable, two-dimensional,
// unit column stride; rows may be strided (a column or row range of a wider matrix). Anything
// else is refused -- letting pybind11 convert it would fill a temporary copy and leave the
// caller's matrix untouched without a word.
struct OutputMatrix {
    float* data;
    size_t rows;
    size_t columns;
    size_t ld;   // floats between the starts of consecutive rows
};

OutputMatrix outputMatrix(const py::array& out)
{
    if (!py::isinstance<py::array_t<float>>(out) || !py::dtype::of<float>().is(out.dtype())) {
        throw py::type_error("out must be a numpy float32 array (no conversion is made: the result is written in place)");
    }
    if (!out.writeable()) {
        throw py::type_error("out is read-only");
    }
    if (out.ndim() != 2) {
        throw py::type_error("out must be 2-dimensional");
    }
    const py::ssize_t item = static_cast<py::ssize_t>(sizeof(float));
    if ((out.shape(1) > 1 && out.strides(1) != item) || out.strides(0) < 0 || out.strides(0) % item != 0 ||
        (out.shape(0) > 1 && out.strides(0) < out.shape(1) * item)) {
        throw py::type_error("out must have unit column stride and non-overlapping rows (row slices and column ranges of a C-contiguous matrix are fine)");
    }
    OutputMatrix matrix;
    matrix.data = static_cast<float*>(const_cast<void*>(out.data()));
    matrix.rows = static_cast<size_t>(out.shape(0));
    matrix.columns = static_cast<size_t>(out.shape(1));
    matrix.ld = out.shape(0) > 1 ? static_cast<size_t>(out.strides(0) / item) : matrix.columns;
    return matrix;
}

PYBIND11_MODULE(_memb, m) {
    py::class_<memb::Builder>(m, "Builder")
        .def(py::init<size_t, const std::string&, size_t>())
        .def(py::init<size_t, const std::string&, size_t, int>(),
             py::arg("dim"), py::arg("storage_type"), py::arg("bits_per_weight"), py::arg("device"))
        .def(
            "add_word",
            [](memb::Builder& builder, const std::string& word, py::array_t<float, py::array::c_style> values)
            {
                auto valuesBuffer = values.request();
                if (valuesBuffer.ndim != 1) {
                    throw std::runtime_error("Word vector must be 1-dimensional");
                }
                builder.addWord(
                    word, reinterpret_cast<const float*>(valuesBuffer.ptr), static_cast<size_t>(valuesBuffer.shape[0]));
            })
        .def(
            "add_words",
            [](memb::Builder& builder,
               const std::vector<std::string>& words,
               py::array_t<float, py::array::c_style | py::array::forcecast> matrix)
            {
                auto buffer = matrix.request();
                if (buffer.ndim != 2 || static_cast<size_t>(buffer.shape[0]) != words.size()) {
                    throw std::runtime_error("Expected a matrix with one row per word");
                }
                const float* values = reinterpret_cast<const float*>(buffer.ptr);
                const size_t dim = static_cast<size_t>(buffer.shape[1]);
                py::gil_scoped_release release;   // copies rows: other Python threads may run meanwhile
                builder.addWords(words, values, dim);
            })
        .def(
            "save",
            [](memb::Builder& builder, const std::string& filename)
            {
                py::gil_scoped_release release;
                builder.save(filename);
            });

    // a batch of query words on a device (memb::WordBatch): see Reader.words_to_rows_device
    py::class_<memb::WordBatch, std::shared_ptr<memb::WordBatch>>(m, "WordBatch")
        .def(py::init<int>(), py::arg("device"))
        .def("size", [](memb::WordBatch& batch) { return batch.size(); })
        .def("device", [](memb::WordBatch& batch) { return batch.device(); })
        .def(
            "pack",
            [](memb::WordBatch& batch, const py::sequence& wordList) {
                BatchClaim claim(batch);
                return WordFiller::fill(batch, wordList, [](size_t, size_t) {});
            },
            py::arg("words"),
            "fills the batch from a list of str (no lookup); returns the number of words");

    py::class_<memb::Reader, std::shared_ptr<memb::Reader>>(m, "Reader")
        .def(py::init([](const std::string& filename, size_t numThreads) {
            return makeReader(filename, numThreads, -1, 0);
        }))
        .def(
            py::init([](const std::string& filename, size_t numThreads, int device, size_t maxDirectDecodeBits) {
                return makeReader(filename, numThreads, device, maxDirectDecodeBits);
            }),
            py::arg("filename"),
            py::arg("num_threads"),
            py::arg("device"),
            py::arg("max_direct_decode_bits") = 0)
        .def("dim", [](memb::Reader& reader) { return reader.dim(); })
        .def(
            "word_embedding",
            [](memb::Reader& reader, const std::string& word)
            {
                py::array_t<float> result(reader.dim());
                auto buffer = result.request();
                reader.wordEmbeddingToBuffer(word, reinterpret_cast<float*>(buffer.ptr));
                return result;
            })
        .def(
            "batch_embedding",
            [](memb::Reader& reader, const py::sequence& wordList)
            {
                const size_t count = static_cast<size_t>(py::len(wordList));
                py::array_t<float> result({count, reader.dim()});
                auto buffer = result.request();
                float* destination = reinterpret_cast<float*>(buffer.ptr);
                adviseHugePages(destination, count * reader.dim() * sizeof(float));
                wordsToHostRows(reader, wordList, count, destination, reader.dim(), 0);
                return result;
            })
        .def("keys", [](memb::Reader& reader) { return reader.keys(); })
        // ---- additions ----
        .def("size", [](memb::Reader& reader) { return reader.size(); })
        .def("device", [](memb::Reader& reader) { return reader.device(); })
        .def("set_host_below", [](memb::Reader& reader, size_t words) { reader.setHostBelow(words); })
        .def("host_below", [](memb::Reader& reader) { return reader.hostBelow(); })
        .def("host_rows_decoded", [](memb::Reader& reader) { return reader.hostRowsDecoded(); })
        .def("storage_name", [](memb::Reader& reader) { return reader.storageName(); })
        .def("info", &contextInfo, py::arg("batch_words") = 0)
        .def(
            "set_option",
            [](memb::Reader& reader, const std::string& name, uint64_t value) {
                if (memb_hip_ctx_set_option(reader.deviceContext(), name.c_str(), value) != MEMB_HIP_OK) {
                    throw std::runtime_error(memb_hip_last_error());
                }
            },
            "tuning knob of the device context (include/memb_hip.h: memb_hip_ctx_set_option)")
        .def("has_word_index", [](memb::Reader& reader) { return reader.hasWordIndex(); })
        .def(
            "context_handle",
            [](memb::Reader& reader) { return reinterpret_cast<uintptr_t>(reader.deviceContext()); })
        .def(
            "resolve_rows",
            [](memb::Reader& reader, const py::sequence& wordList)
            {
                WordPointers words(wordList);
                py::array_t<uint32_t> rows(words.size());
                auto buffer = rows.request();
                uint32_t* destination = reinterpret_cast<uint32_t*>(buffer.ptr);
                {
                    py::gil_scoped_release release;
                    reader.resolveRows(words.data(), words.size(), destination);
                }
                return rows;
            })
        .def(
            "batches_to_device",
            [](memb::Reader& reader, const std::vector<std::tuple<uintptr_t, size_t, uintptr_t, size_t, size_t>>& batches,
               uintptr_t stream) {
                std::vector<memb_hip_batch> list(batches.size());
                for (size_t k = 0; k < batches.size(); ++k) {
                    list[k].rows = reinterpret_cast<const uint32_t*>(std::get<0>(batches[k]));
                    list[k].n = std::get<1>(batches[k]);
                    list[k].out = reinterpret_cast<float*>(std::get<2>(batches[k]));
                    list[k].ld = std::get<3>(batches[k]);
                    list[k].col_off = std::get<4>(batches[k]);
                }
                reader.batchesToDeviceBuffers(list.data(), list.size(), reinterpret_cast<void*>(stream));
            },
            py::arg("batches"),
            py::arg("stream") = 0,
            "several (rows_ptr, n, out_ptr, ld, col_off) lookups in one launch (memb_hip_decode_batches_device)")
        .def("stage_words", [](memb::Reader& reader) {
            py::gil_scoped_release release;
            reader.stageWords();
        })
        .def(
            "resolve_batch_to_device",
            [](memb::Reader& reader, memb::WordBatch& batch, uintptr_t rows, uintptr_t stream) {
                BatchClaim claim(batch);
                py::gil_scoped_release release;   // (may stage the keys on first use)
                reader.resolveRowsToDevice(batch, reinterpret_cast<uint32_t*>(rows), reinterpret_cast<void*>(stream));
            },
            py::arg("batch"),
            py::arg("rows_ptr"),
            py::arg("stream") = 0,
            "row ids of an already packed batch into device memory (batch.size() uint32 entries)")
        .def(
            "words_to_rows_device",
            [](memb::Reader& reader, memb::WordBatch& batch, const py::sequence& wordList, uintptr_t rows, uintptr_t stream) {
                // fill + lookup under the batch's claim (no second call shares the batch meanwhile); the lookups of finished
                // runs of jobs are enqueued while the pool fills the next. Staging the keys (first call only: tens of MB to
                // HBM, the hash table built, a synchronize) runs with the GIL released.
                BatchClaim claim(batch);
                const size_t count = static_cast<size_t>(py::len(wordList));   // (the rows at rows_ptr)
                {
                    py::gil_scoped_release release;
                    reader.stageWords();
                }
                return WordFiller::fill(batch, wordList, [&](size_t firstWord, size_t words) {
                    reader.resolveRangeToDevice(batch, firstWord, words, reinterpret_cast<uint32_t*>(rows), reinterpret_cast<void*>(stream));
                }, count);
            },
            py::arg("batch"),
            py::arg("words"),
            py::arg("rows_ptr"),
            py::arg("stream") = 0,
            "words -> row ids in device memory (len(words) uint32 entries at rows_ptr), enqueued on `stream`")
        .def(
            "packed_to_rows_device",
            [](memb::Reader& reader, memb::WordBatch& batch, const py::buffer& bytes, const py::array& offsets, uintptr_t rows, uintptr_t stream) {
                const py::buffer_info blob = bytes.request();
                const PackedWords packed = packedWords(blob, offsets);
                BatchClaim claim(batch);
                py::gil_scoped_release release;   // (plain memory from here on: the views above keep it alive)
                reader.stageWords();
                return PackedFiller::fill(batch, packed.data, packed.dataBytes, packed.offsets, packed.count, [&](size_t firstWord, size_t words) {
                    reader.resolveRangeToDevice(batch, firstWord, words, reinterpret_cast<uint32_t*>(rows), reinterpret_cast<void*>(stream));
                });
            },
            py::arg("batch"),
            py::arg("bytes"),
            py::arg("offsets"),
            py::arg("rows_ptr"),
            py::arg("stream") = 0,
            "words packed as one buffer of UTF-8 bytes + n + 1 ascending uint32 offsets -> row ids in device memory")
        .def(
            "packed_device_to_rows_device",
            [](memb::Reader& reader, uintptr_t bytes, size_t bytesLen, uintptr_t offsets, size_t count, uintptr_t rows, uintptr_t stream) {
                py::gil_scoped_release release;
                reader.stageWords();
                if (memb_hip_resolve_packed_device_bounded(
                        reader.deviceContext(), reinterpret_cast<const uint8_t*>(bytes), bytesLen, reinterpret_cast<const uint32_t*>(offsets),
                        count, reinterpret_cast<uint32_t*>(rows), reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("HIP word search failed: ") + memb_hip_last_error());
                }
            },
            py::arg("bytes_ptr"),
            py::arg("bytes_len"),
            py::arg("offsets_ptr"),
            py::arg("n"),
            py::arg("rows_ptr"),
            py::arg("stream") = 0,
            "the same for bytes (bytes_len of them) and offsets that are in device memory already: a word whose offsets run "
            "backwards or reach past bytes_len is not in the model (memb_hip_resolve_packed_device_bounded)")
        .def(
            "batch_embedding_into",
            [](memb::Reader& reader,
               const py::sequence& wordList,
               const py::array& out,
               size_t colOff)
            {
                const size_t count = static_cast<size_t>(py::len(wordList));
                const OutputMatrix matrix = outputMatrix(out);
                if (matrix.rows != count || matrix.columns < colOff + reader.dim()) {
                    throw std::runtime_error("Output must be a (len(words), >= col_off + dim) float32 matrix");
                }
                wordsToHostRows(reader, wordList, count, matrix.data, matrix.ld, colOff);
            })
        .def(
            "rows_embedding",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows)
            {
                auto rowsBuffer = rows.request();
                if (rowsBuffer.ndim != 1) {
                    throw std::runtime_error("Row ids must be 1-dimensional");
                }
                size_t n = static_cast<size_t>(rowsBuffer.shape[0]);
                py::array_t<float> result({n, reader.dim()});
                auto buffer = result.request();
                float* destination = reinterpret_cast<float*>(buffer.ptr);
                adviseHugePages(destination, n * reader.dim() * sizeof(float));
                const uint32_t* source = reinterpret_cast<const uint32_t*>(rowsBuffer.ptr);
                {
                    py::gil_scoped_release release;
                    reader.rowsToBuffer(source, n, destination, reader.dim(), 0);
                }
                return result;
            })
        .def(
            "rows_embedding_into",
            [](memb::Reader& reader,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
               const py::array& out,
               size_t colOff)
            {
                auto rowsBuffer = rows.request();
                const OutputMatrix matrix = outputMatrix(out);
                if (rowsBuffer.ndim != 1 || matrix.rows != static_cast<size_t>(rowsBuffer.shape[0]) ||
                    matrix.columns < colOff + reader.dim()) {
                    throw std::runtime_error("Output must be a (len(rows), >= col_off + dim) float32 matrix");
                }
                const uint32_t* source = reinterpret_cast<const uint32_t*>(rowsBuffer.ptr);
                const size_t n = matrix.rows;
                py::gil_scoped_release release;
                reader.rowsToBuffer(source, n, matrix.data, matrix.ld, colOff);
            },
            py::arg("rows"),
            py::arg("out"),
            py::arg("col_off") = 0)
        .def(
            "rows_to_device",
            [](memb::Reader& reader,
               uintptr_t rows,
               size_t n,
               uintptr_t out,
               size_t ld,
               size_t colOff,
               uintptr_t stream,
               bool accumulate,
               float divisor,
               bool randomOrder)
            {
                reader.rowsToDeviceBuffer(
                    reinterpret_cast<const uint32_t*>(rows),
                    n,
                    reinterpret_cast<float*>(out),
                    ld,
                    colOff,
                    reinterpret_cast<void*>(stream),
                    accumulate,
                    divisor,
                    randomOrder);
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("out_ptr"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("stream") = 0,
            py::arg("accumulate") = false,
            py::arg("divisor") = 0.0f,
            py::arg("random_order") = false)
        .def(
            "rows_to_device_typed",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t out, int outType, size_t ld, size_t colOff,
               uintptr_t stream)
            {
                reader.rowsToDeviceBufferTyped(
                    reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<void*>(out), outType, ld, colOff,
                    reinterpret_cast<void*>(stream));
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("out_ptr"),
            py::arg("out_type"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("stream") = 0)
        .def(
            "pool_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType)
            {
                reader.poolRowsDevice(pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream));
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("bags"),
            py::arg("out_ptr"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("mode") = MEMB_HIP_POOL_MEAN,
            py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32)
        .def(
            "pool_known_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType, uintptr_t counts)
            {
                memb::PooledLookup lookup = pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream);
                lookup.skip = true;
                lookup.counts = reinterpret_cast<uint32_t*>(counts);
                reader.poolRowsDevice(lookup);
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("bags"),
            py::arg("out_ptr"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("mode") = MEMB_HIP_POOL_MEAN,
            py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32,
            py::arg("counts_ptr") = 0)
        .def(
            "pool_chunked_workspace_bytes",
            [](memb::Reader& reader, size_t n, size_t bags) { return reader.poolChunkedWorkspaceBytes(n, bags); },
            py::arg("n"),
            py::arg("bags"))
        .def(
            "pool_rows_chunked_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType, bool skipMissing, uintptr_t counts, uintptr_t workspace,
               size_t workspaceBytes)
            {
                memb::PooledLookup lookup = pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream);
                lookup.skip = skipMissing;
                lookup.counts = reinterpret_cast<uint32_t*>(counts);
                lookup.chunked = true;
                lookup.workspace = reinterpret_cast<void*>(workspace);
                lookup.workspaceBytes = workspaceBytes;
                reader.poolRowsDevice(lookup);
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("bags"),
            py::arg("out_ptr"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("mode") = MEMB_HIP_POOL_MEAN,
            py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32,
            py::arg("skip_missing") = false,
            py::arg("counts_ptr") = 0,
            py::arg("workspace_ptr") = 0,
            py::arg("workspace_bytes") = 0)
        .def(
            "pooled_algorithmic_bytes",
            [](memb::Reader& reader,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> offsets,
               int outType)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs bags + 1 entries");
                }
                uint64_t bytes = 0;
                if (memb_hip_pooled_algorithmic_bytes_typed(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), outType, &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_pooled_algorithmic_bytes_typed: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("offsets"),
            py::arg("out_type") = MEMB_HIP_OUT_F32)
        // include/memb_hip_norms.h. Device pointers. False where the fused kernel does not exist for this model
        // (MEMB_HIP_UNSUPPORTED): the caller decodes the rows and calls dense_row_norms_to_device.
        .def(
            "row_norms_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t norms, uintptr_t stream)
            {
                const int code = memb_hip_row_norms_device(
                    reader.deviceContext(), reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<float*>(norms),
                    reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_row_norms_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("norms_ptr"),
            py::arg("stream") = 0)
        .def(
            "unit_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t out, size_t ld, size_t colOff, uintptr_t norms,
               uintptr_t stream)
            {
                if (memb_hip_decode_unit_rows_device(
                        reader.deviceContext(), reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<float*>(out), ld,
                        colOff, reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_decode_unit_rows_device: ") + memb_hip_last_error());
                }
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("out_ptr"),
            py::arg("ld"),
            py::arg("col_off") = 0,
            py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family row_norms_to_device (unit_rows false) or unit_rows_to_device launches for this output
        .def(
            "norms_kernel_name",
            [](memb::Reader& reader, bool unitRows, uintptr_t out, size_t ld, size_t colOff)
            {
                return std::string(memb_hip_norms_kernel_name(
                    reader.deviceContext(), unitRows ? 1 : 0, reinterpret_cast<const void*>(out), ld, colOff));
            },
            py::arg("unit_rows"),
            py::arg("out_ptr") = 0,
            py::arg("ld") = 0,
            py::arg("col_off") = 0)
        .def(
            "norms_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows, bool unitRows,
               bool norms)
            {
                uint64_t bytes = 0;
                if (memb_hip_norms_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), unitRows ? 1 : 0, norms ? 1 : 0,
                        &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_norms_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("unit_rows") = false,
            py::arg("norms") = true)
        // include/memb_hip_pairs.h. Device pointers: 2 n interleaved row ids; each of the three outputs may be 0. False where
        // the fused kernel does not exist for this model (MEMB_HIP_UNSUPPORTED): the caller decodes the rows and calls
        // dense_pair_similarity_to_device.
        .def(
            "pair_similarity_to_device",
            [](memb::Reader& reader, uintptr_t pairs, size_t n, uintptr_t cosines, uintptr_t dots, uintptr_t norms,
               uintptr_t stream)
            {
                const int code = memb_hip_pair_similarity_device(
                    reader.deviceContext(), reinterpret_cast<const uint32_t*>(pairs), n, reinterpret_cast<float*>(cosines),
                    reinterpret_cast<float*>(dots), reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_pair_similarity_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("pairs_ptr"),
            py::arg("n"),
            py::arg("cosines_ptr"),
            py::arg("dots_ptr") = 0,
            py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family pair_similarity_to_device launches, '' where it returns False
        .def(
            "pairs_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_pairs_kernel_name(reader.deviceContext())); })
        .def(
            "pairs_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> pairs, bool cosines,
               bool dots, bool norms)
            {
                uint64_t bytes = 0;
                if (memb_hip_pairs_algorithmic_bytes(
                        reader.deviceContext(), pairs.data(), static_cast<size_t>(pairs.size() / 2), cosines ? 1 : 0,
                        dots ? 1 : 0, norms ? 1 : 0, &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_pairs_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("pairs"),
            py::arg("cosines") = true,
            py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_bag_pairs.h. Device pointers: n row ids cut into 2 * pairs bags by 2 * pairs + 1 offsets; each of
        // the three outputs may be 0. False where the fused kernel does not exist for this model (MEMB_HIP_UNSUPPORTED): the
        // caller pools the bags and calls dense_pair_similarity_to_device.
        .def(
            "bag_pair_similarity_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t pairs, int mode, uintptr_t cosines,
               uintptr_t dots, uintptr_t norms, uintptr_t stream)
            {
                const int code = memb_hip_bag_pair_similarity_device(
                    reader.deviceContext(), reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<const uint32_t*>(offsets),
                    pairs, mode, reinterpret_cast<float*>(cosines), reinterpret_cast<float*>(dots),
                    reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_bag_pair_similarity_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("pairs"),
            py::arg("mode"),
            py::arg("cosines_ptr"),
            py::arg("dots_ptr") = 0,
            py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family bag_pair_similarity_to_device launches, '' where it returns False
        .def(
            "bag_pairs_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_bag_pairs_kernel_name(reader.deviceContext())); })
        .def(
            "bag_pairs_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> offsets, bool cosines, bool dots, bool norms)
            {
                if (offsets.size() < 1 || offsets.size() % 2 != 1) {
                    throw std::invalid_argument("offsets needs 2 * pairs + 1 entries");
                }
                uint64_t bytes = 0;
                if (memb_hip_bag_pairs_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() / 2), cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0,
                        &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_bag_pairs_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("offsets"),
            py::arg("cosines") = true,
            py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_queries.h. Device pointers: `groups` fp32 query rows ld_queries floats apart, n candidate row ids
        // cut into groups by groups + 1 offsets; each of the three outputs (n floats) may be 0. False where the fused kernel
        // does not exist for this model (MEMB_HIP_UNSUPPORTED): the caller decodes the candidates and calls
        // dense_pair_similarity_to_device.
        .def(
            "query_similarity_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t groups, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, uintptr_t cosines, uintptr_t dots, uintptr_t norms, uintptr_t stream)
            {
                const int code = memb_hip_query_similarity_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), groups, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<const uint32_t*>(offsets),
                    reinterpret_cast<float*>(cosines), reinterpret_cast<float*>(dots), reinterpret_cast<float*>(norms),
                    reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_similarity_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("groups"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("cosines_ptr"),
            py::arg("dots_ptr") = 0,
            py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family query_similarity_to_device launches, '' where it returns False
        .def(
            "query_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_query_kernel_name(reader.deviceContext())); })
        .def(
            "query_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> offsets, bool cosines, bool dots, bool norms)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs groups + 1 entries");
                }
                uint64_t bytes = 0;
                if (memb_hip_query_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0,
                        &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("offsets"),
            py::arg("cosines") = true,
            py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_query_matrix.h. Device pointers: n_queries fp32 query rows ld_queries floats apart, n candidate
        // row ids every query shares; cosines and dots are (n_queries, n) matrices with rows ld_out floats apart, norms n
        // floats; each of the three may be 0. False where the fused kernel does not exist for this model
        // (MEMB_HIP_UNSUPPORTED): the caller decodes the candidates and calls dense_pair_similarity_to_device.
        .def(
            "query_matrix_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t cosines, uintptr_t dots, size_t ldOut, uintptr_t norms, uintptr_t stream)
            {
                const int code = memb_hip_query_matrix_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), nQueries, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<float*>(cosines), reinterpret_cast<float*>(dots),
                    ldOut, reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_matrix_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("n_queries"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("cosines_ptr"),
            py::arg("dots_ptr"),
            py::arg("ld_out"),
            py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family query_matrix_to_device launches, '' where it returns False
        .def(
            "query_matrix_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_query_matrix_kernel_name(reader.deviceContext())); })
        .def(
            "query_matrix_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows, size_t nQueries,
               bool cosines, bool dots, bool norms)
            {
                uint64_t bytes = 0;
                if (memb_hip_query_matrix_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), nQueries, cosines ? 1 : 0,
                        dots ? 1 : 0, norms ? 1 : 0, &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_matrix_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("n_queries"),
            py::arg("cosines") = true,
            py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_query_topk.h. Device pointers: the queries and candidates of query_matrix_to_device, k values
        // (float32) and k positions (int64) per query with rows ld_out elements apart, and a workspace of at least
        // query_topk_workspace_bytes(.., minimal=True) bytes, which decides the slicing. False where the fused kernel does
        // not exist for this model (MEMB_HIP_UNSUPPORTED): the caller takes the matrix in slices and calls
        // dense_topk_to_device with merge.
        .def(
            "query_topk_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n, uint32_t k,
               uintptr_t values, uintptr_t positions, size_t ldOut, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                const int code = memb_hip_query_topk_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), nQueries, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, k, reinterpret_cast<float*>(values),
                    reinterpret_cast<int64_t*>(positions), ldOut, reinterpret_cast<void*>(workspace), workspaceBytes,
                    reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_topk_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("n_queries"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("k"),
            py::arg("values_ptr"),
            py::arg("positions_ptr"),
            py::arg("ld_out"),
            py::arg("workspace_ptr"),
            py::arg("workspace_bytes"),
            py::arg("stream") = 0)
        // include/memb_hip_analogies.h: query_topk_to_device with a (n_queries, width) int64 device matrix of excluded
        // positions, rows ld_excluded entries apart (0 / 0 / 0: none). False likewise: the caller takes the matrix in slices
        // and calls dense_topk_excluding_to_device with merge.
        .def(
            "query_topk_excluding_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n, uint32_t k,
               uintptr_t excluded, size_t width, size_t ldExcluded, uintptr_t values, uintptr_t positions, size_t ldOut,
               uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                const int code = memb_hip_query_excluding_topk_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), nQueries, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, k, reinterpret_cast<const int64_t*>(excluded), width, ldExcluded,
                    reinterpret_cast<float*>(values), reinterpret_cast<int64_t*>(positions), ldOut,
                    reinterpret_cast<void*>(workspace), workspaceBytes, reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_excluding_topk_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("n_queries"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("k"),
            py::arg("excluded_ptr"),
            py::arg("width"),
            py::arg("ld_excluded"),
            py::arg("values_ptr"),
            py::arg("positions_ptr"),
            py::arg("ld_out"),
            py::arg("workspace_ptr"),
            py::arg("workspace_bytes"),
            py::arg("stream") = 0)
        // the kernel families query_topk_excluding_to_device launches, '' where it returns False
        .def(
            "query_topk_excluding_kernel_name",
            [](memb::Reader& reader) {
                memb_hip_ctx* ctx = reader.deviceContext();
                return std::string(ctx ? memb_hip_query_excluding_topk_kernel_name(ctx) : "");
            })
        .def(
            "query_topk_workspace_bytes",
            [](memb::Reader& reader, size_t nQueries, size_t n, uint32_t k, bool minimal) {
                return memb_hip_query_topk_workspace_bytes(reader.deviceContext(), nQueries, n, k, minimal ? 1 : 0);
            },
            py::arg("n_queries"),
            py::arg("n"),
            py::arg("k"),
            py::arg("minimal") = false)
        // the kernel families query_topk_to_device launches, '' where it returns False
        .def(
            "query_topk_kernel_name",
            [](memb::Reader& reader) {
                memb_hip_ctx* ctx = reader.deviceContext();
                return std::string(ctx ? memb_hip_query_topk_kernel_name(ctx) : "");
            })
        .def(
            "query_topk_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows, size_t nQueries,
               uint32_t k)
            {
                uint64_t bytes = 0;
                if (memb_hip_query_topk_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), nQueries, k, &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_topk_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("n_queries"),
            py::arg("k"))
        // include/memb_hip_query_bags.h. Device pointers: the queries of query_matrix_to_device, n entry ids cut into bags
        // by bags + 1 offsets, mode POOL_SUM / POOL_MEAN; cosines and dots (n_queries rows of bags floats, ld_out floats
        // apart) and norms (bags floats), each of which may be 0. False where the fused kernel does not exist for this
        // model (MEMB_HIP_UNSUPPORTED): the caller pools the bags and calls dense_pair_similarity_to_device.
        .def(
            "query_bags_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, size_t bags, int mode, uintptr_t cosines, uintptr_t dots, size_t ldOut, uintptr_t norms,
               uintptr_t stream)
            {
                const int code = memb_hip_query_bags_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), nQueries, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<const uint32_t*>(offsets), bags, mode,
                    reinterpret_cast<float*>(cosines), reinterpret_cast<float*>(dots), ldOut, reinterpret_cast<float*>(norms),
                    reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_bags_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("n_queries"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("bags"),
            py::arg("mode"),
            py::arg("cosines_ptr"),
            py::arg("dots_ptr"),
            py::arg("ld_out"),
            py::arg("norms_ptr"),
            py::arg("stream") = 0)
        // the kernel family query_bags_to_device launches, '' where it returns False
        .def(
            "query_bags_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_query_bags_kernel_name(reader.deviceContext())); })
        .def(
            "query_bags_algorithmic_bytes",
            [](memb::Reader& reader, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
               py::array_t<uint32_t, py::array::c_style | py::array::forcecast> offsets, size_t nQueries, bool cosines, bool dots,
               bool norms)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs bags + 1 entries");
                }
                uint64_t bytes = 0;
                if (memb_hip_query_bags_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), nQueries, cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0,
                        &bytes) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_bags_algorithmic_bytes: ") + memb_hip_last_error());
                }
                return bytes;
            },
            py::arg("rows"),
            py::arg("offsets"),
            py::arg("n_queries"),
            py::arg("cosines") = true,
            py::arg("dots") = false,
            py::arg("norms") = false)
        // the k nearest bags of every query: query_topk_to_device with bags for candidates. False likewise: the caller takes
        // the matrix in slices and calls dense_topk_to_device with merge.
        .def(
            "query_bags_topk_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, size_t bags, int mode, uint32_t k, uintptr_t values, uintptr_t positions, size_t ldOut,
               uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                const int code = memb_hip_query_bags_topk_device(
                    reader.deviceContext(), reinterpret_cast<const float*>(queries), nQueries, ldQueries,
                    reinterpret_cast<const uint32_t*>(rows), n, reinterpret_cast<const uint32_t*>(offsets), bags, mode, k,
                    reinterpret_cast<float*>(values), reinterpret_cast<int64_t*>(positions), ldOut,
                    reinterpret_cast<void*>(workspace), workspaceBytes, reinterpret_cast<void*>(stream));
                if (code == MEMB_HIP_UNSUPPORTED) {
                    return false;
                }
                if (code != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("memb_hip_query_bags_topk_device: ") + memb_hip_last_error());
                }
                return true;
            },
            py::arg("queries_ptr"),
            py::arg("n_queries"),
            py::arg("ld_queries"),
            py::arg("rows_ptr"),
            py::arg("n"),
            py::arg("offsets_ptr"),
            py::arg("bags"),
            py::arg("mode"),
            py::arg("k"),
            py::arg("values_ptr"),
            py::arg("positions_ptr"),
            py::arg("ld_out"),
            py::arg("workspace_ptr"),
            py::arg("workspace_bytes"),
            py::arg("stream") = 0)
        .def(
            "query_bags_topk_workspace_bytes",
            [](memb::Reader& reader, size_t nQueries, size_t bags, uint32_t k, bool minimal) {
                return memb_hip_query_bags_topk_workspace_bytes(reader.deviceContext(), nQueries, bags, k, minimal ? 1 : 0);
            },
            py::arg("n_queries"),
            py::arg("bags"),
            py::arg("k"),
            py::arg("minimal") = false)
        // the kernel families query_bags_topk_to_device launches, '' where it returns False
        .def(
            "query_bags_topk_kernel_name",
            [](memb::Reader& reader) { return std::string(memb_hip_query_bags_topk_kernel_name(reader.deviceContext())); });

    // include/memb_hip_query_topk.h: the k best columns of every row of any fp32 device matrix, positions as base +
    // column; merge: what values / positions hold takes part. The workspace needs dense_topk_workspace_bytes bytes.
    m.def(
        "dense_topk_to_device",
        [](int device, uintptr_t matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
           uintptr_t values, uintptr_t positions, size_t ldOut, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            if (memb_hip_dense_topk_device(
                    device, reinterpret_cast<const float*>(matrix), nRows, n, ld, base, k, merge ? 1 : 0,
                    reinterpret_cast<float*>(values), reinterpret_cast<int64_t*>(positions), ldOut,
                    reinterpret_cast<void*>(workspace), workspaceBytes, reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_dense_topk_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("matrix_ptr"),
        py::arg("n_rows"),
        py::arg("n"),
        py::arg("ld"),
        py::arg("base"),
        py::arg("k"),
        py::arg("merge"),
        py::arg("values_ptr"),
        py::arg("positions_ptr"),
        py::arg("ld_out"),
        py::arg("workspace_ptr"),
        py::arg("workspace_bytes"),
        py::arg("stream") = 0);
    // include/memb_hip_analogies.h: dense_topk_to_device with a (n_rows, width) int64 device matrix of excluded positions
    // (base + column), rows ld_excluded entries apart; the same workspace.
    m.def(
        "dense_topk_excluding_to_device",
        [](int device, uintptr_t matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
           uintptr_t excluded, size_t width, size_t ldExcluded, uintptr_t values, uintptr_t positions, size_t ldOut,
           uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            if (memb_hip_dense_excluding_topk_device(
                    device, reinterpret_cast<const float*>(matrix), nRows, n, ld, base, k, merge ? 1 : 0,
                    reinterpret_cast<const int64_t*>(excluded), width, ldExcluded, reinterpret_cast<float*>(values),
                    reinterpret_cast<int64_t*>(positions), ldOut, reinterpret_cast<void*>(workspace), workspaceBytes,
                    reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_dense_excluding_topk_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("matrix_ptr"),
        py::arg("n_rows"),
        py::arg("n"),
        py::arg("ld"),
        py::arg("base"),
        py::arg("k"),
        py::arg("merge"),
        py::arg("excluded_ptr"),
        py::arg("width"),
        py::arg("ld_excluded"),
        py::arg("values_ptr"),
        py::arg("positions_ptr"),
        py::arg("ld_out"),
        py::arg("workspace_ptr"),
        py::arg("workspace_bytes"),
        py::arg("stream") = 0);
    m.def("dense_topk_excluding_kernel_name", []() { return std::string(memb_hip_query_excluding_topk_kernel_name(nullptr)); });
    m.attr("QUERY_TOPK_MAX_EXCLUDED") = MEMB_HIP_MAX_EXCLUDED;
    // include/memb_hip_analogies.h: sums of weighted rows of any fp32 device matrix in entry order; offsets: n_sums + 1
    // uint32 on the device, weights: one float32 per entry (0: all +1).
    m.def(
        "weighted_rows_sum_to_device",
        [](int device, uintptr_t matrix, size_t ld, uintptr_t weights, uintptr_t offsets, size_t nSums, size_t dim, uintptr_t out,
           size_t ldOut, uintptr_t stream)
        {
            if (memb_hip_weighted_rows_sum_device(
                    device, reinterpret_cast<const float*>(matrix), ld, reinterpret_cast<const float*>(weights),
                    reinterpret_cast<const uint32_t*>(offsets), nSums, dim, reinterpret_cast<float*>(out), ldOut,
                    reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_weighted_rows_sum_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("matrix_ptr"),
        py::arg("ld"),
        py::arg("weights_ptr"),
        py::arg("offsets_ptr"),
        py::arg("n_sums"),
        py::arg("dim"),
        py::arg("out_ptr"),
        py::arg("ld_out"),
        py::arg("stream") = 0);
    m.def("dense_topk_workspace_bytes", &memb_hip_dense_topk_workspace_bytes, py::arg("n_rows"), py::arg("n"), py::arg("k"));
    m.def("dense_topk_kernel_name", []() { return std::string(memb_hip_query_topk_kernel_name(nullptr)); });
    m.attr("QUERY_TOPK_MAX_K") = MEMB_HIP_TOPK_MAX_K;
    // launch geometry of the selection (hip_query_topk.h), never the result: the tests size their matrices by these
    m.attr("QUERY_TOPK_MIN_SEGMENT") = memb_query_topk::MIN_SEGMENT;
    m.attr("QUERY_TOPK_MIN_SLICE") = memb_query_topk::MIN_SLICE;

    // queries query_matrix_trained holds in registers at once (hip_query_matrix.h): geometry, never the result
    m.attr("QUERY_MATRIX_BLOCK") = memb_query_matrix::QUERY_BLOCK;
    // pooled rows query_bags_trained holds in registers at once (hip_query_bags.h): geometry, never the result
    m.attr("QUERY_BAGS_GROUP") = memb_query_bags::BAG_GROUP;
    m.attr("OUT_F32") = MEMB_HIP_OUT_F32;
    m.attr("OUT_BF16") = MEMB_HIP_OUT_BF16;
    m.attr("OUT_F16") = MEMB_HIP_OUT_F16;
    m.attr("POOL_SUM") = MEMB_HIP_POOL_SUM;
    m.attr("POOL_MEAN") = MEMB_HIP_POOL_MEAN;
    m.attr("POOL_CHUNK") = MEMB_HIP_POOL_CHUNK;

    m.def("available_compression_strategies", &memb::availableCompressionStrategies);

    // Hooks for the reference's unit tests of the Builder's pieces
    // (src/kmeans_tests.cpp:9-38, src/bit_stream_tests.cpp:31-59).
    m.def("_kmeans_fit_predict", [](const std::vector<float>& data, size_t levels) {
        memb::KMeansClusterizer clusterizer(levels);
        clusterizer.fit(data);
        std::vector<uint8_t> assignments;
        clusterizer.predict(data.data(), data.size(), &assignments);
        return py::make_tuple(clusterizer.centroids(), std::vector<int>(assignments.begin(), assignments.end()));
    });
    m.def("_bit_pack", [](const std::vector<std::pair<uint32_t, uint32_t>>& codes) {
        memb::BitWriter writer;
        for (const auto& code : codes) {
            writer.push(code.first, code.second);
        }
        writer.flushToByte();
        return py::bytes(reinterpret_cast<const char*>(writer.bytes().data()), writer.bytes().size());
    });
    m.def("_huffman_description", [](const std::vector<uint64_t>& counts) {
        auto lengths = memb::huffmanCodeLengths(counts);
        std::vector<uint8_t> keys;
        std::vector<uint32_t> sizeOffsets;
        memb::decoderDescription(lengths, &keys, &sizeOffsets);
        return py::make_tuple(std::vector<int>(keys.begin(), keys.end()), sizeOffsets);
    });
    m.def("_decode_table", [](const std::vector<int>& keys, const std::vector<uint32_t>& sizeOffsets, uint32_t rootBitsLimit) {
        std::vector<uint8_t> narrow(keys.begin(), keys.end());
        auto lengths = memb::codeLengthsFromSizeOffsets(narrow.data(), narrow.size(), sizeOffsets.data(), sizeOffsets.size());
        auto table = memb::buildDecodeTable(lengths, rootBitsLimit);
        return py::make_tuple(table.rootBits, table.maxCodeBits, table.hasSubTables, table.entries);
    });

    // ReadersUnion 'concatenate' as one launch; false when the readers cannot share a kernel
    // (the caller then decodes them one by one). Pointers are device pointers.
    m.def(
        "union_rows_to_device",
        [](const std::vector<std::shared_ptr<memb::Reader>>& readers,
           const std::vector<uintptr_t>& rows,
           const std::vector<size_t>& colOffs,
           size_t n,
           uintptr_t out,
           size_t ld,
           uintptr_t stream,
           bool average)
        {
            if (readers.size() != rows.size() || readers.size() != colOffs.size() || readers.empty()) {
                throw std::runtime_error("One row-id array and one column offset per reader are needed");
            }
            std::vector<memb_hip_ctx*> contexts;
            std::vector<const uint32_t*> rowPointers;
            for (size_t i = 0; i < readers.size(); ++i) {
                contexts.push_back(readers[i]->deviceContext());
                rowPointers.push_back(reinterpret_cast<const uint32_t*>(rows[i]));
            }
            int code = memb_hip_decode_rows_union_device(
                contexts.data(), rowPointers.data(), colOffs.data(), readers.size(), n, reinterpret_cast<float*>(out), ld,
                reinterpret_cast<void*>(stream), average ? MEMB_HIP_UNION_AVERAGE : 0u);
            if (code == MEMB_HIP_UNSUPPORTED) {
                return false;
            }
            if (code != MEMB_HIP_OK) {
                throw std::runtime_error(memb_hip_last_error());
            }
            return true;
        },
        py::arg("readers"),
        py::arg("rows_ptrs"),
        py::arg("col_offs"),
        py::arg("n"),
        py::arg("out_ptr"),
        py::arg("ld"),
        py::arg("stream") = 0,
        py::arg("average") = false);
    // ReadersUnion 'average' pooled in one launch (memb_hip_pool_rows_union_device); false when the readers cannot share
    // the kernel (the caller then merges the rows and pools them with pool_dense_rows_to_device). Device pointers.
    m.def(
        "pool_union_rows_to_device",
        [](const std::vector<std::shared_ptr<memb::Reader>>& readers,
           const std::vector<uintptr_t>& rows,
           size_t n,
           uintptr_t offsets,
           size_t bags,
           uintptr_t out,
           size_t ld,
           size_t colOff,
           int mode,
           uintptr_t stream,
           int outType)
        {
            if (readers.size() != rows.size() || readers.empty()) {
                throw std::runtime_error("One row-id array per reader is needed");
            }
            std::vector<memb_hip_ctx*> contexts;
            std::vector<const uint32_t*> rowPointers;
            for (size_t i = 0; i < readers.size(); ++i) {
                contexts.push_back(readers[i]->deviceContext());
                rowPointers.push_back(reinterpret_cast<const uint32_t*>(rows[i]));
            }
            const int code = memb_hip_pool_rows_union_device(
                contexts.data(), rowPointers.data(), readers.size(), n, reinterpret_cast<const uint32_t*>(offsets), bags,
                reinterpret_cast<void*>(out), outType, ld, colOff, mode, reinterpret_cast<void*>(stream));
            if (code == MEMB_HIP_UNSUPPORTED) {
                return false;
            }
            if (code != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_pool_rows_union_device: ") + memb_hip_last_error());
            }
            return true;
        },
        py::arg("readers"),
        py::arg("rows_ptrs"),
        py::arg("n"),
        py::arg("offsets_ptr"),
        py::arg("bags"),
        py::arg("out_ptr"),
        py::arg("ld"),
        py::arg("col_off") = 0,
        py::arg("mode") = MEMB_HIP_POOL_MEAN,
        py::arg("stream") = 0,
        py::arg("out_type") = MEMB_HIP_OUT_F32);
    // what the last pooled union launch with this reader as its first ran ("" before any)
    m.def("pool_union_kernel_name", [](const std::shared_ptr<memb::Reader>& first) {
        return std::string(memb_hip_pool_union_kernel_name(first->deviceContext()));
    });
    // the kernel pool_dense_rows_to_device launches for an out type
    m.def("pool_dense_kernel_name", [](int outType) { return std::string(memb_hip_pool_dense_kernel_name(outType)); });
    // the bags of n rows of a dense fp32 matrix on `device` (memb_hip_pool_dense_rows_device). Device pointers.
    m.def(
        "pool_dense_rows_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t offsets, size_t bags, uintptr_t out,
           size_t ld, size_t colOff, int mode, uintptr_t stream, int outType)
        {
            if (memb_hip_pool_dense_rows_device(
                    device, reinterpret_cast<const float*>(values), n, dim, ldValues, reinterpret_cast<const uint32_t*>(offsets),
                    bags, reinterpret_cast<void*>(out), outType, ld, colOff, mode, reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_pool_dense_rows_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("values_ptr"),
        py::arg("n"),
        py::arg("dim"),
        py::arg("ld_values"),
        py::arg("offsets_ptr"),
        py::arg("bags"),
        py::arg("out_ptr"),
        py::arg("ld"),
        py::arg("col_off") = 0,
        py::arg("mode") = MEMB_HIP_POOL_MEAN,
        py::arg("stream") = 0,
        py::arg("out_type") = MEMB_HIP_OUT_F32);
    // the norms (memb_hip_dense_row_norms_device) and the unit rows (memb_hip_dense_unit_rows_device) of n rows of a dense
    // fp32 matrix on `device`. Device pointers.
    m.def(
        "dense_row_norms_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t norms, uintptr_t stream)
        {
            if (memb_hip_dense_row_norms_device(
                    device, reinterpret_cast<const float*>(values), n, dim, ldValues, reinterpret_cast<float*>(norms),
                    reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_dense_row_norms_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("values_ptr"),
        py::arg("n"),
        py::arg("dim"),
        py::arg("ld_values"),
        py::arg("norms_ptr"),
        py::arg("stream") = 0);
    m.def(
        "dense_unit_rows_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t out, size_t ld, size_t colOff,
           uintptr_t norms, uintptr_t stream)
        {
            if (memb_hip_dense_unit_rows_device(
                    device, reinterpret_cast<const float*>(values), n, dim, ldValues, reinterpret_cast<float*>(out), ld, colOff,
                    reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream)) != MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_dense_unit_rows_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("values_ptr"),
        py::arg("n"),
        py::arg("dim"),
        py::arg("ld_values"),
        py::arg("out_ptr"),
        py::arg("ld"),
        py::arg("col_off") = 0,
        py::arg("norms_ptr") = 0,
        py::arg("stream") = 0);
    // the kernels those two launch
    m.def("dense_norms_kernel_name", [](bool unitRows) {
        return std::string(memb_hip_norms_kernel_name(nullptr, unitRows ? 1 : 0, nullptr, 0, 0));
    });
    // the cosines, dots and norms (memb_hip_dense_pair_similarity_device) of the n pairs of rows (2i, 2i + 1) of a dense fp32
    // matrix of 2 n rows on `device`. Device pointers; each of the three outputs may be 0.
    m.def(
        "dense_pair_similarity_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t cosines, uintptr_t dots,
           uintptr_t norms, uintptr_t stream)
        {
            if (memb_hip_dense_pair_similarity_device(
                    device, reinterpret_cast<const float*>(values), n, dim, ldValues, reinterpret_cast<float*>(cosines),
                    reinterpret_cast<float*>(dots), reinterpret_cast<float*>(norms), reinterpret_cast<void*>(stream)) !=
                MEMB_HIP_OK) {
                throw std::runtime_error(std::string("memb_hip_dense_pair_similarity_device: ") + memb_hip_last_error());
            }
        },
        py::arg("device"),
        py::arg("values_ptr"),
        py::arg("n"),
        py::arg("dim"),
        py::arg("ld_values"),
        py::arg("cosines_ptr"),
        py::arg("dots_ptr") = 0,
        py::arg("norms_ptr") = 0,
        py::arg("stream") = 0);
    m.def("dense_pairs_kernel_name", [] { return std::string(memb_hip_pairs_kernel_name(nullptr)); });
    // one batch of words resolved by several readers of one device (ReadersUnion): packed and copied once
    m.def(
        "union_words_to_rows_device",
        [](memb::WordBatch& batch,
           const py::sequence& wordList,
           const std::vector<std::shared_ptr<memb::Reader>>& readers,
           const std::vector<uintptr_t>& rows,
           uintptr_t stream)
        {
            if (readers.size() != rows.size()) {
                throw std::runtime_error("One row-id array per reader is needed");
            }
            BatchClaim claim(batch);
            const size_t count = static_cast<size_t>(py::len(wordList));   // (the rows at every rows_ptrs entry)
            std::vector<const memb::Reader*> models;
            std::vector<uint32_t*> targets;
            for (size_t i = 0; i < readers.size(); ++i) {
                {
                    py::gil_scoped_release release;   // (first call: copies the keys to HBM and builds the table)
                    readers[i]->stageWords();
                }
                models.push_back(readers[i].get());
                targets.push_back(reinterpret_cast<uint32_t*>(rows[i]));
            }
            // one launch per finished run of jobs: every word fetched and hashed once, probed in each reader's table
            return WordFiller::fill(batch, wordList, [&](size_t firstWord, size_t words) {
                memb::Reader::resolveRangeToDevice(models, batch, firstWord, words, targets, reinterpret_cast<void*>(stream));
            }, count);
        },
        py::arg("batch"),
        py::arg("words"),
        py::arg("readers"),
        py::arg("rows_ptrs"),
        py::arg("stream") = 0);
    // measurement hook (bench.py's word_search block, tools/perf): seconds the calling thread and the pool spend
    // writing a list of str into a word batch's pinned memory -- the host work of a device word search
    m.def("_word_fill_seconds", [](memb::WordBatch& batch, const py::sequence& wordList) {
        BatchClaim claim(batch);
        const auto start = std::chrono::steady_clock::now();
        WordFiller::fill(batch, wordList, [](size_t, size_t) {});
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    });
    m.def("_packed_fill_seconds", [](memb::WordBatch& batch, const py::buffer& bytes, const py::array& offsets) {
        const py::buffer_info blob = bytes.request();
        const PackedWords packed = packedWords(blob, offsets);
        BatchClaim claim(batch);
        py::gil_scoped_release release;
        const auto start = std::chrono::steady_clock::now();
        PackedFiller::fill(batch, packed.data, packed.dataBytes, packed.offsets, packed.count, [](size_t, size_t) {});
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    });
    m.attr("HOST_DEVICE") = static_cast<int>(memb::CompressedStorage::HOST_DEVICE);
    m.def("_writer_mimics_official_layout", [](bool enabled) {
        memb::wire::BufferBuilder::omitDefaults() = enabled;
    });
    m.def("hip_device_count", []() {
        int count = 0;
        memb_hip_device_count(&count);
        return count;
    });
}
