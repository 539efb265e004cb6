// `_memb`: words in. Lists of str, or words a tokenizer packed already, into a word batch's pinned memory (WordFiller,
// PackedFiller), and the Reader and module entries that search them: on the device (include/memb_hip.h: memb_hip_words,
// memb_hip_resolve_*), or on the host over UTF-8 pointers.
#include "bindings_support.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

namespace memb_bindings {

namespace {

// UTF-8 pointers of a sequence of str, without copying the words (pybind11's
// vector<string> caster copies every one). The pointers stay valid while the
// sequence is alive; a word with an embedded NUL ends there, as it does for the
// reference's strcmp.
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
}  // namespace

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

size_t packWords(memb::WordBatch& batch, const py::sequence& wordList)
{
    BatchClaim claim(batch);
    return WordFiller::fill(batch, wordList, [](size_t, size_t) {});
}

void bindWords(py::module_& m, ReaderClass& cls)
{
    cls
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
        .def("stage_words", [](memb::Reader& reader) {
            py::gil_scoped_release release;
            reader.stageWords();
        })
        .def(
            "resolve_batch_to_device",
            [](memb::Reader& reader, memb::WordBatch& batch, uintptr_t rows, uintptr_t stream) {
                BatchClaim claim(batch);
                py::gil_scoped_release release;   // (may stage the keys on first use)
                reader.resolveRowsToDevice(batch, ptr<uint32_t>(rows), ptr<void>(stream));
            },
            py::arg("batch"), py::arg("rows_ptr"), py::arg("stream") = 0,
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
                    reader.resolveRangeToDevice(batch, firstWord, words, ptr<uint32_t>(rows), ptr<void>(stream));
                }, count);
            },
            py::arg("batch"), py::arg("words"), py::arg("rows_ptr"), py::arg("stream") = 0,
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
                    reader.resolveRangeToDevice(batch, firstWord, words, ptr<uint32_t>(rows), ptr<void>(stream));
                });
            },
            py::arg("batch"), py::arg("bytes"), py::arg("offsets"), py::arg("rows_ptr"), py::arg("stream") = 0,
            "words packed as one buffer of UTF-8 bytes + n + 1 ascending uint32 offsets -> row ids in device memory")
        .def(
            "packed_device_to_rows_device",
            [](memb::Reader& reader, uintptr_t bytes, size_t bytesLen, uintptr_t offsets, size_t count, uintptr_t rows, uintptr_t stream) {
                py::gil_scoped_release release;
                reader.stageWords();
                if (memb_hip_resolve_packed_device_bounded(
                        reader.deviceContext(), ptr<const uint8_t>(bytes), bytesLen, ptr<const uint32_t>(offsets), count,
                        ptr<uint32_t>(rows), ptr<void>(stream)) != MEMB_HIP_OK) {
                    throw std::runtime_error(std::string("HIP word search failed: ") + memb_hip_last_error());
                }
            },
            py::arg("bytes_ptr"), py::arg("bytes_len"), py::arg("offsets_ptr"), py::arg("n"), py::arg("rows_ptr"),
            py::arg("stream") = 0,
            "the same for bytes (bytes_len of them) and offsets that are in device memory already: a word whose offsets run "
            "backwards or reach past bytes_len is not in the model (memb_hip_resolve_packed_device_bounded)");

    // one batch of words resolved by several readers of one device (ReadersUnion): packed and copied once
    m.def(
        "union_words_to_rows_device",
        [](memb::WordBatch& batch, const py::sequence& wordList, const ReaderList& readers, const std::vector<uintptr_t>& rows,
           uintptr_t stream)
        {
            if (readers.size() != rows.size()) {
                throw std::runtime_error("One row-id array per reader is needed");
            }
            BatchClaim claim(batch);
            const size_t count = static_cast<size_t>(py::len(wordList));   // (the rows at every rows_ptrs entry)
            std::vector<const memb::Reader*> models;
            for (const auto& reader : readers) {
                {
                    py::gil_scoped_release release;   // (first call: copies the keys to HBM and builds the table)
                    reader->stageWords();
                }
                models.push_back(reader.get());
            }
            const std::vector<uint32_t*> targets = pointers<uint32_t>(rows);
            // one launch per finished run of jobs: every word fetched and hashed once, probed in each reader's table
            return WordFiller::fill(batch, wordList, [&](size_t firstWord, size_t words) {
                memb::Reader::resolveRangeToDevice(models, batch, firstWord, words, targets, ptr<void>(stream));
            }, count);
        },
        py::arg("batch"), py::arg("words"), py::arg("readers"), py::arg("rows_ptrs"), py::arg("stream") = 0);
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
}

}  // namespace memb_bindings
