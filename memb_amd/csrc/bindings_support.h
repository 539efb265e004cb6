// What the entries of the pybind11 module `_memb` share (bindings.cpp and the bindings_*.cpp it calls): the handle of the
// Reader class, the view of a uintptr_t argument as the pointer the C ABI takes, what becomes of the ABI's return
// code, and the few shapes that recur -- algorithmic bytes, kernel names, the per-reader vectors of a union call.
// No class is defined to Python here.
#pragma once

#include "reader.h"
#include "../../include/memb_hip.h"   // the return codes, memb_hip_last_error

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <pybind11/numpy.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace py = pybind11;

namespace memb_bindings {

using ReaderClass = py::class_<memb::Reader, std::shared_ptr<memb::Reader>>;
using ReaderList = std::vector<std::shared_ptr<memb::Reader>>;

// row ids, offsets or pairs in host memory: any integer array, converted to contiguous uint32 where it is not
using HostIds = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;

// A uintptr_t argument -- a device pointer, a stream, a workspace; 0 where the entry allows none -- as the pointer the
// ABI takes. The one place where a binding argument is cast.
template <typename T>
inline T* ptr(uintptr_t address)
{
    return reinterpret_cast<T*>(address);
}

// (the text is built only when there is something to throw, never on the callers' success path)
[[noreturn]] inline void fail(const char* abiName)
{
    const std::string error = memb_hip_last_error();
    throw std::runtime_error(abiName ? std::string(abiName) + ": " + error : error);
}

// A call that may not refuse: any code but OK is a RuntimeError "<abi name>: <memb_hip_last_error()>". The oldest
// entries (info, set_option, union_rows_to_device) pass no name and report the error's own text alone.
inline void check(int code, const char* abiName)
{
    if (code != MEMB_HIP_OK) {
        fail(abiName);
    }
}

// A call that may refuse: false for MEMB_HIP_UNSUPPORTED (no fused kernel for this model; the entry's comment says what
// the caller does then), otherwise as check.
inline bool supported(int code, const char* abiName)
{
    if (code == MEMB_HIP_UNSUPPORTED) {
        return false;
    }
    check(code, abiName);
    return true;
}

// *_algorithmic_bytes: call(&bytes) is the ABI call, which counts on the host what the launch would move.
template <typename Call>
inline uint64_t algorithmicBytes(const char* abiName, Call call)
{
    uint64_t bytes = 0;
    check(call(&bytes), abiName);
    return bytes;
}

// *_kernel_name of a reader, for the ABI functions that take the context alone ...
template <const char* (*Name)(const memb_hip_ctx*)>
std::string kernelName(memb::Reader& reader)
{
    return std::string(Name(reader.deviceContext()));
}

// ... and dense_*_kernel_name: the same functions without a context
template <const char* (*Name)(const memb_hip_ctx*)>
std::string denseKernelName()
{
    return std::string(Name(nullptr));
}

// The union entries take one reader and one device array of row ids per model: the vectors the ABI wants of them.
// (Each entry checks the sizes first, with a text of its own.)
inline std::vector<memb_hip_ctx*> contexts(const ReaderList& readers)
{
    std::vector<memb_hip_ctx*> result;
    for (const auto& reader : readers) {
        result.push_back(reader->deviceContext());
    }
    return result;
}

template <typename T>
inline std::vector<T*> pointers(const std::vector<uintptr_t>& addresses)
{
    std::vector<T*> result;
    for (uintptr_t address : addresses) {
        result.push_back(ptr<T>(address));
    }
    return result;
}

// bindings_words.cpp: a list of str into a word batch (WordBatch.pack), and batch_embedding's rows of a list of str
// into host memory -- on the device where the batch is large enough, see there.
size_t packWords(memb::WordBatch& batch, const py::sequence& wordList);
void wordsToHostRows(memb::Reader& reader, const py::sequence& wordList, size_t count, float* destination, size_t ld, size_t colOff);

// The binders bindings.cpp calls once Reader and WordBatch are registered (the signatures in the docstrings name them).
void bindWords(py::module_& m, ReaderClass& cls);     // bindings_words.cpp
void bindDecode(py::module_& m, ReaderClass& cls);    // bindings_decode.cpp
void bindPooled(py::module_& m, ReaderClass& cls);    // bindings_pooled.cpp
void bindPairs(py::module_& m, ReaderClass& cls);     // bindings_pairs.cpp
void bindQueries(py::module_& m, ReaderClass& cls);   // bindings_queries.cpp

}  // namespace memb_bindings
