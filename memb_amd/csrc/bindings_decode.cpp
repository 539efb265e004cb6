// `_memb`: rows out. Words or row ids to rows in host memory, row ids to rows in device memory (include/memb_hip.h,
// include/memb_hip_narrow.h; ReadersUnion 'concatenate': memb_hip_decode_rows_union_device), and the device context's
// facts and tuning knobs.
#include "bindings_support.h"

#include <sys/mman.h>

namespace memb_bindings {

namespace {

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
    check(memb_hip_ctx_get_info(reader.deviceContext(), &info), nullptr);
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

}  // namespace

void bindDecode(py::module_& m, ReaderClass& cls)
{
    cls
        .def(
            "word_embedding",
            [](memb::Reader& reader, const std::string& word)
            {
                py::array_t<float> result(reader.dim());
                auto buffer = result.request();
                reader.wordEmbeddingToBuffer(word, reinterpret_cast<float*>(buffer.ptr));
                return result;
            })
        // batch_embedding / batch_embedding_into: the word search runs on the host or on the device (wordsToHostRows)
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
            [](memb::Reader& reader, HostIds rows)
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
            [](memb::Reader& reader, HostIds rows, const py::array& out, size_t colOff)
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
            py::arg("rows"), py::arg("out"), py::arg("col_off") = 0)
        .def(
            "rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t out, size_t ld, size_t colOff, uintptr_t stream,
               bool accumulate, float divisor, bool randomOrder)
            {
                reader.rowsToDeviceBuffer(
                    ptr<const uint32_t>(rows), n, ptr<float>(out), ld, colOff, ptr<void>(stream), accumulate, divisor, randomOrder);
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("out_ptr"), py::arg("ld"), py::arg("col_off") = 0,
            py::arg("stream") = 0, py::arg("accumulate") = false, py::arg("divisor") = 0.0f,
            py::arg("random_order") = false)
        .def(
            "rows_to_device_typed",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t out, int outType, size_t ld, size_t colOff,
               uintptr_t stream)
            {
                reader.rowsToDeviceBufferTyped(ptr<const uint32_t>(rows), n, ptr<void>(out), outType, ld, colOff, ptr<void>(stream));
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("out_ptr"), py::arg("out_type"), py::arg("ld"),
            py::arg("col_off") = 0, py::arg("stream") = 0)
        .def(
            "batches_to_device",
            [](memb::Reader& reader, const std::vector<std::tuple<uintptr_t, size_t, uintptr_t, size_t, size_t>>& batches,
               uintptr_t stream) {
                std::vector<memb_hip_batch> list(batches.size());
                for (size_t k = 0; k < batches.size(); ++k) {
                    list[k].rows = ptr<const uint32_t>(std::get<0>(batches[k]));
                    list[k].n = std::get<1>(batches[k]);
                    list[k].out = ptr<float>(std::get<2>(batches[k]));
                    list[k].ld = std::get<3>(batches[k]);
                    list[k].col_off = std::get<4>(batches[k]);
                }
                reader.batchesToDeviceBuffers(list.data(), list.size(), ptr<void>(stream));
            },
            py::arg("batches"), py::arg("stream") = 0,
            "several (rows_ptr, n, out_ptr, ld, col_off) lookups in one launch (memb_hip_decode_batches_device)")
        .def("info", &contextInfo, py::arg("batch_words") = 0)
        .def(
            "set_option",
            [](memb::Reader& reader, const std::string& name, uint64_t value) {
                check(memb_hip_ctx_set_option(reader.deviceContext(), name.c_str(), value), nullptr);
            },
            "tuning knob of the device context (include/memb_hip.h: memb_hip_ctx_set_option)");

    // ReadersUnion 'concatenate' as one launch; false when the readers cannot share a kernel
    // (the caller then decodes them one by one). Pointers are device pointers.
    m.def(
        "union_rows_to_device",
        [](const ReaderList& readers, const std::vector<uintptr_t>& rows, const std::vector<size_t>& colOffs, size_t n,
           uintptr_t out, size_t ld, uintptr_t stream, bool average)
        {
            if (readers.size() != rows.size() || readers.size() != colOffs.size() || readers.empty()) {
                throw std::runtime_error("One row-id array and one column offset per reader are needed");
            }
            return supported(
                memb_hip_decode_rows_union_device(
                    contexts(readers).data(), pointers<const uint32_t>(rows).data(), colOffs.data(), readers.size(), n,
                    ptr<float>(out), ld, ptr<void>(stream), average ? MEMB_HIP_UNION_AVERAGE : 0u),
                nullptr);
        },
        py::arg("readers"), py::arg("rows_ptrs"), py::arg("col_offs"), py::arg("n"), py::arg("out_ptr"), py::arg("ld"),
        py::arg("stream") = 0, py::arg("average") = false);
}

}  // namespace memb_bindings
