// pybind11 module `_memb`: the reference's binding surface
// (python/memb_bindings.cpp:11-72) -- Reader(filename, num_threads) with
// dim / word_embedding / batch_embedding / keys, Builder(dim, storage, bits)
// with add_word / save, available_compression_strategies() -- plus additions
// for device-resident results and strided (concatenated) outputs.
// Here: the module, the classes and their constructors, the constants and the reference's test hooks. The entries of
// Reader and of the module are bound by concern in bindings_words.cpp (words in), bindings_decode.cpp (rows out),
// bindings_pooled.cpp, bindings_pairs.cpp and bindings_queries.cpp; bindings_support.h is what they share.
#include "bindings_support.h"
#include "builder.h"
#include "compression_strategy.h"
#include "codec.h"

using namespace memb_bindings;

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

}  // namespace

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
            &packWords,
            py::arg("words"),
            "fills the batch from a list of str (no lookup); returns the number of words");

    ReaderClass cls(m, "Reader");
    cls
        .def(py::init([](const std::string& filename, size_t numThreads) {
            return makeReader(filename, numThreads, -1, 0);
        }))
        .def(
            py::init([](const std::string& filename, size_t numThreads, int device, size_t maxDirectDecodeBits) {
                return makeReader(filename, numThreads, device, maxDirectDecodeBits);
            }),
            py::arg("filename"), py::arg("num_threads"), py::arg("device"), py::arg("max_direct_decode_bits") = 0)
        .def("dim", [](memb::Reader& reader) { return reader.dim(); })
        .def("keys", [](memb::Reader& reader) { return reader.keys(); })
        // ---- additions ----
        .def("size", [](memb::Reader& reader) { return reader.size(); })
        .def("device", [](memb::Reader& reader) { return reader.device(); })
        .def("set_host_below", [](memb::Reader& reader, size_t words) { reader.setHostBelow(words); })
        .def("host_below", [](memb::Reader& reader) { return reader.hostBelow(); })
        .def("host_rows_decoded", [](memb::Reader& reader) { return reader.hostRowsDecoded(); })
        .def("storage_name", [](memb::Reader& reader) { return reader.storageName(); })
        .def("has_word_index", [](memb::Reader& reader) { return reader.hasWordIndex(); })
        .def(
            "context_handle",
            [](memb::Reader& reader) { return reinterpret_cast<uintptr_t>(reader.deviceContext()); });
    bindWords(m, cls);
    bindDecode(m, cls);
    bindPooled(m, cls);
    bindPairs(m, cls);
    bindQueries(m, cls);

    m.attr("OUT_F32") = MEMB_HIP_OUT_F32;
    m.attr("OUT_BF16") = MEMB_HIP_OUT_BF16;
    m.attr("OUT_F16") = MEMB_HIP_OUT_F16;
    m.attr("POOL_SUM") = MEMB_HIP_POOL_SUM;
    m.attr("POOL_MEAN") = MEMB_HIP_POOL_MEAN;
    m.attr("POOL_CHUNK") = MEMB_HIP_POOL_CHUNK;
    m.attr("HOST_DEVICE") = static_cast<int>(memb::CompressedStorage::HOST_DEVICE);

    m.def("available_compression_strategies", &memb::availableCompressionStrategies);
    m.def("hip_device_count", []() {
        int count = 0;
        memb_hip_device_count(&count);
        return count;
    });

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
    m.def("_writer_mimics_official_layout", [](bool enabled) {
        memb::wire::BufferBuilder::omitDefaults() = enabled;
    });
}
