// `_memb`: pooled lookups, the sum or mean of each bag of rows -- of one model (include/memb_hip_pooled.h, _known.h,
// _chunked.h, through memb::Reader::poolRowsDevice), of a ReadersUnion and of a dense matrix
// (include/memb_hip_pooled_union.h).
#include "bindings_support.h"
#include "../../include/memb_hip_pooled_union.h"

namespace memb_bindings {

namespace {

// What every pool_*_to_device method passes on: the sequential lookup over every entry, to which the method adds its own
memb::PooledLookup pooledLookup(
    uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, int outType, size_t ld, size_t colOff, int mode,
    uintptr_t stream)
{
    memb::PooledLookup lookup{
        ptr<const uint32_t>(rows), n, ptr<const uint32_t>(offsets), bags, ptr<void>(out), outType, ld, colOff, mode};
    lookup.stream = ptr<void>(stream);
    return lookup;
}

}  // namespace

void bindPooled(py::module_& m, ReaderClass& cls)
{
    cls
        .def(
            "pool_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType)
            {
                reader.poolRowsDevice(pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream));
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("offsets_ptr"), py::arg("bags"), py::arg("out_ptr"),
            py::arg("ld"), py::arg("col_off") = 0, py::arg("mode") = MEMB_HIP_POOL_MEAN, py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32)
        .def(
            "pool_known_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType, uintptr_t counts)
            {
                memb::PooledLookup lookup = pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream);
                lookup.skip = true;
                lookup.counts = ptr<uint32_t>(counts);
                reader.poolRowsDevice(lookup);
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("offsets_ptr"), py::arg("bags"), py::arg("out_ptr"),
            py::arg("ld"), py::arg("col_off") = 0, py::arg("mode") = MEMB_HIP_POOL_MEAN, py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32, py::arg("counts_ptr") = 0)
        .def(
            "pool_chunked_workspace_bytes",
            [](memb::Reader& reader, size_t n, size_t bags) { return reader.poolChunkedWorkspaceBytes(n, bags); },
            py::arg("n"), py::arg("bags"))
        .def(
            "pool_rows_chunked_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out, size_t ld,
               size_t colOff, int mode, uintptr_t stream, int outType, bool skipMissing, uintptr_t counts, uintptr_t workspace,
               size_t workspaceBytes)
            {
                memb::PooledLookup lookup = pooledLookup(rows, n, offsets, bags, out, outType, ld, colOff, mode, stream);
                lookup.skip = skipMissing;
                lookup.counts = ptr<uint32_t>(counts);
                lookup.chunked = true;
                lookup.workspace = ptr<void>(workspace);
                lookup.workspaceBytes = workspaceBytes;
                reader.poolRowsDevice(lookup);
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("offsets_ptr"), py::arg("bags"), py::arg("out_ptr"),
            py::arg("ld"), py::arg("col_off") = 0, py::arg("mode") = MEMB_HIP_POOL_MEAN, py::arg("stream") = 0,
            py::arg("out_type") = MEMB_HIP_OUT_F32, py::arg("skip_missing") = false, py::arg("counts_ptr") = 0,
            py::arg("workspace_ptr") = 0, py::arg("workspace_bytes") = 0)
        .def(
            "pooled_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, HostIds offsets, int outType)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs bags + 1 entries");
                }
                return algorithmicBytes("memb_hip_pooled_algorithmic_bytes_typed", [&](uint64_t* bytes) {
                    return memb_hip_pooled_algorithmic_bytes_typed(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), outType, bytes);
                });
            },
            py::arg("rows"), py::arg("offsets"), py::arg("out_type") = MEMB_HIP_OUT_F32);

    // ReadersUnion 'average' pooled in one launch (memb_hip_pool_rows_union_device); false when the readers cannot share
    // the kernel (the caller then merges the rows and pools them with pool_dense_rows_to_device). Device pointers.
    m.def(
        "pool_union_rows_to_device",
        [](const ReaderList& readers, const std::vector<uintptr_t>& rows, size_t n, uintptr_t offsets, size_t bags, uintptr_t out,
           size_t ld, size_t colOff, int mode, uintptr_t stream, int outType)
        {
            if (readers.size() != rows.size() || readers.empty()) {
                throw std::runtime_error("One row-id array per reader is needed");
            }
            return supported(
                memb_hip_pool_rows_union_device(
                    contexts(readers).data(), pointers<const uint32_t>(rows).data(), readers.size(), n,
                    ptr<const uint32_t>(offsets), bags, ptr<void>(out), outType, ld, colOff, mode, ptr<void>(stream)),
                "memb_hip_pool_rows_union_device");
        },
        py::arg("readers"), py::arg("rows_ptrs"), py::arg("n"), py::arg("offsets_ptr"), py::arg("bags"),
        py::arg("out_ptr"), py::arg("ld"), py::arg("col_off") = 0, py::arg("mode") = MEMB_HIP_POOL_MEAN,
        py::arg("stream") = 0, py::arg("out_type") = MEMB_HIP_OUT_F32);
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
            check(
                memb_hip_pool_dense_rows_device(
                    device, ptr<const float>(values), n, dim, ldValues, ptr<const uint32_t>(offsets), bags, ptr<void>(out),
                    outType, ld, colOff, mode, ptr<void>(stream)),
                "memb_hip_pool_dense_rows_device");
        },
        py::arg("device"), py::arg("values_ptr"), py::arg("n"), py::arg("dim"), py::arg("ld_values"),
        py::arg("offsets_ptr"), py::arg("bags"), py::arg("out_ptr"), py::arg("ld"), py::arg("col_off") = 0,
        py::arg("mode") = MEMB_HIP_POOL_MEAN, py::arg("stream") = 0, py::arg("out_type") = MEMB_HIP_OUT_F32);
}

}  // namespace memb_bindings
