// `_memb`: what is computed of rows without writing them -- norms and unit rows (include/memb_hip_norms.h), cosines of
// pairs of rows (include/memb_hip_pairs.h) and of pairs of bags (include/memb_hip_bag_pairs.h) -- each fused with the
// decode for a model, and for a dense matrix that holds the rows already.
#include "bindings_support.h"
#include "../../include/memb_hip_norms.h"
#include "../../include/memb_hip_pairs.h"
#include "../../include/memb_hip_bag_pairs.h"

namespace memb_bindings {

void bindPairs(py::module_& m, ReaderClass& cls)
{
    cls
        // include/memb_hip_norms.h. Device pointers. False where the fused kernel does not exist for this model:
        // the caller decodes the rows and calls dense_row_norms_to_device.
        .def(
            "row_norms_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t norms, uintptr_t stream)
            {
                return supported(
                    memb_hip_row_norms_device(
                        reader.deviceContext(), ptr<const uint32_t>(rows), n, ptr<float>(norms), ptr<void>(stream)),
                    "memb_hip_row_norms_device");
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("norms_ptr"), py::arg("stream") = 0)
        .def(
            "unit_rows_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t out, size_t ld, size_t colOff, uintptr_t norms,
               uintptr_t stream)
            {
                check(
                    memb_hip_decode_unit_rows_device(
                        reader.deviceContext(), ptr<const uint32_t>(rows), n, ptr<float>(out), ld, colOff, ptr<float>(norms),
                        ptr<void>(stream)),
                    "memb_hip_decode_unit_rows_device");
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("out_ptr"), py::arg("ld"), py::arg("col_off") = 0,
            py::arg("norms_ptr") = 0, py::arg("stream") = 0)
        // the kernel family row_norms_to_device (unit_rows false) or unit_rows_to_device launches for this output
        .def(
            "norms_kernel_name",
            [](memb::Reader& reader, bool unitRows, uintptr_t out, size_t ld, size_t colOff)
            {
                return std::string(
                    memb_hip_norms_kernel_name(reader.deviceContext(), unitRows ? 1 : 0, ptr<const void>(out), ld, colOff));
            },
            py::arg("unit_rows"), py::arg("out_ptr") = 0, py::arg("ld") = 0, py::arg("col_off") = 0)
        .def(
            "norms_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, bool unitRows, bool norms)
            {
                return algorithmicBytes("memb_hip_norms_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_norms_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), unitRows ? 1 : 0, norms ? 1 : 0,
                        bytes);
                });
            },
            py::arg("rows"), py::arg("unit_rows") = false, py::arg("norms") = true)
        // include/memb_hip_pairs.h. Device pointers: 2 n interleaved row ids; each of the three outputs may be 0. False where
        // the fused kernel does not exist for this model: the caller decodes the rows and calls dense_pair_similarity_to_device.
        .def(
            "pair_similarity_to_device",
            [](memb::Reader& reader, uintptr_t pairs, size_t n, uintptr_t cosines, uintptr_t dots, uintptr_t norms,
               uintptr_t stream)
            {
                return supported(
                    memb_hip_pair_similarity_device(
                        reader.deviceContext(), ptr<const uint32_t>(pairs), n, ptr<float>(cosines), ptr<float>(dots),
                        ptr<float>(norms), ptr<void>(stream)),
                    "memb_hip_pair_similarity_device");
            },
            py::arg("pairs_ptr"), py::arg("n"), py::arg("cosines_ptr"), py::arg("dots_ptr") = 0,
            py::arg("norms_ptr") = 0, py::arg("stream") = 0)
        // the kernel family pair_similarity_to_device launches, '' where it returns False
        .def("pairs_kernel_name", &kernelName<memb_hip_pairs_kernel_name>)
        .def(
            "pairs_algorithmic_bytes",
            [](memb::Reader& reader, HostIds pairs, bool cosines, bool dots, bool norms)
            {
                return algorithmicBytes("memb_hip_pairs_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_pairs_algorithmic_bytes(
                        reader.deviceContext(), pairs.data(), static_cast<size_t>(pairs.size() / 2), cosines ? 1 : 0,
                        dots ? 1 : 0, norms ? 1 : 0, bytes);
                });
            },
            py::arg("pairs"), py::arg("cosines") = true, py::arg("dots") = false, py::arg("norms") = false)
        // include/memb_hip_bag_pairs.h. Device pointers: n row ids cut into 2 * pairs bags by 2 * pairs + 1 offsets; each of
        // the three outputs may be 0. False where the fused kernel does not exist for this model: the caller pools
        // the bags and calls dense_pair_similarity_to_device.
        .def(
            "bag_pair_similarity_to_device",
            [](memb::Reader& reader, uintptr_t rows, size_t n, uintptr_t offsets, size_t pairs, int mode, uintptr_t cosines,
               uintptr_t dots, uintptr_t norms, uintptr_t stream)
            {
                return supported(
                    memb_hip_bag_pair_similarity_device(
                        reader.deviceContext(), ptr<const uint32_t>(rows), n, ptr<const uint32_t>(offsets), pairs, mode,
                        ptr<float>(cosines), ptr<float>(dots), ptr<float>(norms), ptr<void>(stream)),
                    "memb_hip_bag_pair_similarity_device");
            },
            py::arg("rows_ptr"), py::arg("n"), py::arg("offsets_ptr"), py::arg("pairs"), py::arg("mode"),
            py::arg("cosines_ptr"), py::arg("dots_ptr") = 0, py::arg("norms_ptr") = 0, py::arg("stream") = 0)
        // the kernel family bag_pair_similarity_to_device launches, '' where it returns False
        .def("bag_pairs_kernel_name", &kernelName<memb_hip_bag_pairs_kernel_name>)
        .def(
            "bag_pairs_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, HostIds offsets, bool cosines, bool dots, bool norms)
            {
                if (offsets.size() < 1 || offsets.size() % 2 != 1) {
                    throw std::invalid_argument("offsets needs 2 * pairs + 1 entries");
                }
                return algorithmicBytes("memb_hip_bag_pairs_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_bag_pairs_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() / 2), cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0, bytes);
                });
            },
            py::arg("rows"), py::arg("offsets"), py::arg("cosines") = true, py::arg("dots") = false,
            py::arg("norms") = false);

    // the norms (memb_hip_dense_row_norms_device) and the unit rows (memb_hip_dense_unit_rows_device) of n rows of a dense
    // fp32 matrix on `device`. Device pointers.
    m.def(
        "dense_row_norms_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t norms, uintptr_t stream)
        {
            check(
                memb_hip_dense_row_norms_device(
                    device, ptr<const float>(values), n, dim, ldValues, ptr<float>(norms), ptr<void>(stream)),
                "memb_hip_dense_row_norms_device");
        },
        py::arg("device"), py::arg("values_ptr"), py::arg("n"), py::arg("dim"), py::arg("ld_values"),
        py::arg("norms_ptr"), py::arg("stream") = 0);
    m.def(
        "dense_unit_rows_to_device",
        [](int device, uintptr_t values, size_t n, size_t dim, size_t ldValues, uintptr_t out, size_t ld, size_t colOff,
           uintptr_t norms, uintptr_t stream)
        {
            check(
                memb_hip_dense_unit_rows_device(
                    device, ptr<const float>(values), n, dim, ldValues, ptr<float>(out), ld, colOff, ptr<float>(norms),
                    ptr<void>(stream)),
                "memb_hip_dense_unit_rows_device");
        },
        py::arg("device"), py::arg("values_ptr"), py::arg("n"), py::arg("dim"), py::arg("ld_values"),
        py::arg("out_ptr"), py::arg("ld"), py::arg("col_off") = 0, py::arg("norms_ptr") = 0, py::arg("stream") = 0);
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
            check(
                memb_hip_dense_pair_similarity_device(
                    device, ptr<const float>(values), n, dim, ldValues, ptr<float>(cosines), ptr<float>(dots),
                    ptr<float>(norms), ptr<void>(stream)),
                "memb_hip_dense_pair_similarity_device");
        },
        py::arg("device"), py::arg("values_ptr"), py::arg("n"), py::arg("dim"), py::arg("ld_values"),
        py::arg("cosines_ptr"), py::arg("dots_ptr") = 0, py::arg("norms_ptr") = 0, py::arg("stream") = 0);
    m.def("dense_pairs_kernel_name", &denseKernelName<memb_hip_pairs_kernel_name>);
}

}  // namespace memb_bindings
