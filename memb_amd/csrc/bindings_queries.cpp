// `_memb`: fp32 query vectors against candidates that are decoded, or pooled, and never written -- per group of
// candidates (include/memb_hip_queries.h), as a matrix (include/memb_hip_query_matrix.h), the k nearest
// (include/memb_hip_query_topk.h), with exclusion lists and weighted sums for analogies (include/memb_hip_analogies.h),
// against bags (include/memb_hip_query_bags.h) -- their dense counterparts, and the launch geometry the tests size by.
#include "bindings_support.h"
#include "../../include/memb_hip_queries.h"
#include "../../include/memb_hip_query_matrix.h"
#include "hip_query_matrix.h"
#include "../../include/memb_hip_query_topk.h"
#include "hip_query_topk.h"
#include "../../include/memb_hip_analogies.h"
#include "../../include/memb_hip_query_bags.h"
#include "hip_query_bags.h"

namespace memb_bindings {

void bindQueries(py::module_& m, ReaderClass& cls)
{
    cls
        // include/memb_hip_queries.h. Device pointers: `groups` fp32 query rows ld_queries floats apart, n candidate row ids
        // cut into groups by groups + 1 offsets; each of the three outputs (n floats) may be 0. False where the fused kernel
        // does not exist for this model: the caller decodes the candidates and calls dense_pair_similarity_to_device.
        .def(
            "query_similarity_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t groups, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, uintptr_t cosines, uintptr_t dots, uintptr_t norms, uintptr_t stream)
            {
                return supported(
                    memb_hip_query_similarity_device(
                        reader.deviceContext(), ptr<const float>(queries), groups, ldQueries, ptr<const uint32_t>(rows), n,
                        ptr<const uint32_t>(offsets), ptr<float>(cosines), ptr<float>(dots), ptr<float>(norms),
                        ptr<void>(stream)),
                    "memb_hip_query_similarity_device");
            },
            py::arg("queries_ptr"), py::arg("groups"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("offsets_ptr"), py::arg("cosines_ptr"), py::arg("dots_ptr") = 0, py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family query_similarity_to_device launches, '' where it returns False
        .def("query_kernel_name", &kernelName<memb_hip_query_kernel_name>)
        .def(
            "query_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, HostIds offsets, bool cosines, bool dots, bool norms)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs groups + 1 entries");
                }
                return algorithmicBytes("memb_hip_query_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_query_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0, bytes);
                });
            },
            py::arg("rows"), py::arg("offsets"), py::arg("cosines") = true, py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_query_matrix.h. Device pointers: n_queries fp32 query rows ld_queries floats apart, n candidate
        // row ids every query shares; cosines and dots are (n_queries, n) matrices with rows ld_out floats apart, norms n
        // floats; each of the three may be 0. False where the fused kernel does not exist for this model:
        // the caller decodes the candidates and calls dense_pair_similarity_to_device.
        .def(
            "query_matrix_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t cosines, uintptr_t dots, size_t ldOut, uintptr_t norms, uintptr_t stream)
            {
                return supported(
                    memb_hip_query_matrix_device(
                        reader.deviceContext(), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n,
                        ptr<float>(cosines), ptr<float>(dots), ldOut, ptr<float>(norms), ptr<void>(stream)),
                    "memb_hip_query_matrix_device");
            },
            py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("cosines_ptr"), py::arg("dots_ptr"), py::arg("ld_out"), py::arg("norms_ptr") = 0,
            py::arg("stream") = 0)
        // the kernel family query_matrix_to_device launches, '' where it returns False
        .def("query_matrix_kernel_name", &kernelName<memb_hip_query_matrix_kernel_name>)
        .def(
            "query_matrix_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, size_t nQueries, bool cosines, bool dots, bool norms)
            {
                return algorithmicBytes("memb_hip_query_matrix_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_query_matrix_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), nQueries, cosines ? 1 : 0,
                        dots ? 1 : 0, norms ? 1 : 0, bytes);
                });
            },
            py::arg("rows"), py::arg("n_queries"), py::arg("cosines") = true, py::arg("dots") = false,
            py::arg("norms") = false)
        // include/memb_hip_query_topk.h. Device pointers: the queries and candidates of query_matrix_to_device, k values
        // (float32) and k positions (int64) per query with rows ld_out elements apart, and a workspace of at least
        // query_topk_workspace_bytes(.., minimal=True) bytes, which decides the slicing. False where the fused kernel does
        // not exist for this model: the caller takes the matrix in slices and calls dense_topk_to_device with merge.
        .def(
            "query_topk_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n, uint32_t k,
               uintptr_t values, uintptr_t positions, size_t ldOut, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                return supported(
                    memb_hip_query_topk_device(
                        reader.deviceContext(), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n, k,
                        ptr<float>(values), ptr<int64_t>(positions), ldOut, ptr<void>(workspace), workspaceBytes,
                        ptr<void>(stream)),
                    "memb_hip_query_topk_device");
            },
            py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("k"), py::arg("values_ptr"), py::arg("positions_ptr"), py::arg("ld_out"), py::arg("workspace_ptr"),
            py::arg("workspace_bytes"), py::arg("stream") = 0)
        // include/memb_hip_analogies.h: query_topk_to_device with a (n_queries, width) int64 device matrix of excluded
        // positions, rows ld_excluded entries apart (0 / 0 / 0: none). False likewise: the caller takes the matrix in slices
        // and calls dense_topk_excluding_to_device with merge.
        .def(
            "query_topk_excluding_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n, uint32_t k,
               uintptr_t excluded, size_t width, size_t ldExcluded, uintptr_t values, uintptr_t positions, size_t ldOut,
               uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                return supported(
                    memb_hip_query_excluding_topk_device(
                        reader.deviceContext(), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n, k,
                        ptr<const int64_t>(excluded), width, ldExcluded, ptr<float>(values), ptr<int64_t>(positions), ldOut,
                        ptr<void>(workspace), workspaceBytes, ptr<void>(stream)),
                    "memb_hip_query_excluding_topk_device");
            },
            py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("k"), py::arg("excluded_ptr"), py::arg("width"), py::arg("ld_excluded"), py::arg("values_ptr"),
            py::arg("positions_ptr"), py::arg("ld_out"), py::arg("workspace_ptr"), py::arg("workspace_bytes"),
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
            py::arg("n_queries"), py::arg("n"), py::arg("k"), py::arg("minimal") = false)
        // the kernel families query_topk_to_device launches, '' where it returns False
        .def(
            "query_topk_kernel_name",
            [](memb::Reader& reader) {
                memb_hip_ctx* ctx = reader.deviceContext();
                return std::string(ctx ? memb_hip_query_topk_kernel_name(ctx) : "");
            })
        .def(
            "query_topk_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, size_t nQueries, uint32_t k)
            {
                return algorithmicBytes("memb_hip_query_topk_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_query_topk_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), nQueries, k, bytes);
                });
            },
            py::arg("rows"), py::arg("n_queries"), py::arg("k"))
        // include/memb_hip_query_bags.h. Device pointers: the queries of query_matrix_to_device, n entry ids cut into bags
        // by bags + 1 offsets, mode POOL_SUM / POOL_MEAN; cosines and dots (n_queries rows of bags floats, ld_out floats
        // apart) and norms (bags floats), each of which may be 0. False where the fused kernel does not exist for this
        // model: the caller pools the bags and calls dense_pair_similarity_to_device.
        .def(
            "query_bags_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, size_t bags, int mode, uintptr_t cosines, uintptr_t dots, size_t ldOut, uintptr_t norms,
               uintptr_t stream)
            {
                return supported(
                    memb_hip_query_bags_device(
                        reader.deviceContext(), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n,
                        ptr<const uint32_t>(offsets), bags, mode, ptr<float>(cosines), ptr<float>(dots), ldOut,
                        ptr<float>(norms), ptr<void>(stream)),
                    "memb_hip_query_bags_device");
            },
            py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("offsets_ptr"), py::arg("bags"), py::arg("mode"), py::arg("cosines_ptr"), py::arg("dots_ptr"),
            py::arg("ld_out"), py::arg("norms_ptr"), py::arg("stream") = 0)
        // the kernel family query_bags_to_device launches, '' where it returns False
        .def("query_bags_kernel_name", &kernelName<memb_hip_query_bags_kernel_name>)
        .def(
            "query_bags_algorithmic_bytes",
            [](memb::Reader& reader, HostIds rows, HostIds offsets, size_t nQueries, bool cosines, bool dots, bool norms)
            {
                if (offsets.size() < 1) {
                    throw std::invalid_argument("offsets needs bags + 1 entries");
                }
                return algorithmicBytes("memb_hip_query_bags_algorithmic_bytes", [&](uint64_t* bytes) {
                    return memb_hip_query_bags_algorithmic_bytes(
                        reader.deviceContext(), rows.data(), static_cast<size_t>(rows.size()), offsets.data(),
                        static_cast<size_t>(offsets.size() - 1), nQueries, cosines ? 1 : 0, dots ? 1 : 0, norms ? 1 : 0, bytes);
                });
            },
            py::arg("rows"), py::arg("offsets"), py::arg("n_queries"), py::arg("cosines") = true,
            py::arg("dots") = false, py::arg("norms") = false)
        // the k nearest bags of every query: query_topk_to_device with bags for candidates. False likewise: the caller takes
        // the matrix in slices and calls dense_topk_to_device with merge.
        .def(
            "query_bags_topk_to_device",
            [](memb::Reader& reader, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n,
               uintptr_t offsets, size_t bags, int mode, uint32_t k, uintptr_t values, uintptr_t positions, size_t ldOut,
               uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
            {
                return supported(
                    memb_hip_query_bags_topk_device(
                        reader.deviceContext(), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n,
                        ptr<const uint32_t>(offsets), bags, mode, k, ptr<float>(values), ptr<int64_t>(positions), ldOut,
                        ptr<void>(workspace), workspaceBytes, ptr<void>(stream)),
                    "memb_hip_query_bags_topk_device");
            },
            py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
            py::arg("offsets_ptr"), py::arg("bags"), py::arg("mode"), py::arg("k"), py::arg("values_ptr"),
            py::arg("positions_ptr"), py::arg("ld_out"), py::arg("workspace_ptr"), py::arg("workspace_bytes"),
            py::arg("stream") = 0)
        .def(
            "query_bags_topk_workspace_bytes",
            [](memb::Reader& reader, size_t nQueries, size_t bags, uint32_t k, bool minimal) {
                return memb_hip_query_bags_topk_workspace_bytes(reader.deviceContext(), nQueries, bags, k, minimal ? 1 : 0);
            },
            py::arg("n_queries"), py::arg("bags"), py::arg("k"), py::arg("minimal") = false)
        // the kernel families query_bags_topk_to_device launches, '' where it returns False
        .def("query_bags_topk_kernel_name", &kernelName<memb_hip_query_bags_topk_kernel_name>);

    // include/memb_hip_query_topk.h: the k best columns of every row of any fp32 device matrix, positions as base +
    // column; merge: what values / positions hold takes part. The workspace needs dense_topk_workspace_bytes bytes.
    m.def(
        "dense_topk_to_device",
        [](int device, uintptr_t matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
           uintptr_t values, uintptr_t positions, size_t ldOut, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            check(
                memb_hip_dense_topk_device(
                    device, ptr<const float>(matrix), nRows, n, ld, base, k, merge ? 1 : 0, ptr<float>(values),
                    ptr<int64_t>(positions), ldOut, ptr<void>(workspace), workspaceBytes, ptr<void>(stream)),
                "memb_hip_dense_topk_device");
        },
        py::arg("device"), py::arg("matrix_ptr"), py::arg("n_rows"), py::arg("n"), py::arg("ld"), py::arg("base"),
        py::arg("k"), py::arg("merge"), py::arg("values_ptr"), py::arg("positions_ptr"), py::arg("ld_out"),
        py::arg("workspace_ptr"), py::arg("workspace_bytes"), py::arg("stream") = 0);
    // include/memb_hip_analogies.h: dense_topk_to_device with a (n_rows, width) int64 device matrix of excluded positions
    // (base + column), rows ld_excluded entries apart; the same workspace.
    m.def(
        "dense_topk_excluding_to_device",
        [](int device, uintptr_t matrix, size_t nRows, size_t n, size_t ld, int64_t base, uint32_t k, bool merge,
           uintptr_t excluded, size_t width, size_t ldExcluded, uintptr_t values, uintptr_t positions, size_t ldOut,
           uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            check(
                memb_hip_dense_excluding_topk_device(
                    device, ptr<const float>(matrix), nRows, n, ld, base, k, merge ? 1 : 0, ptr<const int64_t>(excluded), width,
                    ldExcluded, ptr<float>(values), ptr<int64_t>(positions), ldOut, ptr<void>(workspace), workspaceBytes,
                    ptr<void>(stream)),
                "memb_hip_dense_excluding_topk_device");
        },
        py::arg("device"), py::arg("matrix_ptr"), py::arg("n_rows"), py::arg("n"), py::arg("ld"), py::arg("base"),
        py::arg("k"), py::arg("merge"), py::arg("excluded_ptr"), py::arg("width"), py::arg("ld_excluded"),
        py::arg("values_ptr"), py::arg("positions_ptr"), py::arg("ld_out"), py::arg("workspace_ptr"),
        py::arg("workspace_bytes"), py::arg("stream") = 0);
    m.def("dense_topk_excluding_kernel_name", &denseKernelName<memb_hip_query_excluding_topk_kernel_name>);
    m.attr("QUERY_TOPK_MAX_EXCLUDED") = MEMB_HIP_MAX_EXCLUDED;
    // include/memb_hip_analogies.h: sums of weighted rows of any fp32 device matrix in entry order; offsets: n_sums + 1
    // uint32 on the device, weights: one float32 per entry (0: all +1).
    m.def(
        "weighted_rows_sum_to_device",
        [](int device, uintptr_t matrix, size_t ld, uintptr_t weights, uintptr_t offsets, size_t nSums, size_t dim, uintptr_t out,
           size_t ldOut, uintptr_t stream)
        {
            check(
                memb_hip_weighted_rows_sum_device(
                    device, ptr<const float>(matrix), ld, ptr<const float>(weights), ptr<const uint32_t>(offsets), nSums, dim,
                    ptr<float>(out), ldOut, ptr<void>(stream)),
                "memb_hip_weighted_rows_sum_device");
        },
        py::arg("device"), py::arg("matrix_ptr"), py::arg("ld"), py::arg("weights_ptr"), py::arg("offsets_ptr"),
        py::arg("n_sums"), py::arg("dim"), py::arg("out_ptr"), py::arg("ld_out"), py::arg("stream") = 0);
    m.def("dense_topk_workspace_bytes", &memb_hip_dense_topk_workspace_bytes, py::arg("n_rows"), py::arg("n"), py::arg("k"));
    m.def("dense_topk_kernel_name", &denseKernelName<memb_hip_query_topk_kernel_name>);
    m.attr("QUERY_TOPK_MAX_K") = MEMB_HIP_TOPK_MAX_K;
    // launch geometry of the selection (hip_query_topk.h), never the result: the tests size their matrices by these
    m.attr("QUERY_TOPK_MIN_SEGMENT") = memb_query_topk::MIN_SEGMENT;
    m.attr("QUERY_TOPK_MIN_SLICE") = memb_query_topk::MIN_SLICE;
    // queries query_matrix_trained holds in registers at once (hip_query_matrix.h): geometry, never the result
    m.attr("QUERY_MATRIX_BLOCK") = memb_query_matrix::QUERY_BLOCK;
    // pooled rows query_bags_trained holds in registers at once (hip_query_bags.h): geometry, never the result
    m.attr("QUERY_BAGS_GROUP") = memb_query_bags::BAG_GROUP;
}

}  // namespace memb_bindings
