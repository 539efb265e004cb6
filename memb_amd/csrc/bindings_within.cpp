// `_memb_within`: the list of the candidates that precede a mark, per row, in CSR form (include/memb_hip_within.h). A
// module of its own beside `_memb`, whose Python-visible surface is pinned as it is (tests/test_bindings_surface.py), built
// as `_memb_ranks` is: the entries here take a reader's context as the integer Reader.context_handle() gives, so this unit
// needs neither the Reader class nor its sources -- only libmemb_hip.so and the one device-call helper of
// bindings_support.h.
#include "bindings_support.h"
#include "../../include/memb_hip_within.h"

namespace {

using memb_bindings::check;
using memb_bindings::ptr;
using memb_bindings::supported;

}  // namespace

PYBIND11_MODULE(_memb_within, m)
{
    m.doc() = "Lists of the candidates before a mark on the GPU (include/memb_hip_within.h)";
    // The lists of any fp32 device matrix, a column being the position base + column; thresholds: n_rows float32, marks:
    // n_rows int64, excluded: the int64 list of non-candidates, offsets: n_rows + 1 int64, cursors: n_rows int64, positions
    // (int64) and values (float32, or 0: not written): capacity entries each, all on the device. accumulate: row q goes on
    // at offsets[q] + cursors[q]. A workspace of at least dense_within_workspace_bytes(n_rows, n) bytes.
    m.def(
        "dense_within_to_device",
        [](int device, uintptr_t matrix, size_t nRows, size_t n, size_t ld, int64_t base, uintptr_t thresholds, uintptr_t marks,
           uintptr_t excluded, size_t width, size_t ldExcluded, bool accumulate, uintptr_t offsets, uintptr_t cursors,
           uintptr_t positions, uintptr_t values, size_t capacity, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            check(
                memb_hip_dense_within_device(
                    device, ptr<const float>(matrix), nRows, n, ld, base, ptr<const float>(thresholds), ptr<const int64_t>(marks),
                    ptr<const int64_t>(excluded), width, ldExcluded, accumulate ? 1 : 0, ptr<const int64_t>(offsets),
                    ptr<int64_t>(cursors), ptr<int64_t>(positions), ptr<float>(values), capacity, ptr<void>(workspace), workspaceBytes,
                    ptr<void>(stream)),
                "memb_hip_dense_within_device");
        },
        py::arg("device"), py::arg("matrix_ptr"), py::arg("n_rows"), py::arg("n"), py::arg("ld"), py::arg("base"),
        py::arg("thresholds_ptr"), py::arg("marks_ptr"), py::arg("excluded_ptr"), py::arg("width"), py::arg("ld_excluded"),
        py::arg("accumulate"), py::arg("offsets_ptr"), py::arg("cursors_ptr"), py::arg("positions_ptr"), py::arg("values_ptr"),
        py::arg("capacity"), py::arg("workspace_ptr"), py::arg("workspace_bytes"), py::arg("stream") = 0);
    m.def("dense_within_workspace_bytes", &memb_hip_dense_within_workspace_bytes, py::arg("n_rows"), py::arg("n"));
    m.def("dense_within_kernel_name", [] { return std::string(memb_hip_query_within_kernel_name(nullptr)); });
    // Device pointers: n_queries fp32 query vectors ld_queries floats apart, the candidates, the marks, the list of
    // non-candidates and the output as above, positions being indices into the candidates; a workspace of at least
    // query_within_workspace_bytes(.., minimal=True) bytes, which decides the slicing. context: Reader.context_handle().
    // False where the fused matrix kernel does not exist for this model: the caller takes the cosine matrix in slices and
    // calls dense_within_to_device with accumulate.
    m.def(
        "query_within_to_device",
        [](uintptr_t context, uintptr_t queries, size_t nQueries, size_t ldQueries, uintptr_t rows, size_t n, uintptr_t thresholds,
           uintptr_t marks, uintptr_t excluded, size_t width, size_t ldExcluded, uintptr_t offsets, uintptr_t cursors,
           uintptr_t positions, uintptr_t values, size_t capacity, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            return supported(
                memb_hip_query_within_device(
                    ptr<memb_hip_ctx>(context), ptr<const float>(queries), nQueries, ldQueries, ptr<const uint32_t>(rows), n,
                    ptr<const float>(thresholds), ptr<const int64_t>(marks), ptr<const int64_t>(excluded), width, ldExcluded,
                    ptr<const int64_t>(offsets), ptr<int64_t>(cursors), ptr<int64_t>(positions), ptr<float>(values), capacity,
                    ptr<void>(workspace), workspaceBytes, ptr<void>(stream)),
                "memb_hip_query_within_device");
        },
        py::arg("context"), py::arg("queries_ptr"), py::arg("n_queries"), py::arg("ld_queries"), py::arg("rows_ptr"), py::arg("n"),
        py::arg("thresholds_ptr"), py::arg("marks_ptr"), py::arg("excluded_ptr"), py::arg("width"), py::arg("ld_excluded"),
        py::arg("offsets_ptr"), py::arg("cursors_ptr"), py::arg("positions_ptr"), py::arg("values_ptr"), py::arg("capacity"),
        py::arg("workspace_ptr"), py::arg("workspace_bytes"), py::arg("stream") = 0);
    m.def(
        "query_within_workspace_bytes",
        [](uintptr_t context, size_t nQueries, size_t n, bool minimal) {
            return memb_hip_query_within_workspace_bytes(ptr<const memb_hip_ctx>(context), nQueries, n, minimal ? 1 : 0);
        },
        py::arg("context"), py::arg("n_queries"), py::arg("n"), py::arg("minimal") = false);
    // the kernel families query_within_to_device launches, '' where it returns False or the reader has no context
    m.def(
        "query_within_kernel_name",
        [](uintptr_t context) { return std::string(context ? memb_hip_query_within_kernel_name(ptr<const memb_hip_ctx>(context)) : ""); },
        py::arg("context"));
}
