// `_memb_cosmul`: the 3CosMul scores and the k best candidates by them (include/memb_hip_cosmul.h). A module of its own
// beside `_memb`, whose Python-visible surface is pinned as it is (tests/test_bindings_surface.py): the entries here take a
// reader's context as the integer Reader.context_handle() gives, so this unit needs neither the Reader class nor its
// sources -- only libmemb_hip.so and the one device-call helper of bindings_support.h.
#include "bindings_support.h"
#include "../../include/memb_hip_cosmul.h"

namespace {

using memb_bindings::check;
using memb_bindings::ptr;
using memb_bindings::supported;

}  // namespace

PYBIND11_MODULE(_memb_cosmul, m)
{
    m.doc() = "3CosMul scores on the GPU (include/memb_hip_cosmul.h)";
    // The 3CosMul scores of any fp32 device matrix of cosines, one row per term and one column per candidate; offsets:
    // n_questions + 1 uint32 on the device, negatives_from: n_questions uint32 on the device.
    m.def(
        "cosmul_scores_to_device",
        [](int device, uintptr_t cosines, size_t ld, uintptr_t offsets, uintptr_t negativesFrom, size_t nQuestions, size_t n,
           uintptr_t scores, size_t ldScores, uintptr_t stream)
        {
            check(
                memb_hip_cosmul_scores_device(
                    device, ptr<const float>(cosines), ld, ptr<const uint32_t>(offsets), ptr<const uint32_t>(negativesFrom),
                    nQuestions, n, ptr<float>(scores), ldScores, ptr<void>(stream)),
                "memb_hip_cosmul_scores_device");
        },
        py::arg("device"), py::arg("cosines_ptr"), py::arg("ld"), py::arg("offsets_ptr"), py::arg("negatives_from_ptr"),
        py::arg("n_questions"), py::arg("n"), py::arg("scores_ptr"), py::arg("ld_scores"), py::arg("stream") = 0);
    m.def("cosmul_scores_kernel_name", [] { return std::string(memb_hip_query_cosmul_kernel_name(nullptr)); });
    // Device pointers: n_terms fp32 term vectors ld_terms floats apart, cut into questions by n_questions + 1 uint32 offsets,
    // the terms from negatives_from[q] on being negative; the candidates, the list of excluded positions and the outputs of
    // _memb's query_topk_excluding_to_device, one row per question; a workspace of at least
    // query_cosmul_workspace_bytes(.., minimal=True) bytes, which decides the slicing. context: Reader.context_handle().
    // False where the fused matrix kernel does not exist for this model: the caller takes the cosine matrix in slices and
    // calls cosmul_scores_to_device and _memb's dense_topk_excluding_to_device with merge.
    m.def(
        "query_cosmul_nearest_to_device",
        [](uintptr_t context, uintptr_t terms, size_t nTerms, size_t ldTerms, uintptr_t offsets, uintptr_t negativesFrom,
           size_t nQuestions, uintptr_t rows, size_t n, uint32_t k, uintptr_t excluded, size_t width, size_t ldExcluded,
           uintptr_t values, uintptr_t positions, size_t ldOut, uintptr_t workspace, size_t workspaceBytes, uintptr_t stream)
        {
            return supported(
                memb_hip_query_cosmul_nearest_device(
                    ptr<memb_hip_ctx>(context), ptr<const float>(terms), nTerms, ldTerms, ptr<const uint32_t>(offsets),
                    ptr<const uint32_t>(negativesFrom), nQuestions, ptr<const uint32_t>(rows), n, k, ptr<const int64_t>(excluded),
                    width, ldExcluded, ptr<float>(values), ptr<int64_t>(positions), ldOut, ptr<void>(workspace), workspaceBytes,
                    ptr<void>(stream)),
                "memb_hip_query_cosmul_nearest_device");
        },
        py::arg("context"), py::arg("terms_ptr"), py::arg("n_terms"), py::arg("ld_terms"), py::arg("offsets_ptr"),
        py::arg("negatives_from_ptr"), py::arg("n_questions"), py::arg("rows_ptr"), py::arg("n"), py::arg("k"),
        py::arg("excluded_ptr"), py::arg("width"), py::arg("ld_excluded"), py::arg("values_ptr"), py::arg("positions_ptr"),
        py::arg("ld_out"), py::arg("workspace_ptr"), py::arg("workspace_bytes"), py::arg("stream") = 0);
    m.def(
        "query_cosmul_workspace_bytes",
        [](uintptr_t context, size_t nTerms, size_t nQuestions, size_t n, uint32_t k, bool minimal) {
            return memb_hip_query_cosmul_workspace_bytes(ptr<const memb_hip_ctx>(context), nTerms, nQuestions, n, k, minimal ? 1 : 0);
        },
        py::arg("context"), py::arg("n_terms"), py::arg("n_questions"), py::arg("n"), py::arg("k"), py::arg("minimal") = false);
    // the kernel families query_cosmul_nearest_to_device launches, '' where it returns False or the reader has no context
    m.def(
        "query_cosmul_kernel_name",
        [](uintptr_t context) { return std::string(context ? memb_hip_query_cosmul_kernel_name(ptr<const memb_hip_ctx>(context)) : ""); },
        py::arg("context"));
    m.attr("COSMUL_MAX_TERMS") = MEMB_HIP_COSMUL_MAX_TERMS;
}
