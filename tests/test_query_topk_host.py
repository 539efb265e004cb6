"""The k nearest candidates of every query without a GPU: the two restatements of the reference of
tests/query_topk_reference.py against each other and against torch.sort(stable=True, descending=True) on the CPU, the
package's own numpy selection (memb_amd.reader.topk_host) against them, a device='cpu' reader's similarity_topk and
most_similar against the reference over similarity_matrix, the argument checks, the C header and the entry points'
refusals, and hip_query_topk_launch.h's planning, workspace sizes, refusals and byte count built into a program of their own
under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from pooled_reference import ids_with_misses
from query_topk_reference import rows_of_every_kind, same_topk, topk_by_the_contract, topk_entry_by_entry

HEADER = os.path.join(REPO, 'include', 'memb_hip_query_topk.h')
N_ROWS = 3000
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, 130)
RANKS = (1, 2, 10, 63, 64)


def every_kind(n):
    kinds = rows_of_every_kind(n)
    return [name for name, _ in kinds], np.stack([row for _, row in kinds])


def test_the_two_restatements_agree():
    for n in SIZES:
        names, matrix = every_kind(n)
        for k in RANKS:
            vectorised, scalar = topk_by_the_contract(matrix, k, base=7), topk_entry_by_entry(matrix, k, base=7)
            assert same_topk(vectorised, scalar), (n, k)
            found = min(n, k)
            assert (vectorised[1][:, found:] == -1).all() and np.isneginf(vectorised[0][:, found:]).all()
            assert (vectorised[1][:, :found] >= 7).all()
    # by hand: ties lower position first, NaN first, the zeros equal, a real -inf before an empty slot
    row = np.array([[0.0, -0.0, np.nan, 1.0, -np.inf, 1.0, np.nan]], dtype=np.float32)
    values, positions = topk_by_the_contract(row, 8)
    assert positions.tolist() == [[2, 6, 3, 5, 0, 1, 4, -1]]
    assert np.isnan(values[0, :2]).all() and values[0, 2:7].tolist() == [1.0, 1.0, 0.0, -0.0, -np.inf] and np.isneginf(values[0, 7])
    assert np.signbit(values[0, 5]) and not np.signbit(values[0, 4])


def test_the_reference_is_torch_stable_sort():
    import torch
    for n in SIZES:
        _, matrix = every_kind(n)
        ordered = torch.sort(torch.from_numpy(matrix), dim=1, descending=True, stable=True)
        for k in RANKS:
            found = min(n, k)
            values, positions = topk_by_the_contract(matrix, k)
            assert np.array_equal(positions[:, :found], ordered.indices[:, :found].numpy()), (n, k)
            assert np.array_equal(values[:, :found].view(np.uint32), ordered.values[:, :found].numpy().view(np.uint32)), (n, k)


def test_the_packages_host_selection_is_the_reference(native):
    from memb_amd.reader import topk_host
    for n in SIZES:
        _, matrix = every_kind(n)
        for k in RANKS:
            want = topk_by_the_contract(matrix, k, base=5)
            assert same_topk(topk_host(matrix, k, 5), want), (n, k)
            # three slices merged forward and reversed: the same bits
            cuts = [0, n // 3, n - n // 4, n]
            slices = [(cuts[i], cuts[i + 1]) for i in range(3)]
            for order in (slices, slices[::-1]):
                held = None
                for start, stop in order:
                    held = topk_host(matrix[:, start:stop], k, 5 + start, held)
                assert same_topk(held, want), (n, k, order)


def test_the_fallbacks_lists_fit_every_slice(native):
    # the segment lists are not monotonic in the columns: a shorter last slice can need more bytes than a full one, and the
    # one buffer similarity_topk_device's fallback reuses must hold either
    from memb_amd import _memb
    from memb_amd.reader import QUERY_DEVICE_SLICE, topk_fallback_list_bytes
    need = _memb.dense_topk_workspace_bytes
    assert QUERY_DEVICE_SLICE == 524288
    assert need(33, 524288, 10) == 33 * 228 * 10 * 8 and need(33, 509952, 10) == 33 * 249 * 10 * 8
    assert topk_fallback_list_bytes(33, 524288 + 509952, 10, QUERY_DEVICE_SLICE) == need(33, 509952, 10)
    assert need(228, 37120, 64) == 228 * 29 * 64 * 8 < need(228, 29952, 64) == topk_fallback_list_bytes(228, 37120 + 29952, 64, 37120)
    larger_tails = 0
    for count in (1, 2, 32, 33, 64, 100, 199, 228, 4096, 8192):
        for slice_size in (64, 37120, QUERY_DEVICE_SLICE):
            for tail in [0, 1, 63, 1024, 1025, slice_size - 1] + list(range(64, slice_size, max(64, slice_size // 997))):
                tail %= slice_size
                for slices in (0, 1, 3):
                    n = slices * slice_size + tail
                    given = topk_fallback_list_bytes(count, n, 10, slice_size)
                    sizes = [slice_size] * slices + ([tail] if tail else [])
                    assert all(given >= need(count, size, 10) for size in sizes), (count, slice_size, n)
                    assert given == max([need(count, size, 10) for size in sizes] + [0]), (count, slice_size, n)
                    larger_tails += bool(slices and tail and need(count, tail, 10) > need(count, slice_size, 10))
    assert larger_tails > 100   # (the case is common, not a curiosity)


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_host_reader_has_the_contracts_bits(native, make_model, monkeypatch, storage, bits):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # bounded chunks: 53 candidates are four of them
    path, words = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows = ids_with_misses(53, N_ROWS, 7)
    rows[3] = 17
    rows[10:14] = rows[3]                                # repeated ids: ties across chunks
    queries = np.random.default_rng(11).standard_normal((5, 300)).astype(np.float32)
    queries[2] = reader.rows_embedding(rows[3:4])[0]
    matrix = reader.similarity_matrix(queries, rows)
    for k in (1, 10, 53, 54, 64):
        got = reader.similarity_topk(queries, rows, k)
        assert same_topk(got, topk_by_the_contract(matrix, k)), (storage, k)
    assert reader.similarity_topk(queries, rows, 10)[1][2, :5].tolist() == [3, 10, 11, 12, 13]
    one = reader.similarity_topk(queries[1], rows, 3)
    assert same_topk(one, topk_by_the_contract(matrix[1:2], 3))
    none = reader.similarity_topk(queries, np.zeros(0, dtype=np.uint32), 3)
    assert none[0].shape == (5, 3) and (none[1] == -1).all() and np.isneginf(none[0]).all()
    assert reader.similarity_topk(queries[:0], rows, 3)[1].shape == (0, 3)
    # the whole model: positions are row ids; most_similar leaves the word itself out and answers [] for an unknown word
    whole = reader.similarity_topk(queries[2], None, 4)
    assert same_topk(whole, topk_by_the_contract(reader.similarity_matrix(queries[2], np.arange(N_ROWS, dtype=np.uint32)), 4))
    asked = [words[5], 'no such word é', words[5]]
    neighbours = reader.most_similar(asked, k=3)
    assert neighbours[1] == [] and neighbours[0] == neighbours[2] and len(neighbours[0]) == 3
    own = int(reader.resolve_rows([words[5]])[0])
    full = topk_by_the_contract(reader.similarity_matrix(reader.rows_embedding(np.array([own], dtype=np.uint32)), np.arange(N_ROWS, dtype=np.uint32)), 4)
    kept = [(float(value), int(row)) for value, row in zip(full[0][0], full[1][0]) if row != own][:3]
    vocabulary = reader.keys()
    assert neighbours[0] == [(vocabulary[row], value) for value, row in kept]
    assert reader.most_similar([], k=3) == []


def test_argument_checks_raise(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    queries, rows = np.zeros((3, 300), dtype=np.float32), np.arange(9, dtype=np.uint32)
    with pytest.raises(TypeError, match='float32'):
        reader.similarity_topk(queries.astype(np.float64), rows, 3)
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_topk(queries[:, :296], rows, 3)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match='64'):
            reader.similarity_topk(queries, rows, k)
    with pytest.raises(TypeError, match='integer'):
        reader.similarity_topk(queries, rows, 2.5)
    with pytest.raises(ValueError, match='63'):
        reader.most_similar(['a'], k=64)
    assert reader.last_query_topk_kernel == ''
    for call in (lambda: reader.similarity_topk_device(None, None, 3), lambda: reader.most_similar_device(['a'])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_query_matrix.h"' in text and 'STABLE DESCENDING SORT' in text
    for word in ("query_matrix_trained's epilogue", 'k > 64', 'ReadersUnion', 'sharded readers', 'bf16 / fp16', 'exclusion list'):
        assert word in text, word
    # the headers it extends do not know the new names
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_query_topk.h':
            older = open(os.path.join(REPO, 'include', name)).read()
            assert 'query_topk' not in older and 'dense_topk' not in older and 'TOPK' not in older, name


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    call = library.memb_hip_query_topk_device
    call.argtypes = [pointer, pointer, size, size, pointer, size, ctypes.c_uint32, pointer, pointer, size, pointer, size, pointer]
    assert refused(call(None, 64, 2, 300, 128, 5, 3, 256, 512, 3, 1024, 1 << 20, None), b'ctx')
    assert refused(call(None, None, 0, 0, None, 0, 0, None, None, 0, None, 0, None), b'ctx')
    dense = library.memb_hip_dense_topk_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int, pointer, pointer, size,
                      pointer, size, pointer]
    # (every one of these is refused before a pointer is read or the device is touched)
    assert refused(dense(0, 64, 2, 5, 5, 0, 0, 0, 128, 256, 3, 512, 1 << 20, None), b'k must')
    assert refused(dense(0, 64, 2, 5, 5, 0, 65, 0, 128, 256, 65, 512, 1 << 20, None), b'k must')
    assert refused(dense(0, None, 2, 5, 5, 0, 3, 0, 128, 256, 3, 512, 1 << 20, None), b'null')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, None, 256, 3, 512, 1 << 20, None), b'null')
    assert refused(dense(0, 64, 2, 5, 4, 0, 3, 0, 128, 256, 3, 512, 1 << 20, None), b'ld must')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 128, 256, 2, 512, 1 << 20, None), b'ld_out')
    assert refused(dense(0, 64, 2, 5, 5, -1, 3, 0, 128, 256, 3, 512, 1 << 20, None), b'base')
    assert refused(dense(0, 66, 2, 5, 5, 0, 3, 0, 128, 256, 3, 512, 1 << 20, None), b'aligned')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 128, 260, 3, 512, 1 << 20, None), b'aligned')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 128, 256, 3, 512, 47, None), b'workspace')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 128, 256, 3, None, 0, None), b'workspace')
    assert refused(dense(0, 64, 2, 2 ** 31 + 1, 2 ** 31 + 1, 0, 3, 0, 128, 256, 3, 512, 1 << 20, None), b'too large')
    assert dense(0, None, 0, 0, 0, 0, 3, 0, 128, 256, 3, None, 0, None) == 0   # no rows: a no-op, nothing touched
    bytes_needed = library.memb_hip_dense_topk_workspace_bytes
    bytes_needed.restype = size
    bytes_needed.argtypes = [size, size, ctypes.c_uint32]
    assert bytes_needed(2, 5, 3) == 48 and bytes_needed(2, 5, 65) == 0
    workspace = library.memb_hip_query_topk_workspace_bytes
    workspace.restype = size
    workspace.argtypes = [pointer, size, size, ctypes.c_uint32, ctypes.c_int]
    assert workspace(None, 2, 5, 3, 0) == 0
    name = library.memb_hip_query_topk_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b'topk_select+topk_merge'
    count = library.memb_hip_query_topk_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, size, ctypes.c_uint32, pointer]
    assert refused(count(None, None, 0, 0, 3, None), b'null')
    assert refused(count(None, None, 0, 0, 65, None), b'k must')
    assert refused(count(None, None, 0, 2 ** 16 + 1, 3, None), b'too large')

    from memb_amd import _memb
    for method in ('query_topk_to_device', 'query_topk_workspace_bytes', 'query_topk_kernel_name', 'query_topk_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    assert hasattr(_memb, 'dense_topk_to_device') and _memb.QUERY_TOPK_MAX_K == 64
    for method in ('similarity_topk_device', 'most_similar_device', 'most_similar', 'similarity_topk', 'last_query_topk_kernel'):
        assert hasattr(native.Reader, method)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_and_argument_checks_under_the_host_sanitizers(tmp_path):
    # hip_query_topk_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on
    # the HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'query_topk_planning_main.cpp')
    program = str(tmp_path / 'query_topk_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'query topk planning: ok' in run.stdout, run.stdout
