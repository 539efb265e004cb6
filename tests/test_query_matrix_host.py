"""Cosine similarity of many query vectors against one shared candidate list without a GPU: the two restatements of the
reference of tests/query_matrix_reference.py against each other, its rows against queries_by_the_contract with one group of
all rows, the reference against float64, a device='cpu' reader bit for bit against it (include/memb_hip_query_matrix.h's
contract over reader.rows_embedding), the C header and the entry points' refusals, and hip_query_matrix_launch.h's planning,
argument checks and byte count built into a program of their own under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from pooled_reference import ids_with_misses
from queries_reference import queries_by_the_contract
from query_matrix_reference import matrix_by_the_contract, matrix_pair_by_pair

HEADER = os.path.join(REPO, 'include', 'memb_hip_query_matrix.h')
N_ROWS = 3000
ACCURACY_DIMS = (1, 3, 4, 64, 255, 256, 260, 300, 512, 516, 1024)
# tests/test_pairs_host.py asserts 2^-20 absolute for the pair contract against float64 on Gaussian rows; this is the same
# arithmetic over (query, row), so the same figure is asserted.
ACCURACY_BOUND = 2.0 ** -20


def gaussian(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_the_two_restatements_agree():
    for dim, count, n in ((4, 3, 9), (7, 2, 5), (260, 3, 6), (300, 2, 7), (516, 2, 4)):
        queries, values = gaussian((count, dim), dim), gaussian((n, dim), dim + 1)
        values[1] = 0      # a missing row
        values[2] = -0.0
        queries[1] = -0.0
        queries[0, : dim // 2] = 0
        matrix, scalar = matrix_by_the_contract(queries, values), matrix_pair_by_pair(queries, values)
        assert all(bits_equal(one, other) for one, other in zip(matrix, scalar)), dim
        assert matrix[0].shape == (count, n) and matrix[2].shape == (n,) and (matrix[0] != 0).any()
        # -0.0 against the +0.0 of a missing row: -0.0 in every piece, and the sign survives where every lane holds a piece
        assert matrix[1][1, 1].tobytes() == np.float32(-0.0 if dim >= 256 else 0.0).tobytes(), dim


def test_a_row_of_the_matrix_is_one_group_of_all_rows():
    for dim in (4, 300, 512):
        queries, values = gaussian((5, dim), dim + 2), gaussian((23, dim), dim + 3)
        values[3] = 0
        cosines, dots, norms = matrix_by_the_contract(queries, values)
        for q in range(5):
            want = queries_by_the_contract(queries[q:q + 1], values, [0, 23])
            assert want[3].all() and bits_equal(cosines[q], want[0]) and bits_equal(dots[q], want[1]) and bits_equal(norms, want[2])
    empty = matrix_by_the_contract(gaussian((2, 8), 1), np.zeros((0, 8), dtype=np.float32))
    assert empty[0].shape == (2, 0) and empty[2].shape == (0,)
    assert matrix_by_the_contract(np.zeros((0, 8), dtype=np.float32), gaussian((3, 8), 1))[0].shape == (0, 3)


def test_reference_is_close_to_float64():
    for dim in ACCURACY_DIMS:
        queries, values = gaussian((6, dim), 4000 + dim), gaussian((40, dim), 5000 + dim)
        values[:6] = queries + np.float32(0.01) * values[:6]   # cosines near 1 among them
        cosines = matrix_by_the_contract(queries, values)[0]
        x, y = queries.astype(np.float64), values.astype(np.float64)
        exact = (x @ y.T) / np.outer(np.sqrt((x * x).sum(axis=1)), np.sqrt((y * y).sum(axis=1)))
        worst = float(np.abs(cosines.astype(np.float64) - exact).max())
        print('dim', dim, 'worst |cos - cos64| =', worst / 2.0 ** -24, '* 2^-24')
        assert worst <= ACCURACY_BOUND, (dim, worst)
        assert np.abs(cosines).max() <= 1 + 2.0 ** -22 and np.abs(cosines).max() > 0.99


# ---- a device='cpu' reader ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8), ('full', 8)])
def test_host_reader_has_the_contracts_bits(native, make_model, monkeypatch, storage, bits):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # bounded slices: 53 candidates are four of them
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows = ids_with_misses(53, N_ROWS, 7)
    rows[:4] %= np.uint32(N_ROWS)
    assert (rows >= N_ROWS).any()
    queries = gaussian((5, 300), 11)
    queries[2] = reader.rows_embedding(rows[:1])[0]   # a row against itself
    want = matrix_by_the_contract(queries, reader.rows_embedding(rows))
    assert abs(float(want[0][2, 0]) - 1) <= 2.0 ** -22
    cosines = reader.similarity_matrix(queries, rows)
    assert isinstance(cosines, np.ndarray) and cosines.dtype == np.float32 and cosines.shape == (5, 53)
    assert bits_equal(cosines, want[0]), storage
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.similarity_matrix(queries, rows, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and bits_equal(got[0], want[0]), (storage, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms)
        if dots:
            assert got[1].shape == (5, 53) and bits_equal(got[1], want[1])
        if norms:
            from norms_reference import norms_by_the_contract
            assert got[2][1].shape == (53,) and bits_equal(got[2][1], want[2]) and bits_equal(got[2][1], reader.row_norms(rows))
            assert got[2][0].shape == (5,) and bits_equal(got[2][0], norms_by_the_contract(queries))
    # row q is query_similarity of query q against all rows; a (dim,) query is one row
    assert bits_equal(cosines[3], reader.query_similarity(queries[3], rows))
    assert bits_equal(reader.similarity_matrix(queries[3], rows), cosines[3:4])
    # no query, no candidate
    none = np.zeros(0, dtype=np.uint32)
    assert reader.similarity_matrix(queries, none).shape == (5, 0) and reader.similarity_matrix(queries[:0], rows).shape == (0, 53)
    empty = reader.similarity_matrix(queries[:0], rows, return_norms=True)
    assert empty[2][0].shape == (0,) and bits_equal(empty[2][1], want[2])


def test_argument_checks_raise(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    queries, rows = gaussian((3, 300), 1), np.arange(9, dtype=np.uint32)
    with pytest.raises(TypeError, match='float32'):
        reader.similarity_matrix(queries.astype(np.float64), rows)
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_matrix(queries[:, :296], rows)
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_matrix(queries[None], rows)
    assert reader.last_query_matrix_kernel == ''
    for call in (lambda: reader.similarity_matrix_device(None, None), lambda: reader.words_similarity_matrix_device(['a'], ['b'])):
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
    assert '#include "memb_hip_queries.h"' in text
    # why the matrix instructions are not an option, and what is still not built
    assert 'NO MATRIX INSTRUCTIONS' in text and 'MFMA' in text and 'order of their own' in text
    for word in ('top-k', 'bf16 / fp16', 'ReadersUnion', 'sharded readers', 'uniform or full'):
        assert word in text, word
    # the headers it extends are as they were
    for name in ('memb_hip.h', 'memb_hip_pooled.h', 'memb_hip_pairs.h', 'memb_hip_norms.h', 'memb_hip_bag_pairs.h', 'memb_hip_queries.h'):
        assert 'memb_hip_query_matrix' not in open(os.path.join(REPO, 'include', name)).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    # (without a context every call is refused before any pointer is read: the refusals that need one are checked with a
    # staged model in tests/test_gpu_query_matrix.py, and by the stand-alone program below)
    call = library.memb_hip_query_matrix_device
    call.argtypes = [pointer, pointer, size, size, pointer, size, pointer, pointer, size, pointer, pointer]
    assert refused(call(None, 64, 2, 300, 128, 5, 256, 512, 5, None, None), b'ctx')
    assert refused(call(None, None, 0, 0, None, 0, None, None, 0, None, None), b'ctx')
    name = library.memb_hip_query_matrix_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b''
    count = library.memb_hip_query_matrix_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, size, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer]
    assert refused(count(None, None, 0, 0, 1, 0, 0, None), b'null')
    assert refused(count(None, None, 0, 2 ** 16 + 1, 1, 0, 0, None), b'too large')
    assert refused(count(None, None, 2 ** 36 + 1, 1, 1, 0, 0, None), b'too large')

    from memb_amd import _memb
    for method in ('query_matrix_to_device', 'query_matrix_kernel_name', 'query_matrix_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    assert _memb.QUERY_MATRIX_BLOCK >= 1
    for method in ('similarity_matrix_device', 'words_similarity_matrix_device', 'similarity_matrix', 'last_query_matrix_kernel'):
        assert hasattr(native.Reader, method)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_and_argument_checks_under_the_host_sanitizers(tmp_path):
    # hip_query_matrix_launch.h's first part -- what a call is refused for, the grid and its actual values, the byte count by
    # hand -- as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on the HOST code: no GPU, no
    # Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'query_matrix_planning_main.cpp')
    program = str(tmp_path / 'query_matrix_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'query matrix planning: ok' in run.stdout, run.stdout
