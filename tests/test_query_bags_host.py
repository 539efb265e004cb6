"""Every query against every pooled bag of rows without a GPU: the two restatements of the reference of
tests/query_bags_reference.py against each other, a device='cpu' reader's bag_similarity_matrix and bag_similarity_topk
against the reference bit for bit (trained 4-bit and 6-bit, uniform and full models, both modes, bags with misses and
empties, whatever the host path's slice), the Python argument checks, the C header and the entry points' refusals that need
no device, and hip_query_bags_launch.h's planning, workspace sizes, refusals and byte count built into a program of their
own under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from query_bags_reference import (bags_batch, queries_batch, query_bags_by_the_contract, query_bags_pair_by_pair,
                                  query_bags_topk_by_the_contract)
from query_topk_reference import same_topk

HEADER = os.path.join(REPO, 'include', 'memb_hip_query_bags.h')
N_ROWS = 3000
MODES = ('sum', 'mean')


def same(got, want):
    return all(bits_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


def test_the_two_restatements_agree():
    rng = np.random.default_rng(5)
    for dim in (4, 12, 300):
        rows, offsets = bags_batch(4, 11, 50, dim)
        values = rng.standard_normal((len(rows), dim)).astype(np.float32)
        values[rows >= 50] = 0
        queries = queries_batch(3, dim, dim, values)
        for mode in MODES:
            vectorised = query_bags_by_the_contract(queries, values, offsets, mode)
            assert same(vectorised, query_bags_pair_by_pair(queries, values, offsets, mode)), (dim, mode)
            assert vectorised[0].shape == (3, 11) and vectorised[2].shape == (11,)
            assert not vectorised[0][:, 2].view(np.uint32).any()   # bag 2 of the draw is empty: +0.0
    # offsets as the kernels read them: clamped to n, a descent is an empty bag
    values = rng.standard_normal((10, 8)).astype(np.float32)
    queries = queries_batch(2, 8, 1)
    got = query_bags_by_the_contract(queries, values, np.array([0, 4, 2, 0xFFFFFFFF]), 'mean')
    assert same(got, query_bags_pair_by_pair(queries, values, np.array([0, 4, 2, 10]), 'mean'))
    assert not got[2][1:2].view(np.uint32).any() and got[2][2] != 0
    # no query: the norms of the pooled rows still exist
    none = query_bags_by_the_contract(queries[:0], values, np.array([0, 4, 10]), 'sum')
    assert none[0].shape == (0, 2) and same(none, query_bags_pair_by_pair(queries[:0], values, np.array([0, 4, 10]), 'sum'))


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_host_reader_has_the_contracts_bits(native, make_model, monkeypatch, storage, bits):
    import memb_amd.reader
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows, offsets = bags_batch(4, 21, N_ROWS, 7)      # misses, empties, the bag of 300 entries
    values = reader.rows_embedding(rows)
    queries = queries_batch(4, 300, 7, values)
    for mode in MODES:
        want = query_bags_by_the_contract(queries, values, offsets, mode)
        for slice_bags, chunk in ((1 << 12, 1 << 16), (4, 16), (1, 5)):   # the host path's slices never change a bit
            monkeypatch.setattr(memb_amd.reader, 'QUERY_BAGS_HOST_SLICE', slice_bags)
            monkeypatch.setattr(memb_amd.reader, 'BAGS_HOST_CHUNK', chunk)
            context = (storage, bits, mode, slice_bags)
            assert bits_equal(reader.bag_similarity_matrix(queries, rows, offsets, mode), want[0]), context
            cosines, dots, norms = reader.bag_similarity_matrix(queries, rows, offsets, mode, return_dots=True, return_norms=True)
            assert same((cosines, dots, norms[1]), want), context
            assert bits_equal(norms[0], memb_amd.reader.row_norms_host(queries)), context
            for k in (1, 10, 21, 22, 64):
                got = reader.bag_similarity_topk(queries, rows, offsets, k, mode)
                assert same_topk(got, query_bags_topk_by_the_contract(queries, values, offsets, mode, k)), (context, k)
    one = reader.bag_similarity_matrix(queries[1], rows, offsets)
    assert one.shape == (1, 21) and bits_equal(one, query_bags_by_the_contract(queries[1:2], values, offsets, 'mean')[0])
    assert reader.bag_similarity_matrix(queries[:0], rows, offsets).shape == (0, 21)
    assert reader.bag_similarity_matrix(queries, rows[:0], [0]).shape == (4, 0)
    none = reader.bag_similarity_topk(queries, rows[:0], [0], 3)
    assert none[0].shape == (4, 3) and (none[1] == -1).all() and np.isneginf(none[0]).all()
    empty = reader.bag_similarity_topk(queries, rows[:0], [0, 0, 0], 3)    # two empty bags: ties of +0.0 in index order
    assert empty[1].tolist() == [[0, 1, -1]] * 4 and not empty[0][:, :2].view(np.uint32).any()


def test_argument_checks_raise(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    queries, rows, offsets = np.zeros((3, 300), dtype=np.float32), np.arange(9, dtype=np.uint32), [0, 4, 9]
    for call in (reader.bag_similarity_matrix, lambda *a, **kw: reader.bag_similarity_topk(*a, 3, **kw)):
        with pytest.raises(TypeError, match='float32'):
            call(queries.astype(np.float64), rows, offsets)
        with pytest.raises(ValueError, match='shape'):
            call(queries[:, :296], rows, offsets)
        with pytest.raises(ValueError, match='mode'):
            call(queries, rows, offsets, mode='max')
        with pytest.raises(ValueError, match='ascend'):
            call(queries, rows, [0, 5, 4])
        with pytest.raises(ValueError, match='0 .. len'):
            call(queries, rows, [0, 10])
        with pytest.raises(ValueError, match='bags \\+ 1'):
            call(queries, rows, [])
        with pytest.raises(ValueError, match='integers'):
            call(queries, rows, [0.0, 9.0])
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match='64'):
            reader.bag_similarity_topk(queries, rows, offsets, k)
    with pytest.raises(TypeError, match='integer'):
        reader.bag_similarity_topk(queries, rows, offsets, 2.5)
    assert reader.last_query_bags_kernel == '' and reader.last_query_bags_topk_kernel == ''
    for call in (lambda: reader.bag_similarity_matrix_device(None, np.zeros(1), None),
                 lambda: reader.bag_similarity_topk_device(None, np.zeros(1), None, 3),
                 lambda: reader.nearest_sentences_device([['a']], [['b']])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()
    with pytest.raises(ValueError, match='64'):
        reader.nearest_sentences_device([['a']], [['b']], k=65)
    with pytest.raises(ValueError, match='mode'):
        reader.nearest_sentences_device([['a']], [['b']], mode='max')


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_pooled.h"' in text and '#include "memb_hip_query_matrix.h"' in text
    for word in ("missing='skip'", 'chunked order', 'bf16 / fp16', 'ReadersUnion', 'ShardedReader', 'k > 64', 'bags on the query side'):
        assert word in text, word
    # the headers it extends do not know the new names
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_query_bags.h':
            assert 'query_bags' not in open(os.path.join(REPO, 'include', name)).read(), name


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    # (a null context is refused before anything else is looked at: the other refusals need a context, so a device, and
    # are exercised without one by tests/cpp/query_bags_planning_main.cpp)
    call = library.memb_hip_query_bags_device
    call.argtypes = [pointer, pointer, size, size, pointer, size, pointer, size, ctypes.c_int, pointer, pointer, size, pointer, pointer]
    assert refused(call(None, 64, 2, 300, 128, 9, 256, 3, 1, 512, None, 3, None, None), b'ctx')
    assert refused(call(None, None, 0, 0, None, 0, None, 0, 0, None, None, 0, None, None), b'ctx')
    topk = library.memb_hip_query_bags_topk_device
    topk.argtypes = [pointer, pointer, size, size, pointer, size, pointer, size, ctypes.c_int, ctypes.c_uint32, pointer, pointer, size,
                     pointer, size, pointer]
    assert refused(topk(None, 64, 2, 300, 128, 9, 256, 3, 1, 3, 512, 1024, 3, 2048, 1 << 20, None), b'ctx')
    workspace = library.memb_hip_query_bags_topk_workspace_bytes
    workspace.restype = size
    workspace.argtypes = [pointer, size, size, ctypes.c_uint32, ctypes.c_int]
    assert workspace(None, 2, 5, 3, 0) == 0
    for function in (library.memb_hip_query_bags_kernel_name, library.memb_hip_query_bags_topk_kernel_name):
        function.restype = ctypes.c_char_p
        function.argtypes = [pointer]
        assert function(None) == b''
    count = library.memb_hip_query_bags_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, pointer, size, size, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer]
    assert refused(count(None, None, 0, None, 0, 0, 1, 0, 0, None), b'null')
    assert refused(count(None, None, 0, None, 2 ** 36 + 1, 0, 1, 0, 0, None), b'too large')
    assert refused(count(None, None, 0, None, 0, 2 ** 16 + 1, 1, 0, 0, None), b'too large')

    from memb_amd import _memb
    for method in ('query_bags_to_device', 'query_bags_kernel_name', 'query_bags_algorithmic_bytes', 'query_bags_topk_to_device',
                   'query_bags_topk_workspace_bytes', 'query_bags_topk_kernel_name'):
        assert hasattr(_memb.Reader, method)
    assert _memb.QUERY_BAGS_GROUP == 2
    for method in ('bag_similarity_matrix_device', 'bag_similarity_topk_device', 'nearest_sentences_device', 'bag_similarity_matrix',
                   'bag_similarity_topk', 'last_query_bags_kernel', 'last_query_bags_topk_kernel'):
        assert hasattr(native.Reader, method)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_and_argument_checks_under_the_host_sanitizers(tmp_path):
    # hip_query_bags_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on
    # the HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'query_bags_planning_main.cpp')
    program = str(tmp_path / 'query_bags_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'query bags planning: ok' in run.stdout, run.stdout
