"""Cosine similarity of query vectors against groups of candidate rows without a GPU: the two restatements of the
reference of tests/queries_reference.py against each other, the reference against float64, a device='cpu' reader bit for
bit against it (include/memb_hip_queries.h's contract over reader.rows_embedding), the argument checks, the C header and
the entry points' refusals, and hip_queries_launch.h's planning and argument checks built into a program of their own under
the host sanitizers. (memb_hip_query_algorithmic_bytes needs a context, which exists only for a staged model: the call's
count is checked in tests/test_gpu_queries.py, as the pair and bag-pair counts are; the half that needs none -- the entries
that lie in a group and the header's formula over them, by hand -- is checked here by the stand-alone program.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from pooled_reference import offsets_of
from queries_reference import (LONG_GROUP, group_lengths, groups_of_entries, queries_by_the_contract, queries_entry_by_entry,
                               query_batch)

HEADER = os.path.join(REPO, 'include', 'memb_hip_queries.h')
N_ROWS = 3000
GROUPS = 40
ACCURACY_DIMS = (1, 3, 4, 64, 255, 256, 260, 300, 512, 516, 1024)
# tests/test_pairs_host.py asserts 2^-20 absolute for the pair contract against float64 on Gaussian rows; this is the same
# arithmetic over (query, row), so the same figure is asserted.
ACCURACY_BOUND = 2.0 ** -20


def entry_values(reader, rows):
    rows = np.asarray(rows, dtype=np.uint32)
    return reader.rows_embedding(rows) if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)


def test_the_batch_holds_its_edges():
    for words in (1, 2, 4, 7, 21, 64):
        lengths = group_lengths(words, GROUPS, 3)
        offsets = offsets_of(lengths)
        assert len(lengths) == GROUPS and lengths[0] == 0 and lengths[-1] == 0
        assert {0, 1, max(words - 1, 1), words, words + 1, 3 * words + 1, LONG_GROUP} <= set(lengths.tolist())
        assert any((lengths[k:k + 3] == 0).all() and lengths[k - 1] > 0 and lengths[k + 3] > 0 for k in range(1, GROUPS - 4))
        if words > 1:
            assert (offsets[1:-1] % words != 0).any()   # group ends inside tiles
        queries, rows, again = query_batch(words, GROUPS, 300, N_ROWS, 3, head=5, tail=9)
        assert np.array_equal(again, offsets + 5) and len(rows) == again[-1] + 9 and (rows >= N_ROWS).any()
        assert queries.shape == (GROUPS, 300) and queries.dtype == np.float32
    for groups in (0, 1, 2, 3):
        queries, rows, offsets = query_batch(4, groups, 8, N_ROWS, 1)
        assert len(offsets) == groups + 1 and len(rows) == offsets[-1] and len(queries) == groups
    group, inside = groups_of_entries([2, 2, 5, 5, 7], 9)
    assert group[inside].tolist() == [1, 1, 1, 3, 3] and inside.tolist() == [False] * 2 + [True] * 5 + [False] * 2


def test_the_two_restatements_agree():
    for dim, words in ((4, 16), (7, 4), (260, 4), (300, 1), (516, 2)):
        queries, rows, offsets = query_batch(words, 9, dim, N_ROWS, dim, head=2, tail=3)
        rng = np.random.default_rng(dim)
        values = rng.standard_normal((len(rows), dim)).astype(np.float32)
        values[rows >= N_ROWS] = 0
        values[5] = -0.0
        queries[1, : dim // 2] = 0
        matrix = queries_by_the_contract(queries, values, offsets)
        scalar = queries_entry_by_entry(queries, values, offsets)
        assert np.array_equal(matrix[3], scalar[3]) and not matrix[3][:2].any() and not matrix[3][-3:].any()
        assert all(bits_equal(one, other) for one, other in zip(matrix[:3], scalar[:3])), dim
        assert not matrix[0][~matrix[3]].any() and (matrix[0] != 0).any()


def test_reference_is_close_to_float64():
    worst_of_all = 0.0
    for dim in ACCURACY_DIMS:
        rng = np.random.default_rng(3000 + dim)
        groups, per_group = 20, 25
        queries = rng.standard_normal((groups, dim)).astype(np.float32)
        values = rng.standard_normal((groups * per_group, dim)).astype(np.float32)
        # the first candidate of every group is nearly the query, so that cosines near 1 are among them
        values[::per_group] = queries + np.float32(0.01) * values[::per_group]
        offsets = offsets_of([per_group] * groups)
        cosines, _, _, inside = queries_by_the_contract(queries, values, offsets)
        assert inside.all()
        x = np.repeat(queries, per_group, axis=0).astype(np.float64)
        y = values.astype(np.float64)
        exact = (x * y).sum(axis=1) / (np.sqrt((x * x).sum(axis=1)) * np.sqrt((y * y).sum(axis=1)))
        worst = float(np.abs(cosines.astype(np.float64) - exact).max())
        print('dim', dim, 'worst |cos - cos64| =', worst / 2.0 ** -24, '* 2^-24')
        worst_of_all = max(worst_of_all, worst)
        assert worst <= ACCURACY_BOUND, (dim, worst)
        assert np.abs(cosines).max() <= 1 + 2.0 ** -22 and np.abs(cosines).max() > 0.99
    print('worst of all =', worst_of_all / 2.0 ** -24, '* 2^-24')


# ---- a device='cpu' reader ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_host_reader_has_the_contracts_bits(native, make_model, storage, bits):
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    # grouped batches, with entries in front of the first group and behind the last
    for head, tail in ((0, 0), (3, 6)):
        queries, rows, offsets = query_batch(4, GROUPS, 300, N_ROWS, 11, head=head, tail=tail)
        rows[int(offsets[2])] %= N_ROWS   # a row against itself
        queries[2] = reader.rows_embedding(rows[int(offsets[2]):int(offsets[2]) + 1])[0]
        n = len(rows)
        want = queries_by_the_contract(queries, entry_values(reader, rows), offsets)
        assert abs(float(want[0][int(offsets[2])]) - 1) <= 2.0 ** -22 and want[3].sum() == n - head - tail
        cosines = reader.query_similarity(queries, rows, offsets)
        assert isinstance(cosines, np.ndarray) and cosines.dtype == np.float32 and cosines.shape == (n,)
        assert bits_equal(cosines, want[0]), (storage, head)
        for dots, norms in ((True, False), (False, True), (True, True)):
            got = reader.query_similarity(queries, rows, offsets, return_dots=dots, return_norms=norms)
            assert len(got) == 3 and bits_equal(got[0], want[0]), (storage, dots, norms)
            assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms)
            if dots:
                assert got[1].dtype == np.float32 and got[1].shape == (n,) and bits_equal(got[1], want[1])
            if norms:
                query_norms, row_norms = got[2]
                assert row_norms.dtype == np.float32 and row_norms.shape == (n,) and bits_equal(row_norms, want[2])
                assert query_norms.shape == (GROUPS,) and bits_equal(query_norms, _norms(queries))
                inside = want[3]
                assert bits_equal(row_norms[inside], reader.row_norms(rows[inside]))
        assert not np.isnan(cosines).any()
    # offsets=None: one query against all rows, (dim,) or (1, dim)
    rows = query_batch(4, 5, 300, N_ROWS, 2)[1]
    query = np.random.default_rng(5).standard_normal(300).astype(np.float32)
    want = queries_by_the_contract(query[None, :], entry_values(reader, rows), [0, len(rows)])
    assert bits_equal(reader.query_similarity(query, rows), want[0])
    assert bits_equal(reader.query_similarity(query[None, :], rows, return_dots=True)[1], want[1])
    assert bits_equal(reader.query_similarity(query, rows, [0, len(rows)]), want[0])


def _norms(queries):
    from norms_reference import norms_by_the_contract
    return norms_by_the_contract(queries)


def test_host_reader_works_in_bounded_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    queries, rows, offsets = query_batch(4, 15, 300, N_ROWS, 9, head=20, tail=3)
    want = queries_by_the_contract(queries, entry_values(reader, rows), offsets)
    got = reader.query_similarity(queries, rows, offsets, return_dots=True, return_norms=True)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and bits_equal(got[2][1], want[2])


def test_argument_checks_raise(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    queries, rows, offsets = query_batch(4, 7, 300, N_ROWS, 5)
    want = queries_by_the_contract(queries, entry_values(reader, rows), offsets)
    for given in (offsets, offsets.astype(np.uint32), offsets.astype(np.int32), [int(value) for value in offsets]):
        assert bits_equal(reader.query_similarity(queries, rows, given), want[0])
    with pytest.raises(TypeError, match='float32'):
        reader.query_similarity(queries.astype(np.float64), rows, offsets)               # wrong dtype
    with pytest.raises(ValueError, match='shape'):
        reader.query_similarity(queries[:, :296], rows, offsets)                         # wrong dim
    with pytest.raises(ValueError, match='shape'):
        reader.query_similarity(queries[None], rows, offsets)                            # three dimensions
    with pytest.raises(ValueError, match='G \\+ 1'):
        reader.query_similarity(queries, rows, offsets[:-1])                             # offsets of another G
    with pytest.raises(ValueError, match='one query'):
        reader.query_similarity(queries, rows)                                           # offsets=None with G > 1
    with pytest.raises(ValueError, match='ascend'):
        reader.query_similarity(queries, rows, offsets[::-1].copy())
    with pytest.raises(ValueError, match='len\\(rows\\)'):
        reader.query_similarity(queries, rows, offsets + 1)
    # no group, no entry
    none = np.zeros(0, dtype=np.uint32)
    assert reader.query_similarity(queries[:0], none, [0]).shape == (0,)
    assert reader.query_similarity(queries[:0], rows, [0]).tolist() == [0.0] * len(rows)
    empty = reader.query_similarity(queries[:2], none, [0, 0, 0], return_dots=True, return_norms=True)
    assert empty[0].shape == (0,) and empty[2][0].shape == (2,) and empty[2][1].shape == (0,)
    # device methods refuse a host reader before anything else
    assert reader.last_query_kernel == ''
    for call in (lambda: reader.query_similarity_device(None, None), lambda: reader.candidates_similarity_device(['a'], [['b']])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()
    with pytest.raises(ValueError, match='one list of candidates per word'):
        reader.candidates_similarity_device(['a', 'b'], [['c']])


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_pairs.h"' in text
    # the sentence that is both the fallback and the second oracle, and what is not built
    assert 'decode the candidates, put query and row next to each other' in text and 'memb_hip_dense_pair_similarity_device' in text
    for word in ('top-k', 'shared candidate', 'bf16 / fp16', 'ReadersUnion', 'sharded readers', 'uniform or full', 'chunked order'):
        assert word in text, word
    # the headers it extends are as they were
    for name in ('memb_hip.h', 'memb_hip_pooled.h', 'memb_hip_pairs.h', 'memb_hip_norms.h', 'memb_hip_bag_pairs.h'):
        assert 'memb_hip_query' not in open(os.path.join(REPO, 'include', name)).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    # (without a context every call is refused before any pointer is read: the refusals that need one are checked with a
    # staged model in tests/test_gpu_queries.py, and by the stand-alone program below)
    call = library.memb_hip_query_similarity_device
    call.argtypes = [pointer, pointer, size, size, pointer, size, pointer, pointer, pointer, pointer, pointer]
    assert refused(call(None, 64, 2, 300, 128, 5, 256, 512, None, None, None), b'ctx')
    assert refused(call(None, None, 0, 0, None, 0, None, None, None, None, None), b'ctx')
    name = library.memb_hip_query_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b''
    count = library.memb_hip_query_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, pointer, size, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer]
    assert refused(count(None, None, 0, None, 0, 1, 0, 0, None), b'null')
    assert refused(count(None, None, 0, None, 2 ** 32 - 1, 1, 0, 0, None), b'too large')
    assert refused(count(None, None, 2 ** 36 + 1, None, 1, 1, 0, 0, None), b'too large')

    from memb_amd import _memb
    for method in ('query_similarity_to_device', 'query_kernel_name', 'query_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    for method in ('query_similarity_device', 'candidates_similarity_device', 'query_similarity', 'last_query_kernel'):
        assert hasattr(native.Reader, method)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_and_argument_checks_under_the_host_sanitizers(tmp_path):
    # hip_queries_launch.h's first part -- what a call is refused for, the grid and its actual values, the entries that lie
    # in a group, the byte count's formula by hand -- as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on the HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'queries_planning_main.cpp')
    program = str(tmp_path / 'queries_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'queries planning: ok' in run.stdout, run.stdout
