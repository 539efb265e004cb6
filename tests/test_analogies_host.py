"""Analogies without a GPU: the reference of tests/analogies_reference.py against two independent restatements
(torch.sort(stable, descending) followed by dropping the excluded positions, and the plain selection of k + E followed by the
stable-sort drop most_similar_device uses), the package's own numpy selection with `exclude` against it, a device='cpu'
reader's compose_queries, similarity_topk(exclude=), analogies and analogy against the composition of those pieces, the C
header and the entry points' refusals, and hip_analogies_launch.h's argument checks built into a program of their own under
the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from analogies_reference import drop_by_stable_sort, topk_excluding_by_the_contract, weighted_rows_sum_reference
from conftest import REPO
from pooled_reference import ids_with_misses
from query_topk_reference import rows_of_every_kind, same_topk, topk_by_the_contract

HEADER = os.path.join(REPO, 'include', 'memb_hip_analogies.h')
N_ROWS = 3000
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, 130)
RANKS = (1, 2, 10, 63, 64)


def every_kind(n):
    return np.stack([row for _, row in rows_of_every_kind(n)])


def lists_of_every_kind(matrix, width, base, seed):
    """(count, width) excluded positions: row 0 its own best `width`, row 1 all padding, the others random columns with
    repeats, a -1, and positions just outside the candidates"""
    count, n = matrix.shape
    rng = np.random.default_rng(seed)
    lists = base + rng.integers(0, n, size=(count, width)).astype(np.int64)
    best = topk_by_the_contract(matrix[:1], min(width, 64), base=base)[1][0]
    lists[0] = np.resize(best[best >= 0], width)
    lists[1] = -1
    if width >= 4 and count > 2:
        lists[2, :4] = (-1, base - 1, base + n, lists[2, 3])
        lists[2, 3] = lists[2, 4 % width]
    return lists


def test_the_reference_is_torch_stable_sort_without_the_excluded():
    import torch
    for n in SIZES:
        matrix = every_kind(n)
        ordered = torch.sort(torch.from_numpy(matrix), dim=1, descending=True, stable=True)
        for width in (0, 1, 3, 64):
            lists = lists_of_every_kind(matrix, width, 7, n + width)
            for k in RANKS:
                values, positions = topk_excluding_by_the_contract(matrix, k, lists, base=7)
                for q in range(matrix.shape[0]):
                    columns = [int(c) for c in ordered.indices[q] if 7 + int(c) not in set(lists[q].tolist())][:k]
                    assert positions[q, :len(columns)].tolist() == [7 + c for c in columns], (n, width, k, q)
                    assert (positions[q, len(columns):] == -1).all() and np.isneginf(values[q, len(columns):]).all()
                    assert np.array_equal(values[q, :len(columns)].view(np.uint32), matrix[q, columns].view(np.uint32))
                    assert len(columns) == min(k, n - len({c for c in lists[q].tolist() if 7 <= c < 7 + n})), (n, width, k, q)
    # by hand: the NaN at 2 and the 1.0 at 3 are no candidates; the rest keeps its order
    row = np.array([[0.0, -0.0, np.nan, 1.0, -np.inf, 1.0, np.nan]], dtype=np.float32)
    values, positions = topk_excluding_by_the_contract(row, 8, np.array([[3, 2, 3, -1, 7]]))
    assert positions.tolist() == [[6, 5, 0, 1, 4, -1, -1, -1]]


def test_the_reference_is_the_plain_selection_and_the_stable_sort_drop():
    for n in SIZES:
        matrix = every_kind(n)
        for width in (1, 3, 10):
            lists = lists_of_every_kind(matrix, width, 0, 3 * n + width)
            for k in (k for k in RANKS if k + width <= 64):
                wider = topk_by_the_contract(matrix, k + width)
                assert same_topk(drop_by_stable_sort(wider[0], wider[1], lists, k), topk_excluding_by_the_contract(matrix, k, lists)), (n, width, k)
        assert same_topk(topk_excluding_by_the_contract(matrix, 10, None), topk_by_the_contract(matrix, 10))
        assert same_topk(topk_excluding_by_the_contract(matrix, 10, np.full((matrix.shape[0], 5), -1)), topk_by_the_contract(matrix, 10))


def test_the_packages_host_selection_is_the_reference(native):
    from memb_amd.reader import topk_host
    for n in SIZES:
        matrix = every_kind(n)
        for width in (0, 1, 3, 64):
            lists = lists_of_every_kind(matrix, width, 5, 5 * n + width)
            for k in RANKS:
                want = topk_excluding_by_the_contract(matrix, k, lists, base=5)
                assert same_topk(topk_host(matrix, k, 5, exclude=lists), want), (n, width, k)
                # three slices merged forward and reversed, the list naming positions of all of them: the same bits
                cuts = [0, n // 3, n - n // 4, n]
                slices = [(cuts[i], cuts[i + 1]) for i in range(3)]
                for order in (slices, slices[::-1]):
                    held = None
                    for start, stop in order:
                        held = topk_host(matrix[:, start:stop], k, 5 + start, held, exclude=lists)
                    assert same_topk(held, want), (n, width, k, order)
        assert same_topk(topk_host(matrix, 10, 5, exclude=None), topk_by_the_contract(matrix, 10, base=5))


def test_the_packages_host_sum_is_the_reference(native):
    from memb_amd.reader import weighted_rows_sum_host
    rng = np.random.default_rng(3)
    matrix = rng.standard_normal((80, 7)).astype(np.float32)
    matrix[5] = 0
    offsets = np.array([0, 0, 1, 4, 74, 74, 80])
    weights = rng.choice(np.array([1, -1, 0.5, -0.0, 3.25e-3], dtype=np.float32), size=80)
    for given in (weights, None):
        got, want = weighted_rows_sum_host(matrix, given, offsets), weighted_rows_sum_reference(matrix, given, offsets)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not weighted_rows_sum_host(matrix, weights, offsets)[[0, 4]].view(np.uint32).any()   # no entry: +0.0
    assert weighted_rows_sum_host(matrix, None, [0]).shape == (0, 7)
    # not the fused multiply-add: the product is rounded before it is added
    a, b = np.float32(1 + 2.0 ** -13), np.float32(1 - 2.0 ** -13)   # (the product 1 - 2^-26 rounds to 1)
    pair = weighted_rows_sum_reference(np.array([[-1.0], [a]], dtype=np.float32), np.array([1, b], dtype=np.float32), [0, 2])
    assert pair[0, 0] == 0.0 and float(a) * float(b) - 1 != 0.0


@pytest.fixture(scope='module')
def host_reader(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    return native.Reader(path, device='cpu'), words


def test_host_reader_composes_queries(host_reader):
    reader, _ = host_reader
    rows = ids_with_misses(80, N_ROWS, 7)
    rows[2] = 0xFFFFFFFF
    offsets = np.array([0, 0, 1, 4, 74, 80])
    weights = np.random.default_rng(5).choice(np.array([1, -1, 0.5, -0.0], dtype=np.float32), size=80)
    unit = reader.unit_rows_embedding(rows)
    assert not unit[2].any()
    for given in (weights, None):
        got = reader.compose_queries(rows, offsets, given)
        assert got.shape == (5, 300) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), weighted_rows_sum_reference(unit, given, offsets).view(np.uint32))
    with pytest.raises(ValueError, match='offsets'):
        reader.compose_queries(rows, [0, 81])
    with pytest.raises(ValueError, match='weights'):
        reader.compose_queries(rows, offsets, weights[:79])


def test_host_reader_selects_without_the_excluded(host_reader, monkeypatch):
    import memb_amd.reader
    reader, _ = host_reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # bounded chunks: 53 candidates are four of them
    rows = ids_with_misses(53, N_ROWS, 7)
    rows[10:14] = rows[3] = 17                           # repeated ids: ties across chunks
    queries = np.random.default_rng(11).standard_normal((5, 300)).astype(np.float32)
    queries[2] = reader.rows_embedding(rows[3:4])[0]
    matrix = reader.similarity_matrix(queries, rows)
    for width in (0, 3, 64):
        lists = lists_of_every_kind(matrix, width, 0, width)
        if width == 3:
            lists[2] = (11, 3, 40)                       # among the tied best of query 2, in different chunks
        for k in (1, 10, 53, 64):
            got = reader.similarity_topk(queries, rows, k, exclude=lists)
            assert same_topk(got, topk_excluding_by_the_contract(matrix, k, lists)), (width, k)
    assert reader.similarity_topk(queries, rows, 4, exclude=np.array([[11, 3, 40]] * 5))[1][2].tolist() == [10, 12, 13] + [
        int(topk_excluding_by_the_contract(matrix[2:3], 4, [[3, 10, 11, 12, 13]])[1][0, 0])]
    with pytest.raises(TypeError, match='integer'):
        reader.similarity_topk(queries, rows, 3, exclude=np.zeros((5, 2), dtype=np.float32))
    with pytest.raises(ValueError, match='64'):
        reader.similarity_topk(queries, rows, 3, exclude=np.zeros((5, 65), dtype=np.int64))
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_topk(queries, rows, 3, exclude=np.zeros((4, 2), dtype=np.int64))


def test_host_reader_answers_analogies(host_reader):
    reader, words = host_reader
    vocabulary = reader.keys()
    a, b, c, d = words[5], words[17], words[40], words[99]
    positive = [[b, c], [(b, 0.5), c, (d, 2.0)], [a], [b, 'no such word é'], [], [c, c]]
    negative = [[a], [(a, -0.25), d], [], [a], [], []]
    got = reader.analogies(positive, negative, k=7)
    # the pieces: the entries in order, their unit rows summed, the top-k of the whole model without the query's rows
    flat = [[b, c, a], [b, c, d, a, d], [a], None, None, [c, c]]
    weights = [[1, 1, -1], [0.5, 1, 2.0, -0.25, -1], [1], None, None, [1, 1]]
    everything = np.arange(N_ROWS, dtype=np.uint32)
    for q, entries in enumerate(flat):
        if entries is None:
            assert got[q] == []
            continue
        own = reader.resolve_rows(entries)
        query = weighted_rows_sum_reference(reader.unit_rows_embedding(own), np.array(weights[q], dtype=np.float32), [0, len(entries)])
        matrix = reader.similarity_matrix(query, everything)
        values, positions = topk_excluding_by_the_contract(matrix, 7, [own.astype(np.int64)])
        assert got[q] == [(vocabulary[row], float(value)) for value, row in zip(values[0], positions[0])], q
        assert len(got[q]) == 7 and not {word for word, _ in got[q]} & set(entries)
    assert reader.analogy(a, b, c, k=7) == got[0] and reader.analogy(a, b, c) == got[0][:1]
    assert reader.analogies([[b, c]], k=3) == reader.analogies([[b, c]], None, 3) == reader.analogies([[b, c]], [[]], 3)
    assert reader.analogies([], [], 3) == []
    assert len(reader.analogies([[b, c]], [[a]], k=64)[0]) == 64   # nothing reserved for the three dropped words
    with pytest.raises(ValueError, match='64'):
        reader.analogies([[a] * 40], [[b] * 25], 3)
    assert len(reader.analogies([[a] * 40], [[b] * 24], 3)[0]) == 3
    with pytest.raises(ValueError, match='64'):
        reader.analogies([[a]], k=65)
    with pytest.raises(ValueError, match='one list per query'):
        reader.analogies([[a], [b]], [[c]])
    with pytest.raises(ValueError, match='63'):
        reader.most_similar([a], k=64)   # (as it was)
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.analogies_device([[a]])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.compose_queries_device(None, None)


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert 'NOT CANDIDATES' in text and '#define MEMB_HIP_MAX_EXCLUDED 64' in text
    for word in ('3CosMul', 'more than 64 exclusions', 'top-k over pooled bags', 'ReadersUnion', 'sharded readers',
                 'bf16 / fp16', 'k > 64', 'fused with the decode'):
        assert word in text, word
    # no older header knows the new names
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_analogies.h':
            older = open(os.path.join(REPO, 'include', name)).read()
            assert 'excluding' not in older and 'weighted_rows_sum' not in older and 'analogies' not in older, name


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    dense = library.memb_hip_dense_excluding_topk_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int, pointer, size, size,
                      pointer, pointer, size, pointer, size, pointer]
    # (every one of these is refused before a pointer is read or the device is touched)
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 1024, 65, 65, 128, 256, 3, 512, 1 << 20, None), b'at most 64')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 1024, 3, 2, 128, 256, 3, 512, 1 << 20, None), b'ld_excluded')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, None, 3, 3, 128, 256, 3, 512, 1 << 20, None), b'null')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 1028, 3, 3, 128, 256, 3, 512, 1 << 20, None), b'aligned')
    # its sibling's refusals behind them
    assert refused(dense(0, 64, 2, 5, 5, 0, 65, 0, 1024, 3, 3, 128, 256, 65, 512, 1 << 20, None), b'k must')
    assert refused(dense(0, 64, 2, 5, 4, 0, 3, 0, None, 0, 0, 128, 256, 3, 512, 1 << 20, None), b'ld must')
    assert refused(dense(0, 64, 2, 5, 5, 0, 3, 0, 1024, 3, 3, 128, 256, 3, 512, 47, None), b'workspace')
    assert dense(0, None, 0, 0, 0, 0, 3, 0, None, 0, 0, 128, 256, 3, None, 0, None) == 0   # no rows: a no-op, nothing touched
    fused = library.memb_hip_query_excluding_topk_device
    fused.argtypes = [pointer, pointer, size, size, pointer, size, ctypes.c_uint32, pointer, size, size, pointer, pointer, size,
                      pointer, size, pointer]
    assert refused(fused(None, 64, 2, 300, 128, 5, 3, 1024, 65, 65, 256, 512, 3, 2048, 1 << 20, None), b'at most 64')
    assert refused(fused(None, 64, 2, 300, 128, 5, 3, 1024, 3, 2, 256, 512, 3, 2048, 1 << 20, None), b'ld_excluded')
    assert refused(fused(None, 64, 2, 300, 128, 5, 3, None, 1, 1, 256, 512, 3, 2048, 1 << 20, None), b'null')
    assert refused(fused(None, 64, 2, 300, 128, 5, 3, 1026, 1, 1, 256, 512, 3, 2048, 1 << 20, None), b'aligned')
    assert refused(fused(None, 64, 2, 300, 128, 5, 3, None, 0, 0, 256, 512, 3, 2048, 1 << 20, None), b'ctx')
    name = library.memb_hip_query_excluding_topk_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b'topk_select_excluding+topk_merge'
    sums = library.memb_hip_weighted_rows_sum_device
    sums.argtypes = [ctypes.c_int, pointer, size, pointer, pointer, size, size, pointer, size, pointer]
    assert refused(sums(-1, 64, 8, None, 128, 2, 7, 256, 8, None), b'device')
    assert refused(sums(0, 64, 8, None, None, 2, 7, 256, 8, None), b'null')
    assert refused(sums(0, 64, 8, None, 128, 2, 7, None, 8, None), b'null')
    assert refused(sums(0, 64, 6, None, 128, 2, 7, 256, 8, None), b'at least dim')
    assert refused(sums(0, 64, 8, None, 128, 2, 7, 256, 6, None), b'at least dim')
    assert refused(sums(0, 66, 8, None, 128, 2, 7, 256, 8, None), b'aligned')
    assert refused(sums(0, 64, 8, None, 128, 2 ** 24 + 1, 7, 256, 8, None), b'too large')
    assert sums(0, None, 8, None, 128, 0, 7, 256, 8, None) == 0  # no sums: a no-op, nothing touched

    import memb_amd
    from memb_amd import _memb
    for method in ('query_topk_excluding_to_device', 'query_topk_excluding_kernel_name'):
        assert hasattr(_memb.Reader, method)
    assert hasattr(_memb, 'dense_topk_excluding_to_device') and hasattr(_memb, 'weighted_rows_sum_to_device')
    assert memb_amd.QUERY_TOPK_MAX_EXCLUDED == _memb.QUERY_TOPK_MAX_EXCLUDED == 64
    assert _memb.dense_topk_excluding_kernel_name() == 'topk_select_excluding+topk_merge'
    for method in ('compose_queries_device', 'compose_queries', 'analogies_device', 'analogies', 'analogy'):
        assert hasattr(native.Reader, method)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_argument_checks_under_the_host_sanitizers(tmp_path):
    # hip_analogies_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on the
    # HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'analogies_planning_main.cpp')
    program = str(tmp_path / 'analogies_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'analogies planning: ok' in run.stdout, run.stdout
