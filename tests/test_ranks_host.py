"""The rank counts without a GPU: the package's numpy form against the brute-force restatement of tests/ranks_reference.py
on hostile matrices, every kind of mark and list of non-candidates, slices in shuffled order, the slot the selection gives
the same candidate, a device='cpu' reader's rank, count_closer_than, analogy_ranks and evaluate_analogies against answers
worked out by hand, the argument errors, the C header and the entry points' refusals, and hip_ranks_launch.h's planning
built into a program of its own under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from ranks_reference import INT64_MAX, hostile_matrix, key_of, marks_over, ranks_by_the_contract

HEADER = os.path.join(REPO, 'include', 'memb_hip_ranks.h')
FUSED = 'query_matrix_trained+rank_count+rank_fold'


def test_the_restatement_by_hand():
    row = np.array([[0.5, np.nan, 0.5, -0.0, 0.0, -np.inf, 0.5, np.inf]], dtype=np.float32)
    half, zero = np.float32([0.5]), np.float32([0.0])
    assert ranks_by_the_contract(row, half, [-1]).tolist() == [2]            # NaN and +inf are greater
    assert ranks_by_the_contract(row, half, [INT64_MAX]).tolist() == [5]     # and three are equal
    assert ranks_by_the_contract(row, half, [2]).tolist() == [3]             # column 2 is the second of the equals
    assert ranks_by_the_contract(row, half, [3]).tolist() == [4]             # the mark need not be a candidate of that value
    assert ranks_by_the_contract(row, zero, [4]).tolist() == [6]             # -0.0 at 3 ties with +0.0 at 4 and comes first
    assert ranks_by_the_contract(row, np.float32([-0.0]), [3]).tolist() == [5]
    assert ranks_by_the_contract(row, np.float32([np.nan]), [INT64_MAX]).tolist() == [1]
    assert ranks_by_the_contract(row, np.float32([np.nan]), [1]).tolist() == [0]
    assert ranks_by_the_contract(row, half, [2], exclude=[[0, 0, 1, -1, 99]]).tolist() == [1]
    assert ranks_by_the_contract(row, half, [12], base=10).tolist() == [3]
    assert key_of(-0.0) == key_of(0.0) and key_of(np.nan) > key_of(np.inf) > key_of(1.0) > key_of(-1.0) > key_of(-np.inf) > 0


@pytest.mark.parametrize('count,n', [(1, 1), (3, 63), (17, 300), (8, 1000)])
def test_the_packages_host_counts_are_the_restatement(native, count, n):
    from memb_amd.reader import ranks_host
    matrix = hostile_matrix(count, n, seed=7 * count + n)
    for base in (0, 1000):
        thresholds, marks = marks_over(matrix, seed=n, base=base)
        want = ranks_by_the_contract(matrix, thresholds, marks, base)
        got = ranks_host(matrix, thresholds, marks, base)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), (count, n, base)
        # lists with repeats, -1 padding, entries out of range on both sides, and the mark itself
        rng = np.random.default_rng(n)
        lists = base + rng.integers(0, n, size=(count, 9)).astype(np.int64)
        lists[:, 3] = lists[:, 0]
        lists[:, 4] = -1
        lists[:, 5] = base + n + rng.integers(0, 5, size=count)
        lists[:, 6] = base - 1 - rng.integers(0, 5, size=count)
        lists[:, 7] = np.clip(marks, -1, base + n)
        assert ranks_host(matrix, thresholds, marks, base, lists).tolist() == ranks_by_the_contract(matrix, thresholds, marks, base, lists).tolist()
    assert ranks_host(matrix, thresholds[:count], None).tolist() == ranks_by_the_contract(matrix, thresholds, np.full(count, -1)).tolist()
    assert ranks_host(matrix[:, :0], thresholds, marks).tolist() == [0] * count and ranks_host(matrix[:0], thresholds[:0], marks[:0]).shape == (0,)


def test_slices_in_any_order_add_up(native):
    from memb_amd.reader import ranks_host
    matrix = hostile_matrix(5, 700, seed=3)
    thresholds, marks = marks_over(matrix, seed=4)
    lists = np.random.default_rng(5).integers(-3, 710, size=(5, 12)).astype(np.int64)
    whole = ranks_host(matrix, thresholds, marks, 0, lists)
    assert whole.tolist() == ranks_by_the_contract(matrix, thresholds, marks, 0, lists).tolist()
    cuts = [0, 1, 64, 65, 300, 699, 700]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    np.random.default_rng(6).shuffle(pieces)
    total = np.zeros(5, dtype=np.int64)
    for start, stop in pieces:
        total += ranks_host(matrix[:, start:stop], thresholds, marks, start, lists)
    assert total.tolist() == whole.tolist()


def test_a_rank_is_the_slot_of_the_selection(native):
    from memb_amd.reader import ranks_host, topk_host
    matrix = hostile_matrix(24, 400, seed=11)
    matrix[:, :80] = np.nan                                 # the best 64 and more are ties: the position decides
    matrix[5:9, 10:20] = np.inf                             # (ten of them fall behind every NaN of their row)
    rng = np.random.default_rng(12)
    lists = rng.integers(-1, 400, size=(24, 6)).astype(np.int64)
    columns = rng.integers(0, 120, size=24)
    columns = np.where((lists == columns[:, None]).any(axis=1), 399, columns)   # (a non-candidate has no slot)
    lists[lists == 399] = -1
    thresholds = matrix[np.arange(24), columns]
    for exclude in (None, lists):
        ranks = ranks_host(matrix, thresholds, columns.astype(np.int64), 0, exclude)
        positions = topk_host(matrix, 64, exclude=exclude)[1]
        below = np.nonzero(ranks < 64)[0]
        assert below.size >= 8 and (ranks >= 64).any()
        assert (positions[below, ranks[below]] == columns[below]).all()


# ---- a device='cpu' reader ----

@pytest.fixture(scope='module')
def royal(native, tmp_path_factory):
    # axes: royal, male, female, other
    vectors = {'king': (1, 1, 0, 0), 'queen': (1, 0, 1, 0), 'man': (0, 1, 0, 0), 'woman': (0, 0, 1, 0), 'prince': (1, 1, 0, 0.5),
               'apple': (0, 0, 0, 1), 'girl': (0, 0.1, 1, 0.3)}
    builder = native.Builder(4, 'full', 32)
    builder.add_words(list(vectors), np.array(list(vectors.values()), dtype=np.float32))
    path = str(tmp_path_factory.mktemp('royal') / 'royal.bin')
    builder.save(path)
    return native.Reader(path, device='cpu')


def test_ranks_worked_out_by_hand(royal):
    reader = royal
    # around king (1, 1, 0, 0): prince 0.943, man 0.707, queen 0.5, girl 0.067, apple and woman 0 -- apple sorts before
    # woman as a word, so it has the lower row and comes first among the two equals
    assert [word for word, _ in reader.most_similar(['king'], k=6)[0]] == ['prince', 'man', 'queen', 'girl', 'apple', 'woman']
    words = ['prince', 'man', 'queen', 'girl', 'apple', 'woman']
    assert reader.rank(['king'] * 6, words).tolist() == [1, 2, 3, 4, 5, 6]
    assert reader.count_closer_than(['king'] * 6, words).tolist() == [0, 1, 2, 3, 4, 5]
    assert reader.rank(['king'], ['king']).tolist() == [1]                       # nothing but itself is as close, and it is no candidate
    assert reader.rank(['king', 'nobody', 'king'], ['queen', 'queen', 'nobody']).tolist() == [3, 0, 0]
    assert reader.count_closer_than(['nobody'], ['queen']).tolist() == [-1]
    assert reader.rank([], []).shape == (0,)
    with pytest.raises(ValueError, match='one word per pair'):
        reader.rank(['king'], [])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.rank_device(['king'], ['queen'])
    # king - man + woman (tests/test_analogies_host.py: queen, girl, prince, apple is the order of the answers)
    assert [word for word, _ in reader.analogy('man', 'king', 'woman', k=4)] == ['queen', 'girl', 'prince', 'apple']
    positive, negative = [['king', 'woman']] * 6, [['man']] * 6
    expected = ['queen', 'girl', 'prince', 'apple', 'nobody', 'king']
    ranks = reader.analogy_ranks(positive, negative, expected)
    assert ranks[:5].tolist() == [1, 2, 3, 4, 0]
    assert ranks[5] >= 1                                                         # an own word as the expected one: it is left out, the count stands
    assert reader.analogy_ranks([['king', 'nobody']], [['man']], ['queen']).tolist() == [0]
    assert reader.analogy_ranks([[]], None, ['queen']).tolist() == [0] and reader.analogy_ranks([], [], []).shape == (0,)
    with pytest.raises(ValueError, match='one word per question'):
        reader.analogy_ranks(positive, negative, expected[:2])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.analogy_ranks_device(positive, negative, expected)
    result = reader.evaluate_analogies([('man', 'king', 'woman', 'queen'), ('man', 'king', 'woman', 'prince'),
                                        ('man', 'king', 'woman', 'nobody'), ('man', 'king', 'woman', 'girl')])
    assert result == {'questions': 4, 'answered': 3, 'accuracy': 1 / 3, 'mean_reciprocal_rank': (1 + 1 / 3 + 1 / 2) / 3}
    assert reader.evaluate_analogies([]) == {'questions': 0, 'answered': 0, 'accuracy': 0.0, 'mean_reciprocal_rank': 0.0}
    with pytest.raises(ValueError, match='expected'):
        reader.evaluate_analogies([('man', 'king', 'woman')])
    assert reader.last_ranks_kernel == ''


def test_host_reader_counts_over_chunks(native, make_model, monkeypatch):
    import memb_amd.reader
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # bounded chunks: 53 candidates are four of them
    rows = np.random.default_rng(21).integers(0, 3000, size=53).astype(np.uint32)
    rows[10:14] = rows[3] = 17                                      # repeated ids: bit-equal cosines in different chunks
    queries = reader.unit_rows_embedding(np.array([17, 5, 900], dtype=np.uint32))
    matrix = reader.similarity_matrix(queries, rows)
    thresholds = matrix[:, 12].copy()
    marks = np.array([12, -1, INT64_MAX], dtype=np.int64)
    lists = np.array([[11, 3, 40], [-1, 0, 0], [52, 99, 12]], dtype=np.int64)
    for exclude in (None, lists):
        got = reader.similarity_ranks(queries, rows, thresholds, marks, exclude=exclude)
        assert got.tolist() == ranks_by_the_contract(matrix, thresholds, marks, 0, exclude).tolist()
    assert reader.similarity_ranks(queries, rows, thresholds, marks)[0] == 3              # 3, 10 and 11 tie with 12 and come first
    assert reader.similarity_ranks(queries, rows, thresholds, marks, exclude=lists)[0] == 1
    assert reader.similarity_ranks(queries, rows, thresholds).tolist() == ranks_by_the_contract(matrix, thresholds, [-1] * 3).tolist()
    assert reader.similarity_ranks(queries, rows[:0], thresholds, marks).tolist() == [0, 0, 0]
    with pytest.raises(TypeError, match='float32'):
        reader.similarity_ranks(queries.astype(np.float64), rows, thresholds)
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_ranks(queries[:, :299], rows, thresholds)
    with pytest.raises(TypeError, match='thresholds'):
        reader.similarity_ranks(queries, rows, thresholds.astype(np.float64))
    with pytest.raises(ValueError, match='thresholds'):
        reader.similarity_ranks(queries, rows, thresholds[:2])
    with pytest.raises(TypeError, match='marks'):
        reader.similarity_ranks(queries, rows, thresholds, marks.astype(np.float32))
    with pytest.raises(ValueError, match='marks'):
        reader.similarity_ranks(queries, rows, thresholds, marks[:2])
    with pytest.raises(ValueError, match='64'):
        reader.similarity_ranks(queries, rows, thresholds, marks, exclude=np.zeros((3, 65), dtype=np.int64))
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_ranks(queries, rows, thresholds, marks, exclude=lists[:2])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.similarity_ranks_device(None, None, None)


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_query_matrix.h"' in text
    for word in ('p_q = -1', 'p_q = INT64_MAX', '0-based rank', 'stable', 'depends on the inputs alone'):
        assert word in text, word
    not_built = text[text.index('Not built:'):]
    for word in ('closer_than', 'beyond 64', 'ReadersUnion', 'ShardedReader', 'bf16 / fp16', 'pooled-bag', '3CosMul'):
        assert word in not_built, word
    # the names the older headers' tests keep to their own header
    for word in ('query_topk', 'dense_topk', 'TOPK', 'query_bags', 'excluding', 'weighted_rows_sum', 'analogies',
                 'memb_hip_cosmul', 'cosmul_scores', 'COSMUL'):
        assert word not in text, word
    # no older header knows the new names
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_ranks.h':
            older = open(os.path.join(REPO, 'include', name)).read()
            assert 'memb_hip_ranks' not in older and 'rank_count' not in older, name


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    dense = library.memb_hip_dense_ranks_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, ctypes.c_int64, pointer, pointer, pointer, size, size, ctypes.c_int,
                      pointer, pointer, size, pointer]
    good = dict(device=0, matrix=64, n_rows=2, n=7, ld=8, base=0, thresholds=128, marks=256, excluded=512, width=3, ld_excluded=3,
                accumulate=0, counts=1024, workspace=2048, workspace_bytes=64, stream=None)

    def call(**changes):
        return dense(*dict(good, **changes).values())

    # (every one of these is refused before a pointer is read or the device is touched)
    assert refused(call(device=-1), b'device')
    assert refused(call(base=-1), b'base')
    assert refused(call(matrix=None), b'matrix')
    assert refused(call(ld=6), b'at least n')
    for name in ('thresholds', 'marks', 'counts'):
        assert refused(call(**{name: None}), b'null'), name
    assert refused(call(matrix=66), b'aligned') and refused(call(thresholds=130), b'aligned')
    for name in ('marks', 'counts', 'excluded', 'workspace'):
        assert refused(call(**{name: good[name] + 4}), b'aligned'), name
    assert refused(call(width=65, ld_excluded=65), b'at most 64')
    assert refused(call(ld_excluded=2), b'ld_excluded')
    assert refused(call(excluded=None), b'excluded')
    assert refused(call(n_rows=2 ** 16 + 1), b'too large')
    assert refused(call(n=2 ** 31 + 1, ld=2 ** 32), b'too large')
    assert refused(call(workspace=None), b'workspace') and refused(call(workspace_bytes=7), b'workspace too small')
    assert call(n_rows=0) == 0                                        # no row: a no-op, nothing touched
    assert call(n=0, matrix=None, accumulate=1, workspace=None, workspace_bytes=0) == 0   # no column under accumulate: counts stay
    dense_bytes = library.memb_hip_dense_ranks_workspace_bytes
    dense_bytes.restype = size
    dense_bytes.argtypes = [size, size]
    assert dense_bytes(2, 7) == 8 and dense_bytes(3, 2049) == 24 and dense_bytes(1, 2048) == 8 and dense_bytes(5, 0) == 0
    assert dense_bytes(2 ** 16 + 1, 7) == 0 and dense_bytes(2, 2 ** 31 + 1) == 0
    fused = library.memb_hip_query_ranks_device
    fused.argtypes = [pointer, pointer, size, size, pointer, size, pointer, pointer, pointer, size, size, pointer, pointer, size, pointer]
    assert refused(fused(None, 64, 3, 300, 128, 5, 256, 512, None, 0, 0, 1024, 2048, 1 << 20, None), b'ctx')
    size_of = library.memb_hip_query_ranks_workspace_bytes
    size_of.restype = size
    size_of.argtypes = [pointer, size, size, ctypes.c_int]
    assert size_of(None, 3, 1000, 0) == 0
    name = library.memb_hip_query_ranks_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b'rank_count+rank_fold'

    import memb_amd
    from memb_amd import _memb, _memb_ranks
    # the bindings: a module of its own, by context handle; a reader on the host has no context
    for entry in ('dense_ranks_to_device', 'dense_ranks_workspace_bytes', 'query_ranks_to_device', 'query_ranks_workspace_bytes',
                  'query_ranks_kernel_name'):
        assert callable(getattr(_memb_ranks, entry)), entry
    assert _memb_ranks.dense_ranks_kernel_name() == 'rank_count+rank_fold' and _memb_ranks.dense_ranks_workspace_bytes(2, 7) == 8
    assert _memb_ranks.query_ranks_kernel_name(0) == '' and _memb_ranks.query_ranks_workspace_bytes(0, 3, 1000) == 0
    with pytest.raises(RuntimeError, match='memb_hip_query_ranks_device.*ctx'):
        _memb_ranks.query_ranks_to_device(0, 64, 3, 300, 128, 5, 256, 512, 0, 0, 0, 1024, 2048, 1 << 20)
    with pytest.raises(RuntimeError, match='memb_hip_dense_ranks_device.*device'):
        _memb_ranks.dense_ranks_to_device(-1, 64, 2, 7, 8, 0, 128, 256, 0, 0, 0, False, 1024, 2048, 64)
    assert not [entry for entry in dir(_memb) + dir(_memb.Reader) if 'rank' in entry.lower()]   # (the surface of _memb is pinned)
    for method in ('similarity_ranks_device', 'similarity_ranks', 'rank_device', 'rank', 'count_closer_than', 'analogy_ranks_device',
                   'analogy_ranks', 'evaluate_analogies', 'last_ranks_kernel'):
        assert hasattr(native.Reader, method)
    assert callable(memb_amd.reader.ranks_host)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_under_the_host_sanitizers(tmp_path):
    # hip_ranks_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on the
    # HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'ranks_planning_main.cpp')
    program = str(tmp_path / 'ranks_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'ranks planning: ok' in run.stdout, run.stdout
