"""The lists of the candidates before a mark without a GPU: the package's numpy form against the plain-loop restatement of
tests/within_reference.py on hostile matrices, every kind of mark and list of non-candidates, slices with bases, the sizes
ranks_host counts, a device='cpu' reader's similarity_within, closer_than and words_within against the restatement and
against answers worked out by hand, the argument errors, the C header and the entry points' refusals, and
hip_within_launch.h's planning built into a program of its own under the host sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from ranks_reference import INT64_MAX, hostile_matrix, marks_over
from within_reference import same_lists, within_by_the_contract

HEADER = os.path.join(REPO, 'include', 'memb_hip_within.h')
DENSE = 'within_count+within_starts+within_write'


def test_the_restatement_by_hand():
    row = np.array([[0.5, np.nan, 0.5, -0.0, 0.0, -np.inf, 0.5, np.inf]], dtype=np.float32)
    half = np.float32([0.5])

    def positions(thresholds, marks, **more):
        offsets, found, values = within_by_the_contract(row, thresholds, marks, **more)
        assert offsets.tolist() == [0, len(found)]
        assert values.view(np.uint32).tolist() == [int(row[0, c - more.get('base', 0)].view(np.uint32)) for c in found]
        return found.tolist()

    assert positions(half, [-1]) == [1, 7]                        # NaN and +inf are greater
    assert positions(half, [INT64_MAX]) == [0, 1, 2, 6, 7]        # and three are equal
    assert positions(half, [2]) == [0, 1, 7]                      # column 2 is the second of the equals
    assert positions(np.float32([0.0]), [4]) == [0, 1, 2, 3, 6, 7]   # -0.0 at 3 ties with +0.0 at 4 and comes first
    assert positions(np.float32([np.nan]), [INT64_MAX]) == [1]
    assert positions(np.float32([np.nan]), [-1]) == []
    assert positions(half, [INT64_MAX], exclude=[[0, 0, 1, -1, 99]]) == [2, 6, 7]
    assert positions(half, [12], base=10) == [10, 11, 17]


def lists_for(count, n, marks, seed, base=0):
    """int64 (count, 9): repeats, -1 padding, entries out of range on both sides, and the mark itself"""
    rng = np.random.default_rng(seed)
    lists = base + rng.integers(0, n, size=(count, 9)).astype(np.int64)
    lists[:, 3] = lists[:, 0]
    lists[:, 4] = -1
    lists[:, 5] = base + n + rng.integers(0, 5, size=count)
    lists[:, 6] = base - 1 - rng.integers(0, 5, size=count)
    lists[:, 7] = np.clip(marks, -1, base + n)
    return lists


@pytest.mark.parametrize('count,n', [(1, 1), (3, 63), (17, 300), (8, 1000)])
def test_the_packages_host_lists_are_the_restatement(native, count, n):
    from memb_amd.reader import ranks_host, within_host
    matrix = hostile_matrix(count, n, seed=7 * count + n)
    matrix[0, :n // 2] = np.float32(0.5)                    # a run of bit-equal values: the mid-tie mark cuts it
    for base in (0, 1000):
        thresholds, marks = marks_over(matrix, seed=n, base=base)
        thresholds[0], marks[0] = np.float32(0.5), base + n // 4
        for exclude in (None, lists_for(count, n, marks, n, base)):
            got = within_host(matrix, thresholds, marks, base, exclude)
            assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float32
            assert same_lists(got, within_by_the_contract(matrix, thresholds, marks, base, exclude)), (count, n, base)
            # the size of every segment is the count
            assert np.diff(got[0]).tolist() == ranks_host(matrix, thresholds, marks, base, exclude).tolist()
        for kind in (-1, INT64_MAX):
            every = np.full(count, kind, dtype=np.int64)
            assert same_lists(within_host(matrix, thresholds, every, base), within_by_the_contract(matrix, thresholds, every, base))
    assert same_lists(within_host(matrix, thresholds, None), within_by_the_contract(matrix, thresholds, np.full(count, -1)))
    empty = within_host(matrix[:, :0], thresholds, marks)
    assert empty[0].tolist() == [0] * (count + 1) and empty[1].shape == (0,) and empty[2].shape == (0,)
    assert within_host(matrix[:0], thresholds[:0], marks[:0])[0].tolist() == [0]


def test_slices_with_bases_concatenate_to_the_whole(native):
    from memb_amd.reader import within_host
    matrix = hostile_matrix(5, 700, seed=3)
    thresholds, marks = marks_over(matrix, seed=4)
    lists = np.random.default_rng(5).integers(-3, 710, size=(5, 12)).astype(np.int64)
    whole = within_host(matrix, thresholds, marks, 0, lists)
    assert same_lists(whole, within_by_the_contract(matrix, thresholds, marks, 0, lists))
    cuts = [0, 1, 64, 65, 300, 699, 700]
    pieces = [within_host(matrix[:, start:stop], thresholds, marks, start, lists) for start, stop in zip(cuts[:-1], cuts[1:])]
    for q in range(5):
        positions = np.concatenate([piece[1][piece[0][q]:piece[0][q + 1]] for piece in pieces])
        values = np.concatenate([piece[2][piece[0][q]:piece[0][q + 1]] for piece in pieces])
        assert positions.tolist() == whole[1][whole[0][q]:whole[0][q + 1]].tolist()
        assert values.view(np.uint32).tolist() == whole[2][whole[0][q]:whole[0][q + 1]].view(np.uint32).tolist()


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


def test_words_worked_out_by_hand(royal):
    reader = royal
    # around king (1, 1, 0, 0): prince 0.943, man 0.707, queen 0.5, girl 0.067, apple and woman 0 -- apple has the lower row.
    # The lists come in row order: the order of keys()
    order = {word: row for row, word in enumerate(reader.keys())}
    nearest = ['prince', 'man', 'queen', 'girl', 'apple', 'woman']
    for place, word in enumerate(nearest):
        closer = reader.closer_than('king', word)
        assert closer == sorted(nearest[:place], key=order.get), word
        assert len(closer) == reader.count_closer_than(['king'], [word])[0]
    assert reader.closer_than('king', 'king') == []                     # nothing but itself is as close, and it is no candidate
    assert reader.closer_than('nobody', 'queen') == [] and reader.closer_than('king', 'nobody') == []
    within = reader.words_within(['king', 'nobody', 'apple'], 0.45)
    assert [word for word, _ in within[0]] == sorted(['prince', 'man', 'queen'], key=order.get)
    assert all(cosine >= 0.45 for _, cosine in within[0]) and within[1] == []
    assert within[2] == []                                              # apple itself is left out, and nothing else is that close
    assert [word for word, _ in reader.words_within(['king'], -1.0)[0]] == sorted(nearest, key=order.get)
    assert reader.words_within([], 0.5) == []
    with pytest.raises(TypeError, match='min_cosine'):
        reader.words_within(['king'], '0.5')
    with pytest.raises(ValueError, match='NaN'):
        reader.words_within(['king'], float('nan'))
    for call in (lambda: reader.closer_than_device(['king'], ['queen']), lambda: reader.words_within_device(['king'], 0.5),
                 lambda: reader.similarity_within_device(None, None, None)):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()
    assert reader.last_within_kernel == ''


def test_host_reader_lists_over_chunks(native, make_model, monkeypatch):
    import memb_amd.reader
    path, words = make_model(3000, 300, 'trained', 4)
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
        got = reader.similarity_within(queries, rows, thresholds, marks, exclude=exclude)
        assert same_lists(got, within_by_the_contract(matrix, thresholds, marks, 0, exclude))
        assert np.diff(got[0]).tolist() == reader.similarity_ranks(queries, rows, thresholds, marks, exclude=exclude).tolist()
    assert reader.similarity_within(queries, rows, thresholds, marks)[1][:3].tolist() == [3, 10, 11]   # they tie with 12 and come first
    assert same_lists(reader.similarity_within(queries, rows, thresholds), within_by_the_contract(matrix, thresholds, [-1] * 3))
    assert reader.similarity_within(queries, rows[:0], thresholds, marks)[0].tolist() == [0, 0, 0, 0]
    # the words of the whole model, 3000 candidates in chunks of 16
    pair = [words[17], words[40]]
    own = reader.resolve_rows(pair).astype(np.int64)
    everything = reader.similarity_matrix(reader.unit_rows_embedding(own[:1].astype(np.uint32)), np.arange(3000, dtype=np.uint32))
    want = within_by_the_contract(everything, everything[:, own[1]], own[1:], 0, own[None, :1])[1]
    assert reader.closer_than(*pair) == [reader.keys()[row] for row in want]
    assert len(want) == reader.count_closer_than(pair[:1], pair[1:])[0]
    radius = float(np.sort(everything[0])[-20])
    want = within_by_the_contract(everything, np.float32([radius]), [INT64_MAX], 0, own[None, :1])
    got = reader.words_within(pair[:1], radius)[0]
    assert len(got) == 19 and got == [(reader.keys()[row], float(value)) for row, value in zip(want[1], want[2])]
    with pytest.raises(TypeError, match='float32'):
        reader.similarity_within(queries.astype(np.float64), rows, thresholds)
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_within(queries[:, :299], rows, thresholds)
    with pytest.raises(TypeError, match='thresholds'):
        reader.similarity_within(queries, rows, thresholds.astype(np.float64))
    with pytest.raises(ValueError, match='thresholds'):
        reader.similarity_within(queries, rows, thresholds[:2])
    with pytest.raises(TypeError, match='marks'):
        reader.similarity_within(queries, rows, thresholds, marks.astype(np.float32))
    with pytest.raises(ValueError, match='marks'):
        reader.similarity_within(queries, rows, thresholds, marks[:2])
    with pytest.raises(ValueError, match='64'):
        reader.similarity_within(queries, rows, thresholds, marks, exclude=np.zeros((3, 65), dtype=np.int64))
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_within(queries, rows, thresholds, marks, exclude=lists[:2])


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_query_matrix.h"' in text and text.count('#include') == 1
    for word in ('ASCENDING within a row', 'SUPPLIED by the caller', 'WRITES ARE BOUNDED', 'ACCUMULATE', 'depends on the inputs alone',
                 'within_count', 'within_starts', 'within_write'):
        assert word in text, word
    not_built = text[text.index('Not built:'):]
    for word in ('ReadersUnion', 'ShardedReader', 'bf16 / fp16', 'pooled-bag', '3CosMul', 'sorted by cosine'):
        assert word in not_built, word
    # the names the older headers' tests keep to their own header
    for word in ('memb_hip_ranks', 'rank_count', 'query_topk', 'dense_topk', 'TOPK', 'query_bags', 'excluding', 'weighted_rows_sum',
                 'analogies', 'memb_hip_cosmul', 'cosmul_scores', 'COSMUL'):
        assert word not in text, word
    # no older header knows the new names
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_within.h':
            older = open(os.path.join(REPO, 'include', name)).read()
            assert 'memb_hip_within' not in older and 'within_count' not in older and 'dense_within' not in older, name


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    dense = library.memb_hip_dense_within_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, ctypes.c_int64, pointer, pointer, pointer, size, size, ctypes.c_int,
                      pointer, pointer, pointer, pointer, size, pointer, size, pointer]
    good = dict(device=0, matrix=64, n_rows=2, n=7, ld=8, base=0, thresholds=128, marks=256, excluded=512, width=3, ld_excluded=3,
                accumulate=0, offsets=1024, cursors=2048, positions=4096, values=8192, capacity=100, workspace=16384,
                workspace_bytes=64, stream=None)

    def call(**changes):
        return dense(*dict(good, **changes).values())

    # (every one of these is refused before a pointer is read or the device is touched)
    assert refused(call(device=-1), b'device')
    assert refused(call(base=-1), b'base')
    assert refused(call(matrix=None), b'matrix')
    assert refused(call(ld=6), b'at least n')
    for name in ('thresholds', 'marks', 'offsets', 'cursors', 'positions'):
        assert refused(call(**{name: None}), b'null'), name
    for name in ('matrix', 'thresholds', 'values'):
        assert refused(call(**{name: good[name] + 2}), b'aligned'), name
    for name in ('marks', 'offsets', 'cursors', 'positions', 'excluded', 'workspace'):
        assert refused(call(**{name: good[name] + 4}), b'aligned'), name
    assert refused(call(width=65, ld_excluded=65), b'at most 64')
    assert refused(call(ld_excluded=2), b'ld_excluded')
    assert refused(call(excluded=None), b'excluded')
    assert refused(call(n_rows=2 ** 16 + 1), b'too large')
    assert refused(call(n=2 ** 31 + 1, ld=2 ** 32), b'too large')
    assert refused(call(capacity=2 ** 62 + 1), b'capacity')
    assert refused(call(workspace=None), b'workspace') and refused(call(workspace_bytes=23), b'workspace too small')
    assert call(n_rows=0) == 0                                        # no row: a no-op, nothing touched
    assert call(n=0, matrix=None, accumulate=1, workspace=None, workspace_bytes=0) == 0   # no column under accumulate: cursors stay
    dense_bytes = library.memb_hip_dense_within_workspace_bytes
    dense_bytes.restype = size
    dense_bytes.argtypes = [size, size]
    # an int64 start and a 32-bit total per block, the totals rounded up to 8 bytes
    assert dense_bytes(2, 7) == 24 and dense_bytes(3, 2049) == 72 and dense_bytes(1, 2048) == 16 and dense_bytes(5, 0) == 0
    assert dense_bytes(2 ** 16 + 1, 7) == 0 and dense_bytes(2, 2 ** 31 + 1) == 0
    fused = library.memb_hip_query_within_device
    fused.argtypes = [pointer, pointer, size, size, pointer, size, pointer, pointer, pointer, size, size, pointer, pointer, pointer,
                      pointer, size, pointer, size, pointer]
    assert refused(fused(None, 64, 3, 300, 128, 5, 256, 512, None, 0, 0, 1024, 2048, 4096, None, 10, 8192, 1 << 20, None), b'ctx')
    size_of = library.memb_hip_query_within_workspace_bytes
    size_of.restype = size
    size_of.argtypes = [pointer, size, size, ctypes.c_int]
    assert size_of(None, 3, 1000, 0) == 0
    name = library.memb_hip_query_within_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == DENSE.encode()

    import memb_amd
    from memb_amd import _memb, _memb_within
    # the bindings: a module of its own, by context handle; a reader on the host has no context
    for entry in ('dense_within_to_device', 'dense_within_workspace_bytes', 'query_within_to_device', 'query_within_workspace_bytes',
                  'query_within_kernel_name'):
        assert callable(getattr(_memb_within, entry)), entry
    assert _memb_within.dense_within_kernel_name() == DENSE and _memb_within.dense_within_workspace_bytes(2, 7) == 24
    assert _memb_within.query_within_kernel_name(0) == '' and _memb_within.query_within_workspace_bytes(0, 3, 1000) == 0
    with pytest.raises(RuntimeError, match='memb_hip_query_within_device.*ctx'):
        _memb_within.query_within_to_device(0, 64, 3, 300, 128, 5, 256, 512, 0, 0, 0, 1024, 2048, 4096, 0, 10, 8192, 1 << 20)
    with pytest.raises(RuntimeError, match='memb_hip_dense_within_device.*device'):
        _memb_within.dense_within_to_device(-1, 64, 2, 7, 8, 0, 128, 256, 0, 0, 0, False, 1024, 2048, 4096, 0, 10, 8192, 64)
    assert not [entry for entry in dir(_memb) + dir(_memb.Reader) if 'within' in entry.lower()]   # (the surface of _memb is pinned)
    for method in ('similarity_within_device', 'similarity_within', 'closer_than_device', 'closer_than', 'words_within_device',
                   'words_within', 'last_within_kernel'):
        assert hasattr(native.Reader, method)
    assert callable(memb_amd.reader.within_host)


def test_planning_under_the_host_sanitizers(tmp_path):
    # hip_within_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer: host
    # code alone, so the host compiler that builds the bindings builds it -- no GPU, no hipcc, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'within_planning_main.cpp')
    program = str(tmp_path / 'within_planning')
    build = subprocess.run(
        ['g++', '-x', 'c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'within planning: ok' in run.stdout, run.stdout
