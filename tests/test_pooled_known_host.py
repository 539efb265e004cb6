"""Pooling over the rows a model knows, without a GPU: the header and the entry point of include/memb_hip_pooled_known.h,
and bags_embedding(missing='skip') on a device='cpu' reader -- bit for bit against R1, the contract's explicit loop over
reader.rows_embedding(rows), and R2, the existing call (missing='zero') on the batch with its unknown entries taken out."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from pooled_reference import UNKNOWN, compacted, offsets_of, sequential_by_the_contract

HEADER = os.path.join(REPO, 'include', 'memb_hip_pooled_known.h')
POOLED_HEADER = os.path.join(REPO, 'include', 'memb_hip_pooled.h')


def test_header_is_plain_c_and_cxx_and_leaves_the_pooled_header_alone():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert 'memb_hip_pool_known_rows_device_typed' in text and '#include "memb_hip_pooled.h"' in text
    assert '#define MEMB_HIP_POOL_' not in text and 'define MEMB_HIP_OUT_' not in text   # the modes and types are reused
    pooled = open(POOLED_HEADER).read()
    assert re.findall(r'#define (MEMB_HIP_POOL_\w+) (\d+)', pooled) == [('MEMB_HIP_POOL_SUM', '0'), ('MEMB_HIP_POOL_MEAN', '1')]
    assert 'memb_hip_pool_known' not in pooled


def test_entry_point_is_exported_and_refuses_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pool = library.memb_hip_pool_known_rows_device_typed
    pool.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                     ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for out_type in (0, 1, 2):
        for mode in (0, 1):
            assert pool(None, None, 0, None, 0, None, out_type, 300, 0, mode, None, None) == 1   # MEMB_HIP_ERR_INVALID: no context
            assert b'null' in library.memb_hip_last_error()
        for mode in (-1, 2, 7):
            assert pool(None, None, 0, None, 0, None, out_type, 300, 0, mode, None, None) == 1
            assert b'pooling mode' in library.memb_hip_last_error()
    for out_type in (-1, 3, 7):
        assert pool(None, None, 0, None, 0, None, out_type, 300, 0, 0, None, None) == 1
        assert b'out_type' in library.memb_hip_last_error()
    from memb_amd import _memb
    assert 'counts_ptr' in _memb.Reader.pool_known_rows_to_device.__doc__
    assert 'counts_ptr' not in _memb.Reader.pool_rows_to_device.__doc__
    from memb_amd.reader import Reader
    for method in (Reader.bags_embedding_device, Reader.sentences_embedding_device, Reader.bags_embedding):
        parameters = inspect.signature(method).parameters
        assert parameters['missing'].default == 'zero' and parameters['return_counts'].default is False


def check_host(reader, rows, offsets, context):
    n_rows = len(reader)
    values = reader.rows_embedding(rows) if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)
    dense_rows, dense_offsets, _ = compacted(rows, offsets, n_rows)
    for mode in ('sum', 'mean'):
        want, want_counts = sequential_by_the_contract(values, rows, offsets, n_rows, mode, True)
        got, counts = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True)
        assert got.dtype == np.float32 and counts.dtype == np.uint32 and counts.shape == (len(offsets) - 1,)
        assert bits_equal(got, want), (context, mode, 'R1')
        assert np.array_equal(counts, want_counts), (context, mode)
        assert bits_equal(got, reader.bags_embedding(dense_rows, dense_offsets, mode=mode)), (context, mode, 'R2')
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, missing='skip'), want)
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, missing='zero'), reader.bags_embedding(rows, offsets, mode=mode))


def rows_with_unknowns(count, n_rows, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=count, dtype=np.int64)
    unknown = rng.random(count) < 0.35
    rows[unknown] = rng.choice([UNKNOWN, n_rows, n_rows + 11], size=int(unknown.sum()))
    return rows.astype(np.uint32)


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_host_bags_skip_unknown_entries(native, make_model, storage, bits):
    path, _ = make_model(3000, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    lengths = [0, 0, 1, 1, 1, 7, 8, 9, 17, 0, 3, 300] + list(np.random.default_rng(bits).geometric(0.15, size=40)) + [0, 2, 0]
    offsets = offsets_of(lengths)
    rows = rows_with_unknowns(int(offsets[-1]), 3000, 7)
    rows[0:3] = [5, UNKNOWN, 3000]            # bags of one entry: known, unknown, an id >= n_rows
    rows[3:10] = UNKNOWN                      # a bag of unknown entries only
    rows[10], rows[17] = UNKNOWN, UNKNOWN     # unknown first and last
    rows[18:27:2] = UNKNOWN                   # alternating
    check_host(reader, rows, offsets, storage)
    check_host(reader, rows, np.arange(len(rows) + 1), (storage, 'ones'))
    vectors, counts = reader.bags_embedding(rows, [0], missing='skip', return_counts=True)
    assert vectors.shape == (0, 300) and counts.shape == (0,)
    vectors, counts = reader.bags_embedding(np.zeros(0, dtype=np.uint32), [0, 0, 0], missing='skip', return_counts=True)
    assert bits_equal(vectors, np.zeros((2, 300), dtype=np.float32)) and not counts.any()


def test_host_bags_span_chunks(native, make_model, monkeypatch):
    # bags that straddle the bounded chunks of the host path: one longer than several chunks, one whose first known entry
    # lies in a later chunk than its first entry, one whose chunks in the middle hold nothing known
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'BAGS_HOST_CHUNK', 64)
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    offsets = offsets_of([3, 60, 1, 0, 200, 64, 64, 5, 0, 0, 31, 150, 260])
    rows = rows_with_unknowns(int(offsets[-1]), 3000, 3)
    rows[64:128] = UNKNOWN        # a whole chunk inside the bag of 200
    rows[428:428 + 100] = UNKNOWN   # the bag of 150 starts with 100 unknown entries: its sum starts two chunks on
    rows[offsets[-2] + 70:offsets[-2] + 200] = UNKNOWN
    check_host(reader, rows, offsets, 'chunks')
    check_host(reader, np.full(300, UNKNOWN, dtype=np.uint32), offsets_of([100, 0, 200]), 'nothing known')


def test_signed_zeros_and_subnormals_on_the_host(native, tmp_path):
    tiny = np.float32(1e-40)
    vectors = np.array([
        [-0.0, -0.0, -0.0, -0.0, -0.0, -0.0],
        [-0.0, 0.0, tiny, -tiny, 3e-39, 1.0],
        [0.0, -0.0, -3 * tiny, 2 * tiny, 1e-45, 1e-8],
        [1e30, -1e30, 1e-45, -1e-45, 1.1754942e-38, 2.5],
    ], dtype=np.float32)
    builder = native.Builder(vectors.shape[1], 'full', 8)
    builder.add_words(['w{}'.format(i) for i in range(len(vectors))], vectors)
    path = str(tmp_path / 'exact.bin')
    builder.save(path)
    reader = native.Reader(path, device='cpu')
    rows = np.array([UNKNOWN, 0, 0, UNKNOWN, 1, UNKNOWN, 2, UNKNOWN, 4, 3, 2, UNKNOWN, 1], dtype=np.uint32)
    offsets = np.array([0, 2, 4, 7, 9, 13], dtype=np.int64)
    check_host(reader, rows, offsets, 'exact')
    for mode in ('sum', 'mean'):
        skipped = reader.bags_embedding(rows, offsets, mode=mode, missing='skip')
        counted = reader.bags_embedding(rows, offsets, mode=mode, missing='zero')
        assert np.signbit(skipped[:2]).all() and not skipped[:2].any()     # [missing, -0.0] and [-0.0, missing]: -0.0
        assert not np.signbit(counted[:2]).any()                           # +0.0 + -0.0 where missing rows count
        assert not np.signbit(skipped[3]).any() and not skipped[3].any()   # nothing known: +0.0
    total = reader.bags_embedding(rows, offsets, mode='sum', missing='skip')
    assert total[2][2] == np.float32(tiny) + np.float32(-3 * tiny) and total[2][2] != 0   # a subnormal sum is kept


def test_errors_on_the_host_and_the_union(native, make_model):
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows = np.arange(10, dtype=np.uint32)
    with pytest.raises(ValueError, match='missing'):
        reader.bags_embedding(rows, [0, 10], missing='ignore')
    with pytest.raises(ValueError, match='missing'):
        reader.bags_embedding(rows, [0, 10], missing=None)
    with pytest.raises(ValueError, match='return_counts'):
        reader.bags_embedding(rows, [0, 10], return_counts=True)
    with pytest.raises(ValueError, match='return_counts'):
        reader.bags_embedding(rows, [0, 10], missing='zero', return_counts=True)
    with pytest.raises(ValueError):
        reader.bags_embedding(rows, [0, 10], mode='max', missing='skip')
    with pytest.raises(ValueError):
        reader.bags_embedding(rows, [0, 5, 3, 10], missing='skip')
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.sentences_embedding_device([['a', 'b'], ['c']], missing='skip')
    union = native.ReadersUnion([reader, native.Reader(path, device='cpu')], 'average')
    for method in (union.bags_embedding_device, union.bags_embedding, union.sentences_embedding_device):
        with pytest.raises(NotImplementedError, match='ReadersUnion'):
            method(rows, [0, 3], missing='skip', return_counts=True)
