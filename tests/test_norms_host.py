"""Row norms and unit rows without a GPU: the reference of tests/norms_reference.py against float64, a device='cpu' reader
bit for bit against that reference (include/memb_hip_norms.h's contract over reader.rows_embedding), special rows, the C
header and the entry points' refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from norms_reference import (check_special_rows, ids_with_misses, norm_of_one_row, norms_by_the_contract, special_model,
                             unit_rows_by_the_contract)

HEADER = os.path.join(REPO, 'include', 'memb_hip_norms.h')
DIMS = (3, 4, 7, 256, 260, 300, 512, 516, 1028)
STORAGES = [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)]
N_ROWS = 150


# ---- 1. the reference itself ----

@pytest.mark.parametrize('dim', (1, 3, 4, 5, 255, 256, 257, 300, 512, 1000, 1024))
def test_reference_rounds_as_often_as_the_contract_says(dim):
    # one rounding per product, 3 piece adds, ceil(dim / 256) - 1 lane adds, 6 butterfly adds, one root: all terms are
    # positive, so the relative error is below (1 + 3 + 3 + 6 + 1) * 2^-24 < 2^-20
    rng = np.random.default_rng(dim)
    values = np.concatenate([rng.standard_normal((40, dim)), rng.standard_normal((20, dim)) * 1e-3,
                             rng.standard_t(3, size=(20, dim)) * 50]).astype(np.float32)
    norms = norms_by_the_contract(values)
    assert norms.dtype == np.float32 and norms.shape == (80,)
    exact = np.sqrt((values.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(norms.astype(np.float64) - exact) <= 2.0 ** -20 * exact).all()
    # the matrix form is the lane-by-lane walk of one row
    for i in (0, 41, 79):
        assert norms[i].tobytes() == norm_of_one_row(values[i]).tobytes()
    unit, again = unit_rows_by_the_contract(values)
    assert bits_equal(again, norms) and bits_equal(unit, values / norms[:, None])


def test_reference_order_is_the_contracts_not_a_plain_sum():
    # a row whose plain left-to-right float32 sum differs from the tree's: the reference follows the tree
    values = np.zeros((1, 300), dtype=np.float32)
    values[0, 0] = 4096.0
    values[0, 1:] = 1.0 / 3.0
    tree = norms_by_the_contract(values)[0]
    assert tree.tobytes() == norm_of_one_row(values[0]).tobytes()
    running = np.float32(0.0)
    for value in values[0]:
        running = running + value * value
    assert np.sqrt(running).tobytes() != tree.tobytes()


# ---- 2. a device='cpu' reader ----

@pytest.mark.parametrize('storage,bits', STORAGES)
@pytest.mark.parametrize('dim', DIMS)
def test_host_reader_has_the_contracts_bits(native, make_model, storage, bits, dim):
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows = np.concatenate([ids_with_misses(200, N_ROWS, dim + bits), np.arange(N_ROWS, dtype=np.uint32)])
    values = reader.rows_embedding(rows)
    missing = rows >= N_ROWS
    assert missing.any() and not values[missing].any()
    want_unit, want_norms = unit_rows_by_the_contract(values)
    norms = reader.row_norms(rows)
    assert norms.dtype == np.float32 and norms.shape == (len(rows),)
    assert bits_equal(norms, want_norms), (storage, bits, dim)
    assert not norms[missing].any() and (norms[~missing] > 0).all()
    unit = reader.unit_rows_embedding(rows)
    assert unit.dtype == np.float32 and unit.shape == (len(rows), dim)
    assert bits_equal(unit, want_unit), (storage, bits, dim)
    assert not unit[missing].any()
    # n = 0
    none = np.zeros(0, dtype=np.uint32)
    assert reader.row_norms(none).shape == (0,) and reader.unit_rows_embedding(none).shape == (0, dim)


def test_host_reader_works_in_bounded_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 64)
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows = ids_with_misses(64 * 3 + 5, N_ROWS, 9)
    want_unit, want_norms = unit_rows_by_the_contract(reader.rows_embedding(rows))
    assert bits_equal(reader.row_norms(rows), want_norms) and bits_equal(reader.unit_rows_embedding(rows), want_unit)


def test_device_methods_refuse_a_host_reader(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    assert reader.last_norms_kernel == ''
    for call in (lambda: reader.row_norms_device(None), lambda: reader.unit_rows_embedding_device(None),
                 lambda: reader.unit_batch_embedding_device(['a'])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()


# ---- 3. special rows ----

def test_subnormal_sums_and_signed_zero_rows(native, tmp_path):
    path, vectors = special_model(native, tmp_path)
    reader = native.Reader(path, device='cpu')
    rows = np.arange(6, dtype=np.uint32)
    assert bits_equal(reader.rows_embedding(rows), vectors)
    check_special_rows(vectors, reader.row_norms(rows), reader.unit_rows_embedding(rows))


# ---- 4. the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    assert '#include "memb_hip.h"' in open(HEADER).read()
    # the header it extends is as it was
    assert 'norms' not in open(os.path.join(REPO, 'include', 'memb_hip.h')).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    norms = library.memb_hip_row_norms_device
    norms.argtypes = [pointer, pointer, size, pointer, pointer]
    assert norms(None, None, 0, None, None) == 1   # MEMB_HIP_ERR_INVALID: no context
    assert b'null' in library.memb_hip_last_error()
    unit = library.memb_hip_decode_unit_rows_device
    unit.argtypes = [pointer, pointer, size, pointer, size, size, pointer, pointer]
    assert unit(None, None, 0, None, 300, 0, None, None) == 1
    assert b'null' in library.memb_hip_last_error()
    dense = library.memb_hip_dense_row_norms_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, pointer, pointer]
    assert dense(0, None, 5, 300, 300, None, None) == 1   # values missing
    assert b'null' in library.memb_hip_last_error()
    assert dense(0, None, 0, 0, 0, None, None) == 1
    assert b'dim' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 299, None, None) == 1
    assert b'ld_values' in library.memb_hip_last_error()
    assert dense(-1, None, 0, 300, 300, None, None) == 1
    assert b'device' in library.memb_hip_last_error()
    assert dense(0, 2, 0, 300, 300, None, None) == 1      # a pointer that is not aligned to a float
    assert b'aligned' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 300, None, None) == 0   # n == 0: a no-op
    dense_unit = library.memb_hip_dense_unit_rows_device
    dense_unit.argtypes = [ctypes.c_int, pointer, size, size, size, pointer, size, size, pointer, pointer]
    assert dense_unit(0, None, 5, 300, 300, None, 300, 0, None, None) == 1
    assert b'null' in library.memb_hip_last_error()
    assert dense_unit(0, None, 0, 300, 300, None, 299, 0, None, None) == 1
    assert b'ld must be' in library.memb_hip_last_error()
    assert dense_unit(0, None, 0, 300, 300, None, 304, 5, None, None) == 1
    assert b'ld must be' in library.memb_hip_last_error()
    assert dense_unit(0, None, 0, 300, 300, 6, 300, 0, None, None) == 1
    assert b'aligned' in library.memb_hip_last_error()
    assert dense_unit(0, None, 0, 300, 300, None, 300, 0, None, None) == 0
    name = library.memb_hip_norms_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer, ctypes.c_int, pointer, size, size]
    assert name(None, 0, None, 0, 0) == b'norms_dense' and name(None, 1, None, 0, 0) == b'unit_dense'
    count = library.memb_hip_norms_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, ctypes.c_int, ctypes.c_int, pointer]
    assert count(None, None, 0, 0, 1, None) == 1
    assert b'null' in library.memb_hip_last_error()
    from memb_amd import _memb
    for binding in ('dense_row_norms_to_device', 'dense_unit_rows_to_device', 'dense_norms_kernel_name'):
        assert hasattr(_memb, binding)
    for method in ('row_norms_to_device', 'unit_rows_to_device', 'norms_kernel_name', 'norms_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    assert _memb.dense_norms_kernel_name(False) == 'norms_dense' and _memb.dense_norms_kernel_name(True) == 'unit_dense'
    for method in ('row_norms_device', 'unit_rows_embedding_device', 'unit_batch_embedding_device', 'row_norms',
                   'unit_rows_embedding', 'last_norms_kernel'):
        assert hasattr(native.Reader, method)
