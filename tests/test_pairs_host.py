"""Cosine similarity of row pairs without a GPU: the two references of tests/pairs_reference.py against each other and
against float64, the sign rule of the lane partials, a device='cpu' reader bit for bit against the reference
(include/memb_hip_pairs.h's contract over reader.rows_embedding), the C header and the entry points' refusals. (The byte
count needs a staged model and is checked in tests/test_gpu_pairs.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, bits_equal
from norms_reference import ids_with_misses, norms_by_the_contract, special_model
from pairs_reference import pair_of_two_rows, pairs_by_the_contract, pairs_of_rows

HEADER = os.path.join(REPO, 'include', 'memb_hip_pairs.h')
DIMS = (1, 3, 4, 255, 256, 260, 300, 512, 516, 1024)
N_ROWS = 3000
ONE_AND_AN_ULP = np.float32(1.0000001)


def gaussian_pairs(dim, count, seed):
    """`count` Gaussian pairs of three correlations (about 0, 0.5 and 0.99) and three scales"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((count, dim))
    rho = np.array([0.0, 0.5, 0.99])[np.arange(count) % 3][:, None]
    y = rho * x + np.sqrt(1 - rho * rho) * rng.standard_normal((count, dim))
    scale = np.array([1.0, 1e-3, 50.0])[(np.arange(count) // 3) % 3][:, None]
    return (x * scale).astype(np.float32), (y / scale).astype(np.float32)


def with_special_pairs(x, y):
    """the pairs (x, x), (x, -x), a zero row, a -0.0 row and rows of 2^-70 on top of x, y"""
    dim = x.shape[1]
    tiny = np.full(dim, 2.0 ** -70, dtype=np.float32)
    zero = np.zeros(dim, dtype=np.float32)
    extra = [(x[0], x[0]), (x[1], -x[1]), (x[2], zero), (zero, zero), (-zero, x[3]), (zero, -zero), (-zero, -zero),
             (tiny, tiny), (tiny, -tiny), (tiny, x[4])]
    return (np.concatenate([x, np.stack([a for a, _ in extra])]), np.concatenate([y, np.stack([b for _, b in extra])]),
            len(extra))


# ---- 1. the references ----

@pytest.mark.parametrize('dim', DIMS)
def test_matrix_reference_is_the_scalar_one(dim):
    x, y = gaussian_pairs(dim, 300, dim)
    x, y, extra = with_special_pairs(x, y)
    cosines, dots, norms = pairs_by_the_contract(x, y)
    assert cosines.dtype == dots.dtype == norms.dtype == np.float32
    assert cosines.shape == dots.shape == (len(x),) and norms.shape == (len(x), 2)
    # every special pair and every seventh Gaussian one, lane by lane
    for i in list(range(0, 300, 7)) + list(range(300, 300 + extra)):
        want = pair_of_two_rows(x[i], y[i])
        got = (cosines[i], dots[i], norms[i, 0], norms[i, 1])
        assert [value.tobytes() for value in got] == [value.tobytes() for value in want], (dim, i, got, want)
    assert bits_equal(norms[:, 0], norms_by_the_contract(x)) and bits_equal(norms[:, 1], norms_by_the_contract(y))
    # the rows of 2^-70: dim products of 2^-140 sum to a subnormal (dim 1024 included: 2^-130), a flush would give 0; both
    # norms are below 1e-12, so the cosine is the dot over 1e-24
    tiny = 300 + extra - 3
    assert 0 < dots[tiny] < np.float32(1.1754944e-38) and dots[tiny + 1] == -dots[tiny]
    assert dots[tiny] == np.float32(dim * 2.0 ** -140)
    assert (norms[tiny] < 1e-12).all() and cosines[tiny] == dots[tiny] / (np.float32(1e-12) * np.float32(1e-12))
    # zero rows: a cosine of zero, never a NaN
    assert not np.isnan(cosines).any()
    assert (cosines[302:307] == 0).all() and (dots[302:307] == 0).all()


@pytest.mark.parametrize('dim', DIMS)
def test_reference_is_close_to_float64_and_not_clamped(dim):
    x, y = gaussian_pairs(dim, 600, 1000 + dim)
    x = np.concatenate([x, x[:100]])
    y = np.concatenate([y, x[:100]])       # 100 rows with themselves
    cosines, _, _ = pairs_by_the_contract(x, y)
    wide_x, wide_y = x.astype(np.float64), y.astype(np.float64)
    exact = (wide_x * wide_y).sum(axis=1) / (np.sqrt((wide_x * wide_x).sum(axis=1)) * np.sqrt((wide_y * wide_y).sum(axis=1)))
    worst = np.abs(cosines.astype(np.float64) - exact).max()
    print('dim', dim, 'worst |cos - cos64| =', worst / 2.0 ** -24, '* 2^-24')
    assert worst <= 2.0 ** -20, (dim, worst)
    assert np.abs(cosines).max() <= 1 + 2.0 ** -22, (dim, np.abs(cosines).max())
    # a row with itself: dot and both sums of squares are the same bits t, and t / (sqrt(t) * sqrt(t)) is 1 within three
    # roundings (the root twice in the product, the product): 1.0000001 = 1 + 2^-23 is allowed -- nothing clamps it
    own = cosines[600:]
    assert (np.abs(own.astype(np.float64) - 1) <= 2.0 ** -22).all(), own
    assert ONE_AND_AN_ULP > 1 and float(ONE_AND_AN_ULP) == 1 + 2.0 ** -23
    print('dim', dim, 'cos(x, x) == 1.0000001 in', int((own == ONE_AND_AN_ULP).sum()), 'of 100; > 1 in', int((own > 1).sum()))


def test_a_lane_with_one_piece_keeps_the_sign_of_its_zero():
    # dim 260 is 65 pieces: lane 0 holds the pieces 0 and 64, every other lane one piece alone. +0.0 times -1 is -0.0 in
    # every column, so every piece product is -0.0 and so is every lane partial that is SELECTED; a lane that added its
    # lone -0.0 to +0.0 would hold +0.0 and the butterfly would end in +0.0.
    x = np.zeros((1, 260), dtype=np.float32)
    y = -np.ones((1, 260), dtype=np.float32)
    cosines, dots, norms = pairs_by_the_contract(x, y)
    want = pair_of_two_rows(x[0], y[0])
    assert dots[0].tobytes() == want[1].tobytes() == np.float32(-0.0).tobytes()
    assert cosines[0].tobytes() == want[0].tobytes() == np.float32(-0.0).tobytes()
    assert norms[0, 0] == 0 and norms[0, 1] == np.sqrt(np.float32(260))
    # one lane alone with -0.0 among ordinary lanes: lane 5's piece is -0.0, the others' are not zero
    x = np.ones((1, 260), dtype=np.float32)
    x[0, 20:24] = 0.0
    y = -np.ones((1, 260), dtype=np.float32)
    got = pairs_by_the_contract(x, y)
    want = pair_of_two_rows(x[0], y[0])
    assert (got[0][0].tobytes(), got[1][0].tobytes()) == (want[0].tobytes(), want[1].tobytes()) and got[1][0] == -256
    # the production restatement (a device='cpu' reader's) agrees
    from memb_amd.reader import pair_similarity_host
    host = pair_similarity_host(np.zeros((1, 260), dtype=np.float32), y)
    assert host[1][0].tobytes() == np.float32(-0.0).tobytes() and host[0][0].tobytes() == np.float32(-0.0).tobytes()


@pytest.mark.parametrize('dim', DIMS)
def test_host_function_has_the_references_bits(dim):
    from memb_amd.reader import pair_similarity_host, row_norms_host
    x, y = gaussian_pairs(dim, 200, 77 + dim)
    x, y, _ = with_special_pairs(x, y)
    want = pairs_by_the_contract(x, y)
    got = pair_similarity_host(x, y)
    assert all(bits_equal(one, other) for one, other in zip(got, want)), dim
    assert bits_equal(got[2][:, 0], row_norms_host(x)) and bits_equal(got[2][:, 1], row_norms_host(y))
    interleaved = np.empty((2 * len(x), dim), dtype=np.float32)
    interleaved[0::2], interleaved[1::2] = x, y
    assert all(bits_equal(one, other) for one, other in zip(pairs_of_rows(interleaved), want))


# ---- 2. a device='cpu' reader ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_host_reader_has_the_contracts_bits(native, make_model, storage, bits):
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows_a = np.concatenate([ids_with_misses(500, N_ROWS, 1), np.arange(100, dtype=np.uint32)])
    rows_b = np.concatenate([ids_with_misses(500, N_ROWS, 2), np.arange(100, dtype=np.uint32)])   # and 100 rows with themselves
    missing = (rows_a >= N_ROWS) | (rows_b >= N_ROWS)
    assert missing.any() and ((rows_a >= N_ROWS) & (rows_b >= N_ROWS)).any()
    want = pairs_by_the_contract(reader.rows_embedding(rows_a), reader.rows_embedding(rows_b))
    cosines = reader.pair_similarity(rows_a, rows_b)
    assert isinstance(cosines, np.ndarray) and cosines.dtype == np.float32 and cosines.shape == (600,)
    assert bits_equal(cosines, want[0]), storage
    assert not cosines[missing].any() and (np.abs(cosines[500:] - 1) <= 2.0 ** -22).all()
    got = reader.pair_similarity(rows_a, rows_b, return_dots=True, return_norms=True)
    assert len(got) == 3 and got[1].shape == (600,) and got[2].shape == (600, 2)
    assert all(part.dtype == np.float32 for part in got)
    assert all(bits_equal(one, other) for one, other in zip(got, want)), storage
    assert bits_equal(got[2][:, 0], reader.row_norms(rows_a)) and bits_equal(got[2][:, 1], reader.row_norms(rows_b))
    only_dots = reader.pair_similarity(rows_a, rows_b, return_dots=True)
    assert bits_equal(only_dots[0], want[0]) and bits_equal(only_dots[1], want[1]) and only_dots[2] is None
    only_norms = reader.pair_similarity(rows_a, rows_b, return_norms=True)
    assert only_norms[1] is None and bits_equal(only_norms[2], want[2])
    # n = 0
    none = np.zeros(0, dtype=np.uint32)
    assert reader.pair_similarity(none, none).shape == (0,)
    assert reader.pair_similarity(none, none, return_norms=True)[2].shape == (0, 2)
    with pytest.raises(ValueError, match='same length'):
        reader.pair_similarity(rows_a, rows_b[:-1])


def test_host_reader_works_in_bounded_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 64)
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows_a, rows_b = ids_with_misses(64 * 3 + 5, N_ROWS, 9), ids_with_misses(64 * 3 + 5, N_ROWS, 10)
    want = pairs_by_the_contract(reader.rows_embedding(rows_a), reader.rows_embedding(rows_b))
    got = reader.pair_similarity(rows_a, rows_b, return_dots=True, return_norms=True)
    assert all(bits_equal(one, other) for one, other in zip(got, want))


def test_special_rows_on_a_host_reader(native, tmp_path):
    path, vectors = special_model(native, tmp_path)
    reader = native.Reader(path, device='cpu')
    rows_a = np.array([0, 0, 2, 3, 5, 4, 5, 0xFFFFFFFF, 9], dtype=np.uint32)
    rows_b = np.array([0, 1, 3, 3, 5, 5, 77, 0xFFFFFFFF, 0], dtype=np.uint32)
    cosines, dots, norms = reader.pair_similarity(rows_a, rows_b, return_dots=True, return_norms=True)
    padded = np.concatenate([vectors, np.zeros((1, vectors.shape[1]), dtype=np.float32)])
    take = lambda rows: padded[np.minimum(rows, 6)]
    want = pairs_by_the_contract(take(rows_a), take(rows_b))
    assert bits_equal(cosines, want[0]) and bits_equal(dots, want[1]) and bits_equal(norms, want[2])
    assert 0 < dots[0] < np.float32(1.1754944e-38) and cosines[0] == dots[0] / np.float32(1e-12) ** 2 and cosines[1] == -cosines[0]
    assert dots[2].tobytes() == np.float32(-0.0).tobytes() and cosines[2].tobytes() == np.float32(-0.0).tobytes()   # +0 . -0
    assert dots[3] == 0 and not np.signbit(dots[3])                                                                  # -0 . -0
    assert abs(float(cosines[4]) - 1) <= 2.0 ** -22
    assert not cosines[6:].any() and not dots[6:].any()


def test_device_methods_refuse_a_host_reader(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    assert reader.last_pairs_kernel == ''
    for call in (lambda: reader.pair_similarity_device(None, None), lambda: reader.similarity_device(['a'], ['b'])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()


# ---- 3. the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip.h"' in text and '#include "memb_hip_norms.h"' in text
    assert '1.0000001' in text and 'ReadersUnion' in text
    # the headers it extends are as they were
    for name in ('memb_hip.h', 'memb_hip_norms.h'):
        assert 'memb_hip_pair' not in open(os.path.join(REPO, 'include', name)).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    # (device pointers are never read by a refused call: small aligned numbers stand for them)
    pairs = library.memb_hip_pair_similarity_device
    pairs.argtypes = [pointer, pointer, size, pointer, pointer, pointer, pointer]
    assert refused(pairs(None, 64, 5, 128, None, None, None), b'ctx')              # no context
    assert refused(pairs(None, None, 0, None, None, None, None), b'ctx')
    assert refused(pairs(None, None, 5, 128, None, None, None), b'pairs')          # no pairs, n > 0
    assert refused(pairs(None, 64, 5, None, None, None, None), b'at least one')    # no output, n > 0
    for arguments in ((66, 128, None, None), (64, 130, None, None), (64, None, 129, None), (64, None, None, 131)):
        assert refused(pairs(None, arguments[0], 5, *arguments[1:], None), b'aligned'), arguments
    assert refused(pairs(None, 64, 2 ** 36 + 1, 128, None, None, None), b'too large')

    dense = library.memb_hip_dense_pair_similarity_device
    dense.argtypes = [ctypes.c_int, pointer, size, size, size, pointer, pointer, pointer, pointer]
    assert refused(dense(0, None, 5, 300, 300, 128, None, None, None), b'values')
    assert refused(dense(0, 64, 5, 300, 300, None, None, None, None), b'at least one')
    for arguments in ((66, 128, None, None), (64, 130, None, None), (64, None, 129, None), (64, None, None, 131)):
        assert refused(dense(0, arguments[0], 0, 300, 300, *arguments[1:], None), b'aligned'), arguments
    assert refused(dense(0, 64, 2 ** 36 + 1, 300, 300, 128, None, None, None), b'too large')
    assert refused(dense(0, None, 0, 0, 0, None, None, None, None), b'dim')
    assert refused(dense(0, None, 0, 2 ** 32, 2 ** 32, None, None, None, None), b'dim')
    assert refused(dense(0, None, 0, 300, 299, None, None, None, None), b'ld_values')
    assert refused(dense(-1, None, 0, 300, 300, None, None, None, None), b'device')
    assert dense(0, None, 0, 300, 300, None, None, None, None) == 0                # n == 0: a no-op
    assert dense(0, 64, 0, 300, 300, 128, 132, 136, None) == 0

    name = library.memb_hip_pairs_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b'pairs_dense'
    count = library.memb_hip_pairs_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer]
    assert refused(count(None, None, 0, 1, 0, 0, None), b'null')
    assert refused(count(None, None, 2 ** 36 + 1, 1, 0, 0, None), b'too large')

    from memb_amd import _memb
    for binding in ('dense_pair_similarity_to_device', 'dense_pairs_kernel_name'):
        assert hasattr(_memb, binding)
    for method in ('pair_similarity_to_device', 'pairs_kernel_name', 'pairs_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    assert _memb.dense_pairs_kernel_name() == 'pairs_dense'
    for method in ('pair_similarity_device', 'similarity_device', 'pair_similarity', 'last_pairs_kernel'):
        assert hasattr(native.Reader, method)
