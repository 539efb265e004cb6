"""Cosine similarity of pairs of bags without a GPU: a device='cpu' reader bit for bit against the reference of
tests/bag_pairs_reference.py (include/memb_hip_bag_pairs.h's contract over reader.rows_embedding) and against the two-step
path a caller had before (bags_embedding, then pair_similarity_host), the reference against float64, the C header and the
entry points' refusals. (The byte count needs a staged model and is checked in tests/test_gpu_bag_pairs.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bag_pairs_reference import SELF_PAIR, bag_pair_lengths, bag_pairs_batch, bag_pairs_by_the_contract, entry_values
from conftest import REPO, bits_equal
from pooled_reference import offsets_of

HEADER = os.path.join(REPO, 'include', 'memb_hip_bag_pairs.h')
N_ROWS = 3000
PAIRS = 200
ACCURACY_DIMS = (1, 3, 4, 64, 255, 256, 260, 300, 512, 516, 1024)
# The largest |cos - cos64| of the numpy reference over ACCURACY_DIMS and both modes measured 3.07 * 2^-24 (dim 4, mean;
# DESIGN.md section 5.9 has every dim): four times that is 12.3 * 2^-24, rounded up to a power of two. The margin covers
# other seeds.
ACCURACY_BOUND = 2.0 ** -20


def test_the_batch_holds_its_edges():
    for words in (1, 2, 4, 7, 21, 64):
        lengths = bag_pair_lengths(words, PAIRS, 3).reshape(-1, 2)
        offsets = offsets_of(lengths.reshape(-1))
        assert len(lengths) == PAIRS and len(offsets) == 2 * PAIRS + 1
        assert {0, 1, max(words - 1, 1), words, words + 1, 2 * words + 1, 300} <= set(lengths.reshape(-1).tolist())
        assert ((lengths[:, 0] == 0) & (lengths[:, 1] == 0)).any() and ((lengths[:, 0] == 0) & (lengths[:, 1] > 0)).any()
        first_begin, first_end = offsets[0:-1:2], offsets[1::2]
        on_a_boundary = (first_begin % words == 0) & (first_end % words == 0) & (first_end > first_begin)
        assert on_a_boundary[0] and on_a_boundary[10], words
        if words > 1:
            assert (first_end % words != 0).any() and ((offsets[2::2] - 1) // words > first_begin // words).any()
        rows, again = bag_pairs_batch(words, PAIRS, N_ROWS, 3)
        assert np.array_equal(again, offsets) and len(rows) == offsets[-1] and (rows >= N_ROWS).any()
        first, second, end = (int(offsets[2 * SELF_PAIR + k]) for k in range(3))
        assert np.array_equal(rows[first:second], rows[second:end]) and second > first
    for pairs in (0, 1, 2, 3):
        rows, offsets = bag_pairs_batch(4, pairs, N_ROWS, 1)
        assert len(offsets) == 2 * pairs + 1 and len(rows) == offsets[-1]


# ---- 1. a device='cpu' reader ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
@pytest.mark.parametrize('mode', ('sum', 'mean'))
def test_host_reader_has_the_contracts_bits(native, make_model, storage, bits, mode):
    from memb_amd.reader import pair_similarity_host
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows, offsets = bag_pairs_batch(4, PAIRS, N_ROWS, 11)
    want = bag_pairs_by_the_contract(entry_values(reader, rows), offsets, mode)
    assert (want[0] != 0).any() and abs(float(want[0][SELF_PAIR]) - 1) <= 2.0 ** -22
    cosines = reader.bag_pair_similarity(rows, offsets, mode)
    assert isinstance(cosines, np.ndarray) and cosines.dtype == np.float32 and cosines.shape == (PAIRS,)
    assert bits_equal(cosines, want[0]), (storage, mode)
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.bag_pair_similarity(rows, offsets, mode=mode, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and bits_equal(got[0], want[0]), (storage, mode, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms)
        if dots:
            assert got[1].dtype == np.float32 and got[1].shape == (PAIRS,) and bits_equal(got[1], want[1])
        if norms:
            assert got[2].dtype == np.float32 and got[2].shape == (PAIRS, 2) and bits_equal(got[2], want[2])
    # the two-step path of before: both sides pooled, then the pair contract over the pooled rows
    pooled = reader.bags_embedding(rows, offsets, mode=mode)
    two_steps = pair_similarity_host(pooled[0::2], pooled[1::2])
    assert all(bits_equal(one, other) for one, other in zip(two_steps, want)), (storage, mode)
    from memb_amd.reader import row_norms_host
    assert bits_equal(want[2][:, 0], row_norms_host(pooled[0::2])) and bits_equal(want[2][:, 1], row_norms_host(pooled[1::2]))
    # empty and missing-only bags give zeros, never a NaN
    assert not np.isnan(cosines).any() and cosines[3] == 0 and cosines[1] == 0


def test_host_reader_offsets_and_refusals(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows, offsets = bag_pairs_batch(4, 7, N_ROWS, 5)
    want = bag_pairs_by_the_contract(entry_values(reader, rows), offsets, 'mean')
    # 2 * pairs + 1 offsets, an odd number, of any integer type or a list
    assert len(offsets) % 2 == 1
    for given in (offsets, offsets.astype(np.uint32), offsets.astype(np.int32), [int(value) for value in offsets]):
        assert bits_equal(reader.bag_pair_similarity(rows, given), want[0])
    with pytest.raises(ValueError, match='odd number'):
        reader.bag_pair_similarity(rows, offsets[:-1])
    with pytest.raises(ValueError, match='odd number'):
        reader.bag_pair_similarity(rows, offsets[:2])
    with pytest.raises(ValueError, match='ascend'):
        reader.bag_pair_similarity(rows, offsets[::-1].copy())
    with pytest.raises(ValueError, match='len\\(rows\\)'):
        reader.bag_pair_similarity(rows, offsets + 1)
    with pytest.raises(ValueError, match="'sum' or 'mean'"):
        reader.bag_pair_similarity(rows, offsets, mode='max')
    # no pair, and no entry
    none = np.zeros(0, dtype=np.uint32)
    assert reader.bag_pair_similarity(none, [0]).shape == (0,)
    assert reader.bag_pair_similarity(none, [0], return_norms=True)[2].shape == (0, 2)
    zero_bags = reader.bag_pair_similarity(none, [0, 0, 0, 0, 0], return_dots=True, return_norms=True)
    assert all(not part.any() and not np.signbit(part).any() for part in zero_bags) and zero_bags[0].shape == (2,)
    # device methods refuse a host reader, sentence lists must match
    assert reader.last_bag_pairs_kernel == ''
    for call in (lambda: reader.bag_pair_similarity_device(None, None), lambda: reader.sentence_similarity_device([['a']], [['b']])):
        with pytest.raises(RuntimeError, match="device 'cpu'"):
            call()
    with pytest.raises(ValueError, match='same length'):
        reader.sentence_similarity_device([['a'], ['b']], [['c']])
    with pytest.raises(ValueError, match="'sum' or 'mean'"):
        reader.sentence_similarity_device([['a']], [['c']], mode='max')


def test_host_reader_works_in_bounded_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # slices of 8 pairs
    monkeypatch.setattr(memb_amd.reader, 'BAGS_HOST_CHUNK', 64)    # and of 64 entries: the long bag spans several
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows, offsets = bag_pairs_batch(4, 43, N_ROWS, 9)
    for mode in ('sum', 'mean'):
        want = bag_pairs_by_the_contract(entry_values(reader, rows), offsets, mode)
        got = reader.bag_pair_similarity(rows, offsets, mode, return_dots=True, return_norms=True)
        assert all(bits_equal(one, other) for one, other in zip(got, want)), mode


# ---- 2. the reference against float64 ----

def test_reference_is_close_to_float64():
    from pooled_reference import pooled_by_the_contract
    worst_of_all = 0.0
    for dim in ACCURACY_DIMS:
        rng = np.random.default_rng(2000 + dim)
        pairs = 150
        lengths = rng.integers(1, 41, size=2 * pairs)
        offsets = offsets_of(lengths)
        values = rng.standard_normal((int(offsets[-1]), dim)).astype(np.float32)
        # every third pair shares most of its entries, so that cosines near 1 are among them
        for pair in range(0, pairs, 3):
            a, b, end = (int(offsets[2 * pair + k]) for k in range(3))
            shared = min(b - a, end - b)
            values[b:b + shared] = values[a:a + shared]
        for mode in ('sum', 'mean'):
            cosines, _, _ = bag_pairs_by_the_contract(values, offsets, mode)
            pooled = pooled_by_the_contract(values, offsets, mode).astype(np.float64)   # the same fp32 pooled rows
            x, y = pooled[0::2], pooled[1::2]
            exact = (x * y).sum(axis=1) / (np.sqrt((x * x).sum(axis=1)) * np.sqrt((y * y).sum(axis=1)))
            worst = float(np.abs(cosines.astype(np.float64) - exact).max())
            print('dim', dim, mode, 'worst |cos - cos64| =', worst / 2.0 ** -24, '* 2^-24')
            worst_of_all = max(worst_of_all, worst)
            assert worst <= ACCURACY_BOUND, (dim, mode, worst)
            assert np.abs(cosines).max() <= 1 + 2.0 ** -22
    print('worst of all =', worst_of_all / 2.0 ** -24, '* 2^-24')


# ---- 3. the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_pooled.h"' in text and '#include "memb_hip_pairs.h"' in text
    # the sentence that is both the fallback and the second oracle, and what is not built
    assert 'memb_hip_pool_rows_device, then' in text and 'memb_hip_dense_pair_similarity_device over it' in text
    for word in ("missing='skip'", 'chunked order', 'bf16 / fp16', 'ReadersUnion', 'sharded readers', 'against many'):
        assert word in text, word
    # the headers it extends are as they were
    for name in ('memb_hip.h', 'memb_hip_pooled.h', 'memb_hip_pairs.h', 'memb_hip_norms.h'):
        assert 'memb_hip_bag_pair' not in open(os.path.join(REPO, 'include', name)).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    # (without a context every call is refused before any pointer is read: the refusals that need one -- rows, offsets,
    # outputs, mode, alignment, size -- are checked with a staged model in tests/test_gpu_bag_pairs.py)
    pairs = library.memb_hip_bag_pair_similarity_device
    pairs.argtypes = [pointer, pointer, size, pointer, size, ctypes.c_int, pointer, pointer, pointer, pointer]
    assert refused(pairs(None, 64, 5, 128, 2, 1, 256, None, None, None), b'ctx')
    assert refused(pairs(None, None, 0, None, 0, 1, None, None, None, None), b'ctx')
    name = library.memb_hip_bag_pairs_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b''
    count = library.memb_hip_bag_pairs_algorithmic_bytes
    count.argtypes = [pointer, pointer, size, pointer, size, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer]
    assert refused(count(None, None, 0, None, 0, 1, 0, 0, None), b'null')
    assert refused(count(None, None, 0, None, 2 ** 35 + 1, 1, 0, 0, None), b'too large')

    from memb_amd import _memb
    for method in ('bag_pair_similarity_to_device', 'bag_pairs_kernel_name', 'bag_pairs_algorithmic_bytes'):
        assert hasattr(_memb.Reader, method)
    for method in ('bag_pair_similarity_device', 'sentence_similarity_device', 'bag_pair_similarity', 'last_bag_pairs_kernel'):
        assert hasattr(native.Reader, method)
