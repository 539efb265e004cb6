"""reduction='chunked' of a device='cpu' reader (Reader.bags_embedding): the contract of include/memb_hip_pooled_chunked.h
on the host, against the explicit numpy loop of tests/pooled_chunked_reference.py. Bit for bit; no GPU."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_chunked_reference import (LONGEST, UNKNOWN, chunked_by_the_contract, contract_batch, contract_lengths, in_order,
                                      inner_batches, offsets_of, sequential_by_the_contract)

N_ROWS = 3000


@pytest.fixture(scope='module')
def reader(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    return native.Reader(path, device='cpu')


def test_the_chunk_is_a_constant_of_the_api(native):
    assert native.POOL_CHUNK in (32, 64)
    assert native.POOL_CHUNK % 8 == 0 and native.POOL_CHUNK & (native.POOL_CHUNK - 1) == 0


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8), ('full', 32)])
def test_the_host_path_against_the_contract(native, make_model, storage, bits):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    rows, offsets = contract_batch(chunk, N_ROWS, 11)
    assert [int(length) for length in offsets[1:] - offsets[:-1]] == contract_lengths(chunk) and offsets[0] == 3
    values = reader.rows_embedding(rows)
    for mode in ('sum', 'mean'):
        want, _ = chunked_by_the_contract(values, rows, offsets, N_ROWS, mode, False, chunk)
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, reduction='chunked'), want), (mode, 'zero')
        want, want_counts = chunked_by_the_contract(values, rows, offsets, N_ROWS, mode, True, chunk)
        got, counts = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked')
        assert bits_equal(got, want) and np.array_equal(counts, want_counts) and counts.dtype == np.uint32, (mode, 'skip')
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, missing='skip', reduction='chunked'), want)


def test_the_new_order_is_another_order(native, reader):
    chunk = native.POOL_CHUNK
    rows, offsets = contract_batch(chunk, N_ROWS, 11)
    values = reader.rows_embedding(rows)
    sequential, _ = sequential_by_the_contract(values, rows, offsets, N_ROWS, 'sum', False)
    chunked = reader.bags_embedding(rows, offsets, mode='sum', reduction='chunked')
    assert (sequential[LONGEST].view(np.uint32) != chunked[LONGEST].view(np.uint32)).any()
    assert bits_equal(reader.bags_embedding(rows, offsets, mode='sum'), sequential)   # (and the default is the old one)
    assert bits_equal(reader.bags_embedding(rows, offsets, mode='sum', reduction='sequential'), sequential)


def test_bags_of_at_most_one_chunk_have_the_sequential_bits(native, reader):
    chunk = native.POOL_CHUNK
    rng = np.random.default_rng(5)
    lengths = np.concatenate([[0, chunk, 1, chunk], rng.integers(0, chunk + 1, size=200)])
    rows = rng.integers(0, N_ROWS, size=int(lengths.sum())).astype(np.uint32)
    rows[::5] = UNKNOWN
    offsets = offsets_of(lengths)
    for mode in ('sum', 'mean'):
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, reduction='chunked'),
                          reader.bags_embedding(rows, offsets, mode=mode))
        chunked = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked')
        sequential = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True)
        assert bits_equal(chunked[0], sequential[0]) and np.array_equal(chunked[1], sequential[1])


def test_entries_outside_the_bags_belong_to_no_bag(native, reader):
    chunk = native.POOL_CHUNK
    for name, rows, offsets in inner_batches(chunk, N_ROWS, 13):
        assert offsets[-1] < len(rows)
        values = reader.rows_embedding(rows)
        for mode in ('sum', 'mean'):
            for skip in (False, True):
                want, want_counts = chunked_by_the_contract(values, rows, offsets, N_ROWS, mode, skip, chunk)
                got, counts = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked') \
                    if skip else (reader.bags_embedding(rows, offsets, mode=mode, reduction='chunked'), want_counts)
                assert bits_equal(got, want) and np.array_equal(counts, want_counts), (name, mode, skip)
                short = np.nonzero(offsets[1:] - offsets[:-1] <= chunk)[0]   # at most one chunk: the sequential bits
                sequential = reader.bags_embedding(rows, offsets, mode=mode, missing='skip' if skip else 'zero')
                assert bits_equal(got[short], sequential[short]), (name, mode, skip)


def signed_zero_model(native, directory):
    """A `full` model whose row 0 is all -0.0 and whose rows 1 and 2 are subnormal with mixed signs, -0.0 in their first
    columns."""
    rng = np.random.default_rng(41)
    count, dim = 40, 300
    vectors = rng.integers(-70000, 70000, size=(count, dim)).astype(np.float32) * np.float32(1.4e-45)
    vectors[0] = -0.0
    vectors[1, :50] = -0.0
    vectors[2, :30] = -0.0
    assert (np.abs(vectors) < 1.1754944e-38).all() and (vectors[1] > 0).any() and (vectors[1] < 0).any()
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['s{:04d}'.format(i) for i in range(count)], vectors)
    path = str(directory / 'signed_zero.bin')
    builder.save(path)
    return path, count


def skip_cases(chunk, count):
    """(rows, offsets): a bag of 3 C entries -- first chunk: one known row of -0.0 among unknown entries, middle chunk all
    0xFFFFFFFF, last chunk rows 0, 1, 2 and then row 0 again and again -- a bag of 2 C + 3 unknown entries, and a bag of
    3 C + 1 subnormal rows."""
    first = np.full(chunk, UNKNOWN, dtype=np.uint32)
    first[chunk // 2] = 0
    middle = np.full(chunk, UNKNOWN, dtype=np.uint32)
    last = np.zeros(chunk, dtype=np.uint32)
    last[:3] = [0, 1, 2]
    unknown = np.full(2 * chunk + 3, UNKNOWN, dtype=np.uint32)
    unknown[5] = count   # (an id that is not in the model is unknown too)
    subnormal = (np.arange(3 * chunk + 1) % (count - 1) + 1).astype(np.uint32)
    rows = np.concatenate([first, middle, last, unknown, subnormal])
    return rows, offsets_of([3 * chunk, len(unknown), len(subnormal)])


def check_skip_cases(result, counts, values, rows, offsets, count, chunk):
    """result, counts: mode='sum', missing='skip' of skip_cases; values: the entries' rows."""
    want, want_counts = chunked_by_the_contract(values, rows, offsets, count, 'sum', True, chunk)
    assert bits_equal(result, want) and np.array_equal(counts, want_counts)
    assert counts[0] == 1 + chunk and counts[1] == 0 and counts[2] == 3 * chunk + 1
    last = in_order(values[2 * chunk:3 * chunk])   # the last chunk's sum: -0.0 where rows 0, 1 and 2 all are
    negative_zero = (last == 0) & np.signbit(last)
    assert negative_zero[:30].all() and not negative_zero.all()
    # -0.0 (the first chunk) + nothing (the middle one) + last = last, -0.0 included; a +0.0 from the middle chunk or from
    # the first chunk's unknown entries would have turned those columns into +0.0
    assert bits_equal(result[0], last)
    assert not result[1].any() and not np.signbit(result[1]).any()   # no known entry: +0.0
    assert (result[2] != 0).any() and (np.abs(result[2]) < 1.1754944e-38).all()   # subnormal partial sums are kept


def test_skipped_chunks_add_nothing(native, tmp_path):
    chunk = native.POOL_CHUNK
    path, count = signed_zero_model(native, tmp_path)
    reader = native.Reader(path, device='cpu')
    rows, offsets = skip_cases(chunk, count)
    values = reader.rows_embedding(rows)
    result, counts = reader.bags_embedding(rows, offsets, mode='sum', missing='skip', return_counts=True, reduction='chunked')
    check_skip_cases(result, counts, values, rows, offsets, count, chunk)
    zero = reader.bags_embedding(rows, offsets, mode='sum', reduction='chunked')
    assert not zero[0][:30].any() and not np.signbit(zero[0][:30]).any()   # where unknown entries count, +0.0 + -0.0 = +0.0


def test_another_reduction_is_refused(native, reader):
    rows, offsets = np.arange(10, dtype=np.uint32), np.array([0, 4, 10])
    with pytest.raises(ValueError, match='reduction'):
        reader.bags_embedding(rows, offsets, reduction='tree')
    with pytest.raises(ValueError, match='reduction'):
        reader.bags_embedding(rows, offsets, reduction=None)
