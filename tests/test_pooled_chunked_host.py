"""reduction='chunked' of a device='cpu' reader (Reader.bags_embedding): the contract of include/memb_hip_pooled_chunked.h
on the host, against the explicit numpy loop of tests/pooled_reference.py. Bit for bit; no GPU. Also what
tests/test_gpu_pooled_chunked_geometry.py relies on before it runs: its batch builders, and that the side-by-side reference
it uses for very many bags has the bits of the per-bag loop."""
import os
import re

import numpy as np
import pytest

import pooled_reference as reference
from conftest import REPO, bits_equal
from pooled_reference import (COLUMN_DIMS, COLUMN_ROWS, COLUMN_STORAGES, EDGE_CHUNK_COUNTS, LONGEST, PLAN_BAG_COUNTS, UNKNOWN,
                              UNKNOWN_CHUNKS, WIDE_MODELS, check_negative_zeros_survive, check_skip_cases, chunked_by_the_contract,
                              chunked_side_by_side, column_batch, contract_batch, contract_lengths, edge_batch, inner_batches,
                              offsets_of, plan_batch, sequential_by_the_contract, signed_zero_model, signed_zero_rows, skip_cases,
                              wide_batch, with_unknown_chunks)

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


# ---- the batches and the reference of tests/test_gpu_pooled_chunked_geometry.py, on the host ----

def host_check(reader, rows, offsets, chunk, context, by_the_contract=chunked_by_the_contract, modes=('sum', 'mean')):
    """device='cpu' bags_embedding(reduction='chunked') against R1, both `missing` modes, with the counts."""
    values = reader.rows_embedding(rows)
    for mode in modes:
        for skip in (False, True):
            want, want_counts = by_the_contract(values, rows, offsets, len(reader), mode, skip, chunk)
            if skip:
                got, counts = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked')
                assert np.array_equal(counts, want_counts), (context, mode, 'counts')
            else:
                got = reader.bags_embedding(rows, offsets, mode=mode, reduction='chunked')
            assert bits_equal(got, want), (context, mode, skip)


def test_the_plan_constants_are_the_headers():
    with open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_pooled_chunked.h')) as header:
        text = header.read()
    constant = lambda name: re.search(r'constexpr uint32_t {} = ([^;]+);'.format(name), text).group(1).strip()   # noqa: E731
    assert int(constant('PLAN_THREADS')) == reference.PLAN_THREADS
    assert int(constant('PLAN_BAGS_PER_THREAD')) == reference.PLAN_BAGS_PER_THREAD
    assert constant('PLAN_BAGS_PER_BLOCK') == 'PLAN_THREADS * PLAN_BAGS_PER_THREAD'
    assert reference.PLAN_BAGS_PER_BLOCK == 2048 and reference.PLAN_THREADS == 256   # (what the issue's bag counts assume)
    bags = len(reference.second_round_batch(64, 100, 0)[1]) - 1
    assert -(-bags // reference.PLAN_BAGS_PER_BLOCK) > reference.PLAN_THREADS        # a second round of chunk_scan_sums


def test_the_side_by_side_reference_has_the_bits_of_the_loop(native, make_model, reader):
    chunk = native.POOL_CHUNK
    small_path, _ = make_model(600, 8, 'trained', 4)
    small = native.Reader(small_path, device='cpu')
    rng = np.random.default_rng(17)
    lengths = np.minimum(rng.geometric(1 / 6.0, size=5000) - 1, chunk)
    lengths[::97] = chunk
    lengths[5::101] = chunk - 1
    short_rows = rng.integers(0, 600, size=int(lengths.sum())).astype(np.uint32)
    short_rows[::7] = UNKNOWN
    short_rows[3::11] = 600 + 5
    rows, offsets = contract_batch(chunk, N_ROWS, 11)
    beyond = np.array([0, chunk + 1, len(rows) - 1, len(rows) + 5, 0xFFFFFFFF], dtype=np.int64)   # clamped, as the kernels clamp
    for source, batch_rows, batch_offsets in ((reader, rows, offsets), (reader, rows, beyond), (small, short_rows, offsets_of(lengths))):
        values = source.rows_embedding(batch_rows)
        for mode in ('sum', 'mean'):
            for skip in (False, True):
                want, want_counts = chunked_by_the_contract(values, batch_rows, batch_offsets, len(source), mode, skip, chunk)
                got, counts = chunked_side_by_side(values, batch_rows, batch_offsets, len(source), mode, skip, chunk)
                assert bits_equal(got, want) and np.array_equal(counts, want_counts) and counts.dtype == np.uint32, (mode, skip)


@pytest.mark.parametrize('bags', [count for count in PLAN_BAG_COUNTS if count <= 2 * reference.PLAN_BAGS_PER_BLOCK + 1])
def test_plan_sizes_on_the_host(native, make_model, bags):
    chunk = native.POOL_CHUNK
    path, _ = make_model(600, 6, 'trained', 4)
    host = native.Reader(path, device='cpu')
    rows, offsets = plan_batch(chunk, bags, 600, bags)
    lengths = offsets[1:] - offsets[:-1]
    assert len(lengths) == bags and lengths[0] >= 2 * chunk + 1 and lengths[-1] >= 2 * chunk + 1 and (rows[::7] == UNKNOWN).all()
    for edge in range(reference.PLAN_BAGS_PER_BLOCK, bags, reference.PLAN_BAGS_PER_BLOCK):
        assert lengths[edge - 1] >= 2 * chunk + 1 and lengths[edge] >= 2 * chunk + 1
    assert {2 * chunk + 1, 9 * chunk}.issuperset(lengths[lengths > 2]) and (bags < 2 or (lengths == 9 * chunk).any())
    host_check(host, rows, offsets, chunk, bags, by_the_contract=chunked_side_by_side)


def test_the_batch_edges_of_pool_chunks_on_the_host(native, reader, tmp_path):
    chunk = native.POOL_CHUNK
    rows, offsets = edge_batch(chunk, N_ROWS, 23)
    assert offsets[0] == 3 and [-(-int(length) // chunk) for length in offsets[1:] - offsets[:-1]] == EDGE_CHUNK_COUNTS
    assert {int(length) % chunk for length in offsets[1:] - offsets[:-1]} == {1, chunk - 1, 0}
    values = reader.rows_embedding(rows)
    for skip in (False, True):   # the batch can tell the two orders apart
        chunked, _ = chunked_by_the_contract(values, rows, offsets, N_ROWS, 'sum', skip, chunk)
        sequential, _ = sequential_by_the_contract(values, rows, offsets, N_ROWS, 'sum', skip)
        assert not bits_equal(chunked[1:], sequential[1:]) and bits_equal(chunked[0], sequential[0])
    host_check(reader, rows, offsets, chunk, 'edges')
    rows_back, offsets_back = edge_batch(chunk, N_ROWS, 24, reverse=True)
    assert len(rows_back) == len(rows) and len(offsets_back) == len(offsets) and not np.array_equal(offsets_back, offsets)
    host_check(reader, rows_back, offsets_back, chunk, 'edges, longest first', modes=('mean',))
    path, count = signed_zero_model(native, tmp_path)
    signed = native.Reader(path, device='cpu')
    for which in UNKNOWN_CHUNKS:
        holes = signed_zero_rows(with_unknown_chunks(rows, offsets, chunk, which))
        check_negative_zeros_survive(signed, holes, offsets, chunk)
        host_check(signed, holes, offsets, chunk, ('signed zeros', which), modes=('sum',))


@pytest.mark.parametrize('storage,bits', COLUMN_STORAGES)
def test_column_blocks_on_the_host(native, make_model, storage, bits):
    chunk = native.POOL_CHUNK
    for dim in COLUMN_DIMS:
        path, _ = make_model(COLUMN_ROWS, dim, storage, bits, seed=dim)
        rows, offsets = column_batch(chunk, COLUMN_ROWS, dim)
        assert [int(length) for length in offsets[1:] - offsets[:-1]] == [1, chunk, 0, chunk + 1, 2 * chunk + 1, 9 * chunk + 5]
        host_check(native.Reader(path, device='cpu'), rows, offsets, chunk, (storage, dim))


@pytest.mark.parametrize('storage,bits,dim,count', WIDE_MODELS)
def test_very_wide_rows_on_the_host(native, make_model, storage, bits, dim, count):
    chunk = native.POOL_CHUNK
    path, _ = make_model(count, dim, storage, bits, seed=dim)
    rows, offsets = wide_batch(chunk, count, dim)
    assert len(offsets) == 13 and 2 * chunk + 1 in offsets[1:] - offsets[:-1]
    host_check(native.Reader(path, device='cpu'), rows, offsets, chunk, (storage, dim), modes=('mean',))
