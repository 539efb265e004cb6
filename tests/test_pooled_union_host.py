"""Pooled lookups of a ReadersUnion without a GPU: pooled_rows of a union of device='cpu' readers against the explicit
loop of the contract (include/memb_hip_pooled_union.h) over the readers' own rows merged in numpy float32, the argument
checks, and what the device methods and the old one-array stubs answer."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_reference import merged_rows, offsets_of, pooled_by_the_contract, union_ids

N_ROWS = 3000


@pytest.fixture(scope='module')
def host_readers(native, make_model):
    models = [make_model(N_ROWS, 300, 'trained', 4, seed=11), make_model(N_ROWS, 300, 'trained', 6, seed=12),
              make_model(N_ROWS, 64, 'uniform', 8, seed=13)]
    return [native.Reader(path, device='cpu') for path, _ in models]


@pytest.mark.parametrize('union_mode', ['average', 'concatenate'])
@pytest.mark.parametrize('chunk', [None, 37])
def test_host_union_pools_by_the_contract(native, host_readers, monkeypatch, union_mode, chunk):
    from memb_amd import readers_union
    if chunk:   # slice boundaries inside bags
        monkeypatch.setattr(readers_union, 'POOLED_HOST_CHUNK', chunk)
    readers = host_readers if union_mode == 'concatenate' else host_readers[:2]
    union = native.ReadersUnion(readers, union_mode)
    lengths = [0, 0, 5, 1, 0, 12, 100, 0, 3, 64, 41, 0, 9, 0]
    rows = union_ids(sum(lengths), len(readers), 3, N_ROWS)
    values = merged_rows(union_mode, [reader.rows_embedding(ids) for reader, ids in zip(readers, rows)])
    for mode in ('sum', 'mean'):
        got = union.pooled_rows(rows, offsets_of(lengths), mode=mode)
        assert got.dtype == np.float32 and got.shape == (len(lengths), union.dim)
        assert bits_equal(got, pooled_by_the_contract(values, offsets_of(lengths), mode)), (union_mode, mode, chunk)
    ones = union.pooled_rows(rows, np.arange(sum(lengths) + 1), mode='mean')
    assert bits_equal(ones, values)
    empty = union.pooled_rows([np.zeros(0, dtype=np.uint32)] * len(readers), [0, 0, 0], mode='mean')
    assert empty.shape == (2, union.dim) and not empty.any() and not np.signbit(empty).any()


def test_three_host_readers_average_in_reader_order(native, make_model):
    readers = [native.Reader(make_model(N_ROWS, 300, 'trained', 4, seed=20 + position)[0], device='cpu') for position in range(3)]
    union = native.ReadersUnion(readers, 'average')
    lengths = np.random.default_rng(5).geometric(1 / 6.0, size=60)
    rows = union_ids(int(lengths.sum()), 3, 9, N_ROWS)
    values = merged_rows('average', [reader.rows_embedding(ids) for reader, ids in zip(readers, rows)])
    assert bits_equal(union.pooled_rows(rows, offsets_of(lengths), mode='mean'), pooled_by_the_contract(values, offsets_of(lengths), 'mean'))


def test_argument_checks(native, host_readers):
    union = native.ReadersUnion(host_readers[:2], 'average')
    rows = union_ids(20, 2, 1, N_ROWS)
    with pytest.raises(ValueError, match='sum'):
        union.pooled_rows(rows, [0, 20], mode='max')
    with pytest.raises(ValueError, match='one row-id array per reader'):
        union.pooled_rows(rows[:1], [0, 20])
    with pytest.raises(ValueError, match='one row-id array per reader'):
        union.pooled_rows(rows[0], [0, 20])
    with pytest.raises(ValueError, match='equal length'):
        union.pooled_rows([rows[0], rows[1][:-1]], [0, 19])
    with pytest.raises(ValueError, match='ascend'):
        union.pooled_rows(rows, [0, 10, 5, 20])
    with pytest.raises(ValueError, match='0 .. len'):
        union.pooled_rows(rows, [0, 21])
    with pytest.raises(ValueError, match='integers'):
        union.pooled_rows(rows, [0.0, 20.0])

    class Fake:
        dim = 300
    with pytest.raises(TypeError, match='Reader'):
        native.ReadersUnion([host_readers[0], Fake()], 'average').pooled_rows(rows, [0, 20])


def test_device_methods_refuse_host_readers(native, host_readers):
    union = native.ReadersUnion(host_readers[:2], 'average')
    assert union.last_pooled_kernel == ''
    with pytest.raises(RuntimeError, match='host'):
        union.pooled_rows_device([None, None], None)
    with pytest.raises(RuntimeError, match='host'):
        union.pooled_sentences_device([['a']])
    with pytest.raises(RuntimeError, match='host'):
        union.resolve_rows_device(['a'])
    with pytest.raises(ValueError, match='sum'):
        union.pooled_rows_device([None, None], None, mode='max')

    class Fake:
        dim = 300
        device = 'cpu'
    with pytest.raises(TypeError, match='Reader'):
        native.ReadersUnion([host_readers[0], Fake()], 'average').pooled_rows_device([None, None], None)
    assert union.last_pooled_kernel == ''


def test_the_one_array_stubs_still_refuse(native, host_readers):
    union = native.ReadersUnion(host_readers[:2], 'average')
    for method in (union.bags_embedding_device, union.bags_embedding, union.sentences_embedding_device):
        with pytest.raises(NotImplementedError, match='ReadersUnion'):
            method(np.zeros(1, dtype=np.uint32), [0, 1])
