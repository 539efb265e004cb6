"""bags_embedding on a device='cpu' reader: the contract of include/memb_hip_pooled.h executed without a GPU, bit for bit
against the contract's explicit loop (tests/pooled_reference.py) over reader.rows_embedding(rows)."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_reference import offsets_of, pooled_by_the_contract


def mixed_bags(count, seed):
    """bag lengths with empty bags at the start, in the middle and at the end, bags of one entry and long ones"""
    rng = np.random.default_rng(seed)
    lengths = [0, 0, 1, 1, 7, 8, 9, 17, 0, 1, 300] + list(rng.geometric(0.15, size=40)) + [0, 2, 0]
    lengths = np.array(lengths, dtype=np.int64)
    lengths[-4] += max(0, count - lengths.sum())
    return offsets_of(lengths)


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_host_bags_match_the_explicit_loop(native, make_model, storage, bits):
    path, _ = make_model(3000, 300, storage, bits)
    reader = native.Reader(path, device='cpu')
    offsets = mixed_bags(1200, bits)
    n = int(offsets[-1])
    rng = np.random.default_rng(7)
    rows = rng.integers(0, 3000, size=n, dtype=np.int64)
    rows[::5] = 0xFFFFFFFF          # missing rows inside bags: +0.0, and they count
    rows[3::13] = 3000 + 11         # ids >= n_rows too
    rows = rows.astype(np.uint32)
    values = reader.rows_embedding(rows)
    assert not values[rows >= 3000].any()
    for mode in ('sum', 'mean'):
        got = reader.bags_embedding(rows, offsets, mode=mode)
        assert got.dtype == np.float32 and got.shape == (len(offsets) - 1, 300)
        assert bits_equal(got, pooled_by_the_contract(values, offsets, mode)), (storage, mode)
    # every bag of one entry: the rows themselves
    assert bits_equal(reader.bags_embedding(rows, np.arange(n + 1), mode='sum'), values)
    assert bits_equal(reader.bags_embedding(rows, np.arange(n + 1), mode='mean'), values)
    # no bags, no entries
    assert reader.bags_embedding(rows, [0]).shape == (0, 300)
    empty = reader.bags_embedding(np.zeros(0, dtype=np.uint32), [0, 0, 0])
    assert empty.shape == (2, 300) and bits_equal(empty, np.zeros((2, 300), dtype=np.float32))


def test_host_bags_span_chunks(native, make_model, monkeypatch):
    # bags that straddle the bounded chunks of the host path, one bag longer than several chunks
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'BAGS_HOST_CHUNK', 64)
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    offsets = offsets_of([3, 60, 1, 0, 200, 64, 64, 5, 0, 0, 31])
    rows = np.random.default_rng(3).integers(0, 3100, size=int(offsets[-1])).astype(np.uint32)
    values = reader.rows_embedding(rows)
    for mode in ('sum', 'mean'):
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode), pooled_by_the_contract(values, offsets, mode))


def test_exact_values_signed_zeros_and_subnormals(native, tmp_path):
    # a `full` model holds the floats it is given: -0.0, subnormals of both signs, sums that stay subnormal, cancellation
    tiny = np.float32(1e-40)
    vectors = np.array([
        [-0.0, 0.0, tiny, -tiny, 3e-39, 1.0],
        [-0.0, -0.0, tiny, tiny, -2e-39, -1.0],
        [0.0, -0.0, -3 * tiny, 2 * tiny, 1e-45, 1e-8],
        [1e30, -1e30, 1e-45, -1e-45, 1.1754942e-38, 2.5],
        [-1e30, 1e30, 7e-41, 9e-41, -1.1754942e-38, 1e-3],
    ], dtype=np.float32)
    words = ['w{}'.format(i) for i in range(len(vectors))]
    builder = native.Builder(vectors.shape[1], 'full', 8)
    builder.add_words(words, vectors)
    path = str(tmp_path / 'exact.bin')
    builder.save(path)
    reader = native.Reader(path, device='cpu')
    rows = np.array([0, 1, 0, 2, 1, 3, 4, 2, 0xFFFFFFFF, 1, 2, 2, 3, 4, 0, 4, 3, 1, 2], dtype=np.uint32)
    offsets = np.array([0, 1, 2, 2, 4, 5, 8, 10, 13, 19], dtype=np.int64)
    values = reader.rows_embedding(rows)
    assert bits_equal(values[0], vectors[0]) and np.signbit(values[0][0])
    assert (np.abs(values[:8])[(values[:8] != 0)] < 1.2e-38).any()   # subnormals are among the addends
    for mode in ('sum', 'mean'):
        got = reader.bags_embedding(rows, offsets, mode=mode)
        want = pooled_by_the_contract(values, offsets, mode)
        assert bits_equal(got, want), mode
    got = reader.bags_embedding(rows, offsets, mode='sum')
    assert np.signbit(got[0][0]) and got[0][0] == 0          # a bag of one entry keeps -0.0
    assert not np.signbit(got[2]).any() and not got[2].any()   # an empty bag is +0.0
    assert got[3][2] == np.float32(tiny) + np.float32(-3 * tiny) and got[3][2] != 0   # a subnormal sum is kept


def test_offsets_are_validated_on_the_host(native, make_model):
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    rows = np.arange(10, dtype=np.uint32)
    for bad in ([0, 5, 3, 10], [0, 11], [-1, 4], [0.0, 4.0], [], [[0, 4]], ['a', 'b'], [0, 2 ** 40]):
        with pytest.raises(ValueError):
            reader.bags_embedding(rows, bad)
    with pytest.raises(ValueError):
        reader.bags_embedding(rows, [0, 10], mode='max')
    assert reader.bags_embedding(rows, [0, 10]).shape == (1, 300)
    assert reader.bags_embedding(rows, np.array([2, 2, 7], dtype=np.uint64)).shape == (2, 300)


def test_device_methods_refuse_a_host_reader_and_a_union(native, make_model):
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path, device='cpu')
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.sentences_embedding_device([['a', 'b'], ['c']])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.bags_embedding_device(None, None)
    union = native.ReadersUnion([reader, native.Reader(path, device='cpu')], 'average')
    for method in (union.bags_embedding_device, union.bags_embedding, union.sentences_embedding_device):
        with pytest.raises(NotImplementedError, match='ReadersUnion'):
            method(np.arange(3, dtype=np.uint32), [0, 3])
