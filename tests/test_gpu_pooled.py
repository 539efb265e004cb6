"""Pooled lookups on the GPU (memb_hip_pooled.hip: pool_trained, pool_uniform, pool_full; hip_pooled_launch.h: launchPooled).

The oracle everywhere: the reader's own fp32 rows from rows_embedding_device -- which test_gpu_parity.py pins bit for bit
to the CPU checker -- copied to the host and pooled by the explicit float32 loop of the contract
(include/memb_hip_pooled.h): acc = v_begin, acc = acc + v_i in entry order, one division for the mean, +0.0 for an empty
bag. Compared with bits_equal: the tolerance is zero."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import for_every_key_form, into_a_frame, run_on_two_streams, sweep_options, to_device
from pooled_reference import ids_with_misses, offsets_of, pooled_by_the_contract

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)
STORAGES = [('trained', 2), ('trained', 4), ('trained', 6), ('trained', 8), ('uniform', 8), ('full', 8)]
N_ROWS = 20000


def check_pooled(reader, rows, offsets, context, modes=('sum', 'mean'), col_off=0, spare=0):
    """Both modes against the contract over the reader's own rows; the columns around the bags keep their sentinel.
    Returns the 'sum' result."""
    dim = reader.dim
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    values = reader.rows_embedding_device(device_rows).cpu().numpy() if len(rows) else np.zeros((0, dim), dtype=np.float32)
    bags = len(offsets) - 1
    results = {}
    for mode in modes:
        got = into_a_frame(lambda out: reader.bags_embedding_device(device_rows, device_offsets, mode=mode, out=out, col_off=col_off),
                           bags, dim, context, col_off, spare, sentinel=SENTINEL).numpy()
        want = pooled_by_the_contract(values, offsets, mode)
        if not bits_equal(got, want):
            bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            raise AssertionError('{} {}: {} of {} bags differ, first {}'.format(context, mode, len(bad), bags, bad[:8]))
        results[mode] = got
    return results[modes[0]]


# ---- 1. bag shapes, per storage ----

@pytest.mark.parametrize('storage,bits', STORAGES)
def test_bag_shapes(native, make_model, storage, bits):
    import torch
    path, _ = make_model(N_ROWS, 300, storage, bits, distribution='student' if bits == 8 else 'normal')
    reader = native.Reader(path)
    rng = np.random.default_rng(bits)
    # all bags of one entry: the rows themselves, bit for bit
    rows = ids_with_misses(3001, N_ROWS, 1)
    ones = check_pooled(reader, rows, np.arange(len(rows) + 1), (storage, bits, 'ones'))
    assert bits_equal(ones, reader.rows_embedding_device(to_device(rows)).cpu().numpy())
    # empty bags at the start, in the middle and at the end
    lengths = [0, 0, 0, 5, 1, 0, 12, 0, 0, 3, 64, 0, 9, 0, 0]
    check_pooled(reader, ids_with_misses(sum(lengths), N_ROWS, 2), offsets_of(lengths), (storage, bits, 'empties'))
    # fixed lengths that straddle the 8-word tile
    for length in (7, 8, 9, 17):
        check_pooled(reader, ids_with_misses(length * 1500, N_ROWS, length), np.arange(0, length * 1500 + 1, length),
                     (storage, bits, 'fixed', length))
    # seeded geometric lengths
    for mean_length in (3, 16, 60):
        lengths = rng.geometric(1.0 / mean_length, size=2000) - (rng.random(2000) < 0.05)
        check_pooled(reader, ids_with_misses(int(lengths.sum()), N_ROWS, mean_length), offsets_of(lengths),
                     (storage, bits, 'geometric', mean_length))
    # one bag of 100 000 entries, alone and between small ones
    check_pooled(reader, ids_with_misses(100000, N_ROWS, 5), [0, 100000], (storage, bits, 'one long bag'))
    check_pooled(reader, ids_with_misses(100020, N_ROWS, 6), offsets_of([3, 0, 7, 100000, 1, 9]), (storage, bits, 'long bag among small'))
    # every entry a missing row
    check_pooled(reader, np.array([0xFFFFFFFF, N_ROWS, N_ROWS + 1, 0xFFFFFFFF, 0xFFFFFFFE], dtype=np.uint32), [0, 2, 5],
                 (storage, bits, 'all missing'))
    # bags = 0: nothing is launched, an empty result
    empty = reader.bags_embedding_device(to_device(rows), to_device([len(rows)]))
    assert tuple(empty.shape) == (0, 300)
    # n = 0: zeros for every bag
    zero = check_pooled(reader, np.zeros(0, dtype=np.uint32), [0, 0, 0, 0], (storage, bits, 'n = 0'))
    assert zero.shape == (3, 300) and not zero.any() and not np.signbit(zero).any()
    torch.cuda.synchronize()


# ---- 2. geometries ----

@pytest.mark.parametrize('dim', [300, 64, 512, 516, 302, 6, 7, 257, 1, 2, 3])
@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_dims_and_strided_outputs(native, make_model, storage, bits, dim):
    # dims that are a multiple of 4 (16-byte pieces: one and two per lane, and past the register form), = 2 mod 4, odd and
    # below 4; dense, and ld > dim with col_off > 0 (aligned to a piece and not) between guard columns
    path, _ = make_model(700, dim, storage, bits, seed=dim)
    reader = native.Reader(path)
    lengths = np.random.default_rng(dim).geometric(1 / 9.0, size=300)
    rows = ids_with_misses(int(lengths.sum()), 700, dim)
    for col_off, spare in ((0, 0), (4, 4), (2, 1), (1, 2)):
        check_pooled(reader, rows, offsets_of(lengths), (storage, bits, dim, col_off, spare), col_off=col_off, spare=spare)


@pytest.mark.parametrize('dim,bits,count', [(4096, 8, 120), (9000, 8, 40), (20000, 4, 30)])
def test_very_wide_trained_rows(native, make_model, dim, bits, count):
    # beyond the row-record limits: compact streams, up to one word per wavefront, the column form
    path, _ = make_model(count, dim, 'trained', bits, seed=dim)
    reader = native.Reader(path)
    assert reader.info()['row_layout'] != 2
    lengths = [1, 0, 3, 9, 2, 17, 1]
    check_pooled(reader, ids_with_misses(sum(lengths), count, dim), offsets_of(lengths), ('wide', dim, bits))
    check_pooled(reader, ids_with_misses(sum(lengths), count, dim), offsets_of(lengths), ('wide', dim, bits, 'col_off'), col_off=2, spare=3)


@pytest.mark.parametrize('storage', ['uniform', 'full'])
def test_very_wide_rowwise_rows(native, make_model, storage):
    path, _ = make_model(40, 5001, storage, 8, seed=5001)
    lengths = [1, 0, 3, 9, 2, 17, 1]
    check_pooled(native.Reader(path), ids_with_misses(sum(lengths), 40, 5), offsets_of(lengths), (storage, 5001), col_off=1, spare=2)


def test_key_forms_tables_and_row_layouts(native, make_model, monkeypatch):
    """Nibble keys, byte keys with a one-level table (MEMB_HIP_NO_FAST), two-level tables through
    max_direct_decode_bits=1; row records, compact streams with rowMeta records and with the two index arrays; lanes per
    word from 1 to 64 with spare lanes, blocks of 1 to 8 wavefronts."""
    lengths = np.random.default_rng(1).geometric(1 / 12.0, size=600)
    rows = ids_with_misses(int(lengths.sum()), N_ROWS, 9)
    offsets = offsets_of(lengths)

    def check(reader, context):
        check_pooled(reader, rows, offsets, context)
        check_pooled(reader, rows, offsets, context + ('col_off 1',), modes=('mean',), col_off=1, spare=1)

    for_every_key_form(native, make_model, monkeypatch, N_ROWS, check)


# ---- 3. the mean is the sum and one division ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_mean_is_the_sum_divided_once(native, make_model, storage, bits):
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path)
    lengths = np.array([3, 5, 6, 7, 9, 10, 11, 13, 100, 1000, 3, 7] * 20)
    rows = ids_with_misses(int(lengths.sum()), N_ROWS, 4)
    device_rows, device_offsets = to_device(rows), to_device(offsets_of(lengths))
    total = reader.bags_embedding_device(device_rows, device_offsets, mode='sum').cpu().numpy()
    mean = reader.bags_embedding_device(device_rows, device_offsets).cpu().numpy()   # (the default mode)
    assert bits_equal(mean, np.divide(total, lengths.astype(np.float32)[:, None], dtype=np.float32))
    assert not bits_equal(mean, total * (np.float32(1) / lengths.astype(np.float32))[:, None])   # (a reciprocal multiply is not it)


# ---- 4. subnormal sums of mixed signs: the packed-add trap ----

def test_subnormal_sums_with_mixed_signs(native, tmp_path):
    rng = np.random.default_rng(40)
    count, dim = 500, 300
    # values of both signs between 1e-45 and 1e-40, exact zeros of both signs among them: every partial sum is subnormal
    vectors = (rng.integers(-70000, 70000, size=(count, dim)).astype(np.int64)).astype(np.float32) * np.float32(1.4e-45)
    vectors[rng.random((count, dim)) < 0.05] = -0.0
    assert (np.abs(vectors) < 1.1754944e-38).all() and (vectors != 0).any()
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['s{:04d}'.format(i) for i in range(count)], vectors)
    path = str(tmp_path / 'subnormal.bin')
    builder.save(path)
    reader = native.Reader(path)
    lengths = np.concatenate([[1, 1, 2, 2, 3], rng.geometric(1 / 10.0, size=400)])
    rows = rng.integers(0, count, size=int(lengths.sum())).astype(np.uint32)
    total = check_pooled(reader, rows, offsets_of(lengths), 'subnormal sums')
    assert (total != 0).any() and (np.abs(total[total != 0]) < 1.1754944e-38).all()
    # -0.0 survives a bag of one entry
    assert np.signbit(total[:2]).any()
    for dim_small in (2, 8):   # the same through other column forms
        small = native.Builder(dim_small, 'full', 8)
        small.add_words(['s{:04d}'.format(i) for i in range(count)], vectors[:, :dim_small])
        small_path = str(tmp_path / 'subnormal_{}.bin'.format(dim_small))
        small.save(small_path)
        check_pooled(native.Reader(small_path), rows, offsets_of(lengths), ('subnormal sums', dim_small))


# ---- 5. offsets a host would have refused, in a device tensor: the defined result ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_offsets_beyond_n_and_backwards_give_the_defined_result(native, make_model, storage, bits):
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path)
    n = 1000
    rows = ids_with_misses(n, N_ROWS, 8)
    offsets = np.array([0, 10, 25, 20, 20, 40, 5000, 60, 90, 0xFFFFFFFF, 100, 130, 990, 1000, 1001, 1000], dtype=np.int64)
    pooled = check_pooled(reader, rows, offsets, (storage, bits, 'bad offsets'))
    values = reader.rows_embedding_device(to_device(rows)).cpu().numpy()
    clamped = np.minimum(offsets, n)
    for bag in range(len(offsets) - 1):
        begin, end = clamped[bag], clamped[bag + 1]
        if end <= begin:
            assert not pooled[bag].any(), bag                  # backwards or empty: +0.0
    # the neighbours of the damaged bags are what they are with honest offsets
    honest = check_pooled(reader, rows, [0, 10, 25, 40, 100, 130, 990, 1000], (storage, bits, 'honest'))
    assert bits_equal(pooled[0], honest[0]) and bits_equal(pooled[1], honest[1])
    assert bits_equal(pooled[10], honest[4]) and bits_equal(pooled[11], honest[5]) and bits_equal(pooled[12], honest[6])
    assert bits_equal(pooled[5], pooled_by_the_contract(values, [40, 1000], 'sum')[0])   # 40 .. 5000 is 40 .. n


# ---- 6. launch geometry never changes a result ----

@pytest.mark.parametrize('bits', [4, 6])
def test_results_do_not_depend_on_options(native, make_model, bits):
    path, _ = make_model(N_ROWS, 300, 'trained', bits)
    reader = native.Reader(path)
    lengths = np.random.default_rng(bits).geometric(1 / 16.0, size=3000)
    device_rows, device_offsets = to_device(ids_with_misses(int(lengths.sum()), N_ROWS, 3)), to_device(offsets_of(lengths))
    reference = {mode: reader.bags_embedding_device(device_rows, device_offsets, mode=mode).cpu().numpy() for mode in ('sum', 'mean')}

    def run(waves, tiles):
        for mode in ('sum', 'mean'):
            got = reader.bags_embedding_device(device_rows, device_offsets, mode=mode).cpu().numpy()
            assert bits_equal(got, reference[mode]), (waves, tiles, mode)

    sweep_options(reader, run)


def test_two_threads_on_two_streams(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    jobs = []
    for thread in range(2):
        lengths = np.random.default_rng(thread).geometric(1 / 16.0, size=4000)
        rows = ids_with_misses(int(lengths.sum()), N_ROWS, thread)
        offsets = offsets_of(lengths)
        values = reader.rows_embedding_device(to_device(rows)).cpu().numpy()
        jobs.append((to_device(rows), to_device(offsets), {mode: pooled_by_the_contract(values, offsets, mode) for mode in ('sum', 'mean')}))

    def call(thread, repeat):
        mode = ('sum', 'mean')[repeat % 2]
        got = reader.bags_embedding_device(jobs[thread][0], jobs[thread][1], mode=mode)
        return (got,), (jobs[thread][2][mode],), mode

    run_on_two_streams(jobs, call)


# ---- 7. the Python surface ----

def test_python_entry_points_and_their_errors(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    vocabulary = sorted(words)
    sentences = [vocabulary[:5], [], ['not-in-the-model'], vocabulary[100:117] + ['nor-this'], [vocabulary[7]]]
    flat = [word for sentence in sentences for word in sentence]
    rows = reader.resolve_rows(flat)
    offsets = offsets_of([len(sentence) for sentence in sentences])
    values = reader.rows_embedding(rows)
    for mode in ('sum', 'mean'):
        want = pooled_by_the_contract(values, offsets, mode)
        assert bits_equal(reader.sentences_embedding_device(sentences, mode=mode).cpu().numpy(), want)
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode), want)   # host arrays through the GPU
        assert bits_equal(native.Reader(path, device='cpu').bags_embedding(rows, offsets, mode=mode), want)
    assert tuple(reader.sentences_embedding_device([]).shape) == (0, 300)
    assert not reader.sentences_embedding_device([[], []]).any()
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    with pytest.raises(ValueError):
        reader.bags_embedding_device(device_rows, device_offsets, mode='max')
    with pytest.raises(TypeError, match='float32'):
        reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((5, 300), dtype=torch.bfloat16, device='cuda'))
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows.cpu(), device_offsets)
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows, device_offsets.cpu())
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows, device_offsets.to(torch.int64))
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((4, 300), device='cuda'))
    with pytest.raises(ValueError):
        reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((5, 300), device='cuda'), col_off=4)
    with pytest.raises(ValueError):
        reader.bags_embedding_device(device_rows, device_offsets[:0])
    with pytest.raises(ValueError):
        reader.bags_embedding(rows, [0, 3, 2, len(rows)])


# ---- 8. the headline model at full size ----

def test_headline_model_in_bags_of_sixteen(native):
    import torch
    from memb_amd import synthetic
    count = 2196017
    path, _ = synthetic.cached_model(count, 300, 'trained', 4)   # shared with bench.py and test_gpu_full_size.py on the same box
    reader = native.Reader(path)
    offsets = np.append(np.arange(0, count, 16), count)
    device_offsets = to_device(offsets)
    generator = torch.Generator(device='cuda').manual_seed(5)
    shuffled = torch.randperm(count, device='cuda', generator=generator).to(torch.int32)
    shuffled[::1000] = -1   # 0xFFFFFFFF
    for order, device_rows in (('key order', torch.arange(count, dtype=torch.int32, device='cuda')), ('shuffled', shuffled)):
        pooled = {mode: reader.bags_embedding_device(device_rows, device_offsets, mode=mode).cpu().numpy() for mode in ('sum', 'mean')}
        rows = reader.rows_embedding_device(device_rows)
        torch.cuda.synchronize()
        step = 16 * 12500   # bags of a slice: whole bags
        for start in range(0, count, step):
            stop = min(count, start + step)
            values = rows[start:stop].cpu().numpy()
            local = np.append(np.arange(0, stop - start, 16), stop - start)
            for mode in ('sum', 'mean'):
                want = pooled_by_the_contract(values, local, mode)
                assert bits_equal(pooled[mode][start // 16:start // 16 + len(want)], want), (order, mode, start)
        del rows


def test_pooled_algorithmic_bytes(native, make_model):
    # per entry the id and, for a row of the model, its metadata and bytes; per bag two offsets and the stored row
    rows = np.array([0, 5, 0xFFFFFFFF, 9, 700, 3, 3, 8], dtype=np.uint32)
    offsets = np.array([0, 2, 2, 7, 9], dtype=np.uint32)   # the last bag ends at n: entries 7 .. 8
    present_in_bags = 6   # entries 0 .. 7 are all in bags; two of them are missing rows
    for storage, per_row in (('uniform', 12 + 300), ('full', 4 + 4 * 300)):
        path, _ = make_model(700, 300, storage, 8)
        reader = native.Reader(path)
        reader.info()   # (stages the model)
        want = 8 * 4 + present_in_bags * per_row + 4 * (8 + 4 * 300)
        assert reader._impl.pooled_algorithmic_bytes(rows, offsets) == want, storage
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    one = reader._impl.pooled_algorithmic_bytes(rows[:1], np.array([0, 1], dtype=np.uint32))
    assert 4 + 4 + 8 + 1200 < one < 4 + 4 + 8 + 1200 + 300   # a 4-bit stream of 300 symbols is below 300 bytes
