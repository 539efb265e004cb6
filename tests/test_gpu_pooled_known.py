"""Pooled lookups over the rows a model knows, on the GPU (memb_hip_pooled_known.hip; include/memb_hip_pooled_known.h):
bags_embedding_device / sentences_embedding_device / bags_embedding with missing='skip'.

Two references, both compared with bits_equal (the tolerance is zero):
  R1  the contract's explicit float32 loop over reader.rows_embedding(rows): per bag the KNOWN entries (row id < n_rows) in
      entry order, acc = v_K[0], acc = acc + v_K[j], one division by |K| for the mean, +0.0 where K is empty;
  R2  what the EXISTING pooled call (missing='zero', the kernels of memb_hip_pooled.hip / memb_hip_pooled_narrow.hip) returns
      for the compacted batch: unknown entries taken out, offsets recomputed on the host.
A bf16 / fp16 result is R1 .to(dtype) on the CPU, and R2 with that dtype."""
import itertools

import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import (WAVES_PER_BLOCK, for_every_key_form, into_a_frame, narrow_bits, run_on_two_streams, sweep_options,
                           to_device)
from pooled_reference import UNKNOWN, compacted, ids_with_unknowns, offsets_of, sequential_by_the_contract

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
N_ROWS = 20000


def check_known(reader, rows, offsets, context, modes=('sum', 'mean'), col_off=0, spare=0, dtype=None):
    """Both modes against R1 and R2, with the counts; the columns around the bags keep their sentinel. Returns the fp32
    'sum' vectors (of `dtype` as float32 where one is given) and the counts."""
    import torch
    dim = reader.dim
    n_rows = len(reader)
    rows = np.asarray(rows, dtype=np.uint32)
    kind = dtype or torch.float32
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    values = reader.rows_embedding(rows) if len(rows) else np.zeros((0, dim), dtype=np.float32)
    dense_rows, dense_offsets, _ = compacted(rows, offsets, n_rows)
    bags = len(offsets) - 1
    results = {}
    for mode in modes:
        counted = []

        def run(out):
            returned, counts = reader.bags_embedding_device(
                device_rows, device_offsets, mode=mode, out=out, col_off=col_off, dtype=dtype, missing='skip', return_counts=True)
            counted.append(counts)
            return returned

        got = into_a_frame(run, bags, dim, context, col_off, spare, dtype, sentinel=SENTINEL)
        counts = counted[0]
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (bags,) and counts.is_cuda
        want, want_counts = sequential_by_the_contract(values, rows, offsets, n_rows, mode, True)
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts), (context, mode, 'counts')
        first = torch.from_numpy(want).to(kind)                                                    # R1
        second = reader.bags_embedding_device(to_device(dense_rows), to_device(dense_offsets), mode=mode, dtype=dtype).cpu()   # R2
        for name, reference in (('R1', first), ('R2', second)):
            if not np.array_equal(narrow_bits(got), narrow_bits(reference)):
                bad = np.nonzero((narrow_bits(got) != narrow_bits(reference)).any(axis=1))[0]
                raise AssertionError('{} {} {}: {} of {} bags differ, first {}'.format(context, mode, name, len(bad), bags, bad[:8]))
        results[mode] = got.to(torch.float32).numpy()
    return results[modes[0]], want_counts


def shaped_bags(n_rows, seed):
    """Bags where the accumulation can go wrong, as (rows, offsets). k: some known id."""
    rng = np.random.default_rng(seed)
    k = lambda: int(rng.integers(0, n_rows))   # noqa: E731
    U = UNKNOWN
    bags = [
        [], [k()], [U], [U, U, U], [],
        [U, k(), k()], [k(), k(), U], [k(), U, k(), U, k(), U, k()], [U, k(), U, k(), U],
        [n_rows, k(), n_rows + 5, k(), 0xFFFFFFFE, n_rows + 1000],       # ids >= n_rows other than 0xFFFFFFFF
        [k(), k(), k()], [U] * 5, [k(), k()],                            # an all-unknown bag between two bags
        [k(), k(), k(), k(), k()], [n_rows] * 19, [k()],                 # ... and one that is longer than two tiles
        [U] * 17 + [k()], [k()] + [U] * 17, [U] * 40,
    ]
    for mean_length in (3, 16):
        for length in rng.geometric(1.0 / mean_length, size=150):
            bags.append(list(ids_with_unknowns(int(length), n_rows, int(rng.integers(1 << 30)), share=0.3)))
    bags.append(list(ids_with_unknowns(200, n_rows, seed + 1, share=0.5)))
    rows = np.array([row for bag in bags for row in bag], dtype=np.uint32)
    return rows, offsets_of([len(bag) for bag in bags])


def tile_cases(tile, n_rows, seed):
    """Bags that START on a tile of `tile` words (bag 0 of their call), as (name, rows, offsets): an unknown entry on each
    side of a tile boundary, a bag of three tiles whose middle one is all unknown, and bags whose first known entry lies in
    the second / third tile -- what pins the parked partial sums of the fp32 column form."""
    rng = np.random.default_rng(seed)
    known = lambda count: rng.integers(0, n_rows, size=count).astype(np.uint32)   # noqa: E731
    cases = []
    rows = known(2 * tile + 4)
    rows[tile - 1] = UNKNOWN
    cases.append(('last of the first tile', rows.copy(), [0, len(rows)]))
    rows[tile - 1] = 3
    rows[tile] = n_rows
    cases.append(('first of the second tile', rows.copy(), [0, len(rows)]))
    rows[tile - 1] = UNKNOWN
    cases.append(('both sides of the boundary', rows.copy(), [0, len(rows)]))
    rows = known(3 * tile)
    rows[tile:2 * tile] = UNKNOWN
    cases.append(('middle tile unknown', rows.copy(), [0, len(rows)]))
    rows[2 * tile:] = UNKNOWN
    cases.append(('known tile first only', rows.copy(), [0, len(rows)]))
    rows = known(2 * tile + 3)
    rows[:tile + 2] = UNKNOWN
    cases.append(('first known in the second tile', rows.copy(), [0, len(rows)]))
    rows = known(3 * tile + 1)
    rows[:2 * tile] = UNKNOWN
    rows[-1] = UNKNOWN
    cases.append(('first known in the third tile', rows.copy(), [0, len(rows)]))
    rows = known(3 * tile + 5)
    rows[:tile] = UNKNOWN
    cases.append(('bags after a tile of unknowns', rows.copy(), [0, tile - 1, tile + 1, 2 * tile, 2 * tile, len(rows)]))
    return cases


def tile_words(reader, n):
    info = reader.info(max(int(n), 1))
    return 64 // int(info['lanes_per_word']) if info.get('lanes_per_word') else 8


# ---- 1. storages, key forms and bag shapes ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('trained', 8), ('uniform', 8), ('full', 8)])
def test_storages_and_bag_shapes(native, make_model, storage, bits):
    import torch
    path, _ = make_model(N_ROWS, 300, storage, bits, distribution='student' if bits == 8 and storage == 'trained' else 'normal')
    reader = native.Reader(path)
    rows, offsets = shaped_bags(N_ROWS, bits)
    vectors, counts = check_known(reader, rows, offsets, (storage, bits, 'shapes'))
    assert not vectors[0].any() and counts[0] == 0          # an empty bag
    assert counts[1] == 1 and bits_equal(vectors[1], reader.rows_embedding(rows[:1])[0])   # one known entry: its bits
    assert not vectors[2].any() and not np.signbit(vectors[2]).any() and counts[2] == 0    # one unknown entry: +0.0
    for dtype in (torch.bfloat16, torch.float16):
        check_known(reader, rows, offsets, (storage, bits, 'shapes', dtype), dtype=dtype)
    for tile in sorted({8, tile_words(reader, 20)} if storage == 'trained' else {8}):
        for name, case_rows, case_offsets in tile_cases(tile, N_ROWS, tile):
            check_known(reader, case_rows, case_offsets, (storage, bits, tile, name))
            check_known(reader, case_rows, case_offsets, (storage, bits, tile, name, 'column form'), col_off=1, spare=2)
            check_known(reader, case_rows, case_offsets, (storage, bits, tile, name, 'bf16'), modes=('mean',), dtype=torch.bfloat16)
    # every entry unknown; bags = 0; n = 0
    check_known(reader, [UNKNOWN, N_ROWS, N_ROWS + 1, UNKNOWN, 0xFFFFFFFE], [0, 2, 5], (storage, bits, 'all unknown'))
    empty, no_counts = reader.bags_embedding_device(to_device(rows), to_device([len(rows)]), missing='skip', return_counts=True)
    assert tuple(empty.shape) == (0, 300) and tuple(no_counts.shape) == (0,)
    zero, counts = check_known(reader, np.zeros(0, dtype=np.uint32), [0, 0, 0, 0], (storage, bits, 'n = 0'))
    assert zero.shape == (3, 300) and not zero.any() and not np.signbit(zero).any() and not counts.any()


@pytest.mark.parametrize('dim', [300, 299, 1, 512, 516, 1030])
@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_dims_and_strided_outputs(native, make_model, storage, bits, dim):
    # 300: the piece form; 299 and 1: the column form; 512 / 516: the second accumulator's edge and the first dim past the
    # piece form; 1030: the narrow column form in three blocks. Dense, aligned to a piece, and ld / col_off that break the
    # 16-byte (fp32) and 8-byte (bf16 / fp16) alignment, between guard columns.
    import torch
    path, _ = make_model(3000, dim, storage, bits, seed=dim)
    reader = native.Reader(path)
    lengths = np.random.default_rng(dim).geometric(1 / 9.0, size=120)
    lengths[:6] = [0, 1, 30, 2, 70, 0]
    rows = ids_with_unknowns(int(lengths.sum()), 3000, dim)
    rows[:31] = UNKNOWN   # bags 1 and 2: nothing known
    for dtype in (None, torch.bfloat16, torch.float16):
        for col_off, spare in ((0, 0), (4, 4), (1, 2)):
            check_known(reader, rows, offsets_of(lengths), (storage, bits, dim, col_off, spare, dtype), col_off=col_off, spare=spare,
                        dtype=dtype)


def test_key_forms_tables_and_row_layouts(native, make_model, monkeypatch):
    """Nibble keys, byte keys with a one-level table (MEMB_HIP_NO_FAST) and with two-level tables (max_direct_decode_bits=1);
    row records, compact streams with rowMeta records and with the two index arrays; 1 to 64 lanes per word."""
    import torch
    rows, offsets = shaped_bags(N_ROWS, 9)

    def check(reader, context):
        check_known(reader, rows, offsets, context)
        check_known(reader, rows, offsets, context + ('col_off 1',), modes=('mean',), col_off=1, spare=1)
        check_known(reader, rows, offsets, context + ('fp16',), modes=('mean',), col_off=1, dtype=torch.float16)

    for_every_key_form(native, make_model, monkeypatch, N_ROWS, check)


# ---- 2. offsets a host would have refused: the defined, clamped result ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_offsets_beyond_n_and_backwards_give_the_defined_result(native, make_model, storage, bits):
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path)
    n = 1000
    rows = ids_with_unknowns(n, N_ROWS, 8)
    offsets = np.array([0, 10, 25, 20, 20, 40, 5000, 60, 90, 0xFFFFFFFF, 100, 130, 990, 1000, 1001, 1000], dtype=np.int64)
    pooled, counts = check_known(reader, rows, offsets, (storage, bits, 'bad offsets'))
    clamped = np.minimum(offsets, n)
    for bag in range(len(offsets) - 1):
        if clamped[bag + 1] <= clamped[bag]:
            assert not pooled[bag].any() and counts[bag] == 0, bag   # backwards or empty: +0.0, nothing known
    assert counts[5] == int((rows[40:] < N_ROWS).sum())              # 40 .. 5000 is 40 .. n


# ---- 3. signed zeros and subnormals ----

def test_signed_zeros_and_subnormal_sums(native, tmp_path):
    import torch
    rng = np.random.default_rng(41)
    count, dim = 500, 300
    vectors = (rng.integers(-70000, 70000, size=(count, dim)).astype(np.int64)).astype(np.float32) * np.float32(1.4e-45)
    vectors[rng.random((count, dim)) < 0.05] = -0.0
    vectors[0] = -0.0   # a row of -0.0
    assert (np.abs(vectors) < 1.1754944e-38).all() and (vectors != 0).any()
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['s{:04d}'.format(i) for i in range(count)], vectors)
    path = str(tmp_path / 'subnormal.bin')
    builder.save(path)
    reader = native.Reader(path)
    lengths = np.concatenate([[2, 2, 3, 1], rng.geometric(1 / 10.0, size=300)])
    rows = ids_with_unknowns(int(lengths.sum()), count, 42)
    rows[:8] = [UNKNOWN, 0, 0, count, UNKNOWN, 0, UNKNOWN, UNKNOWN]   # [missing, -0.0] [-0.0, missing] [missing, -0.0, missing] [missing]
    total, counts = check_known(reader, rows, offsets_of(lengths), 'subnormal sums')
    assert (total != 0).any() and (np.abs(total[total != 0]) < 1.1754944e-38).all()   # subnormal partial sums are kept
    for bag in range(3):
        assert counts[bag] == 1 and np.signbit(total[bag]).all() and not total[bag].any(), bag   # -0.0: nothing was added to it
    assert counts[3] == 0 and not np.signbit(total[3]).any()
    device_rows, device_offsets = to_device(rows), to_device(offsets_of(lengths))
    for mode in ('sum', 'mean'):
        skipped = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip').cpu().numpy()
        counted = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='zero').cpu().numpy()
        assert np.signbit(skipped[:3]).all() and not np.signbit(counted[:3]).any()   # +0.0 + -0.0 = +0.0 where missing rows count
    for dtype in (torch.bfloat16, torch.float16):
        check_known(reader, rows, offsets_of(lengths), ('subnormal sums', dtype), dtype=dtype)
    for dim_small in (2, 8):   # the same through other column forms
        small = native.Builder(dim_small, 'full', 8)
        small.add_words(['s{:04d}'.format(i) for i in range(count)], vectors[:, :dim_small])
        small_path = str(tmp_path / 'subnormal_{}.bin'.format(dim_small))
        small.save(small_path)
        check_known(native.Reader(small_path), rows, offsets_of(lengths), ('subnormal sums', dim_small))


# ---- 4. bf16 / fp16: the fp32 result rounded once ----

@pytest.mark.parametrize('dim', [300, 299, 1030])
def test_narrow_results_are_the_fp32_result_rounded_once(native, tmp_path, dim):
    import torch
    values = np.array([1.0, 2.0 ** -8, 60000.0, -60000.0, 3.0], dtype=np.float32)
    vectors = np.repeat(values[:, None], dim, axis=1)
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['w{}'.format(i) for i in range(len(values))], vectors)
    path = str(tmp_path / 'narrow_{}.bin'.format(dim))
    builder.save(path)
    reader = native.Reader(path)
    one, tiny, big, negative = (int(reader.resolve_rows(['w{}'.format(i)])[0]) for i in range(4))
    assert len(reader) == 5   # (so 9 is an id that is not in the model)
    bags = [[one, UNKNOWN, tiny, tiny], [big, UNKNOWN, big], [negative, negative, 9], [UNKNOWN, tiny, UNKNOWN, one, tiny, UNKNOWN]]
    rows = np.array([row for bag in bags for row in bag], dtype=np.uint32)
    offsets = offsets_of([len(bag) for bag in bags])
    fp32, _ = check_known(reader, rows, offsets, ('narrow', dim, 'fp32'))
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    for dtype in (torch.bfloat16, torch.float16):
        check_known(reader, rows, offsets, ('narrow', dim, dtype), dtype=dtype)
        got = reader.bags_embedding_device(device_rows, device_offsets, mode='sum', dtype=dtype, missing='skip').cpu()
        assert np.array_equal(narrow_bits(got), narrow_bits(torch.from_numpy(fp32).to(dtype)))
        if dtype == torch.bfloat16:
            # 1 + 2^-8 is a tie that rounds to 1 in bf16: a partial sum narrowed on the way would end at 1, not 1 + 2^-7
            assert (got[0].to(torch.float32) == 1.0 + 2.0 ** -7).all()
            assert (got[3].to(torch.float32) == 1.0 + 2.0 ** -7).all()
        else:
            assert torch.isinf(got[1]).all() and (got[1] > 0).all() and torch.isinf(got[2]).all() and (got[2] < 0).all()
            mean = reader.bags_embedding_device(device_rows, device_offsets, mode='mean', dtype=dtype, missing='skip').cpu()
            assert (mean[1].to(torch.float32) == 60000.0).all()   # 120 000 / 2: the division came before the narrowing


# ---- 5. missing='zero' is the call without the keyword ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_missing_zero_is_the_existing_call(native, make_model, storage, bits):
    import torch
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path)
    rows, offsets = shaped_bags(N_ROWS, 5)
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    for mode in ('sum', 'mean'):
        for dtype in (None, torch.bfloat16):
            plain = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, dtype=dtype).cpu()
            named = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, dtype=dtype, missing='zero',
                                                 return_counts=False).cpu()
            assert np.array_equal(narrow_bits(plain), narrow_bits(named))
    skipped = reader.bags_embedding_device(device_rows, device_offsets, missing='skip').cpu().numpy()
    assert not bits_equal(skipped, reader.bags_embedding_device(device_rows, device_offsets).cpu().numpy())   # (another mean)


# ---- 6. launch geometry never changes a result ----

@pytest.mark.parametrize('bits', [4, 6])
def test_results_do_not_depend_on_options(native, make_model, bits):
    path, _ = make_model(N_ROWS, 300, 'trained', bits)
    reader = native.Reader(path)
    lengths = np.random.default_rng(bits).geometric(1 / 16.0, size=3000)
    device_rows, device_offsets = to_device(ids_with_unknowns(int(lengths.sum()), N_ROWS, 3)), to_device(offsets_of(lengths))

    def both(mode):
        # the piece form; the fp32 column form, whose parked partial sums move with the tiles (col_off 1 breaks the alignment);
        # the narrow piece form, and the narrow column form
        import torch
        vectors, counts = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip', return_counts=True)
        bags = counts.numel()
        parked = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip', col_off=1,
                                              out=torch.zeros((bags, 302), device='cuda'))
        narrow = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip', dtype=torch.bfloat16)
        narrow_columns = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip', dtype=torch.bfloat16,
                                                      col_off=1, out=torch.zeros((bags, 302), dtype=torch.bfloat16, device='cuda'))
        assert torch.equal(parked[:, 1:301].view(torch.int32), vectors.view(torch.int32)), mode
        assert torch.equal(narrow_columns[:, 1:301].view(torch.int16), narrow.view(torch.int16)), mode
        return np.concatenate([vectors.cpu().numpy(), narrow.to(torch.float32).cpu().numpy()]), counts.cpu().numpy()

    reference = {mode: both(mode) for mode in ('sum', 'mean')}

    def run(waves, tiles):
        for mode in ('sum', 'mean'):
            vectors, counts = both(mode)
            assert bits_equal(vectors, reference[mode][0]) and np.array_equal(counts, reference[mode][1]), (waves, tiles, mode)

    sweep_options(reader, run, itertools.product(WAVES_PER_BLOCK, (1, 2, 5, 8, 64)))


def test_two_threads_on_two_streams(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    jobs = []
    for thread in range(2):
        lengths = np.random.default_rng(thread).geometric(1 / 16.0, size=4000)
        rows = ids_with_unknowns(int(lengths.sum()), N_ROWS, thread)
        offsets = offsets_of(lengths)
        values = reader.rows_embedding(rows)
        jobs.append((to_device(rows), to_device(offsets),
                     {mode: sequential_by_the_contract(values, rows, offsets, N_ROWS, mode, True) for mode in ('sum', 'mean')}))

    def call(thread, repeat):
        mode = ('sum', 'mean')[repeat % 2]
        got = reader.bags_embedding_device(jobs[thread][0], jobs[thread][1], mode=mode, missing='skip', return_counts=True)
        return got, jobs[thread][2][mode], mode

    run_on_two_streams(jobs, call)


# ---- 7. the Python surface ----

def test_python_entry_points_and_their_errors(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    vocabulary = sorted(words)
    sentences = [vocabulary[:5], [], ['not-in-the-model'], ['nor-this'] + vocabulary[100:117] + ['nor-this'], [vocabulary[7]],
                 ['unknown', vocabulary[3], 'unknown too']]
    flat = [word for sentence in sentences for word in sentence]
    rows = reader.resolve_rows(flat)
    offsets = offsets_of([len(sentence) for sentence in sentences])
    values = reader.rows_embedding(rows)
    host_reader = native.Reader(path, device='cpu')
    for mode in ('sum', 'mean'):
        want, want_counts = sequential_by_the_contract(values, rows, offsets, N_ROWS, mode, True)
        assert list(want_counts) == [5, 0, 0, 17, 1, 1]
        vectors, counts = reader.sentences_embedding_device(sentences, mode=mode, missing='skip', return_counts=True)
        assert bits_equal(vectors.cpu().numpy(), want) and list(counts.cpu().numpy()) == list(want_counts)
        assert counts.dtype == torch.int32 and counts.is_cuda
        assert bits_equal(reader.sentences_embedding_device(sentences, mode=mode, missing='skip').cpu().numpy(), want)
        for source in (reader, host_reader):   # host arrays through the GPU, and the numpy branch
            assert bits_equal(source.bags_embedding(rows, offsets, mode=mode, missing='skip'), want)
            vectors, counts = source.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True)
            assert bits_equal(vectors, want) and counts.dtype == np.uint32 and np.array_equal(counts, want_counts)
    assert bits_equal(want[5], values[int(offsets[5]) + 1])   # the mean of one known word among unknown ones: that word
    assert tuple(reader.sentences_embedding_device([], missing='skip').shape) == (0, 300)
    assert not reader.sentences_embedding_device([[], ['unknown']], missing='skip').any()
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    for call in (lambda **k: reader.bags_embedding_device(device_rows, device_offsets, **k),
                 lambda **k: reader.sentences_embedding_device(sentences, **k),
                 lambda **k: reader.bags_embedding(rows, offsets, **k),
                 lambda **k: host_reader.bags_embedding(rows, offsets, **k)):
        with pytest.raises(ValueError, match='missing'):
            call(missing='ignore')
        with pytest.raises(ValueError, match='return_counts'):
            call(return_counts=True)
        with pytest.raises(ValueError, match='return_counts'):
            call(missing='zero', return_counts=True)
        with pytest.raises(ValueError):
            call(mode='max', missing='skip')
    with pytest.raises(TypeError, match='float32'):
        reader.bags_embedding_device(device_rows, device_offsets, missing='skip',
                                     out=torch.empty((6, 300), dtype=torch.bfloat16, device='cuda'))
    with pytest.raises(ValueError):
        reader.bags_embedding_device(device_rows, device_offsets, missing='skip', out=torch.empty((6, 300), device='cuda'), col_off=4)
    union = native.ReadersUnion([reader, native.Reader(path)], 'average')
    with pytest.raises(NotImplementedError):
        union.bags_embedding_device(device_rows, device_offsets, missing='skip')


# ---- 8. the headline model at full size ----

def test_headline_model_in_bags_of_sixteen_with_every_tenth_id_unknown(native):
    import torch
    from memb_amd import synthetic
    count = 2196017
    path, _ = synthetic.cached_model(count, 300, 'trained', 4)   # shared with bench.py and the other full-size tests on the same box
    reader = native.Reader(path)
    offsets = np.append(np.arange(0, count, 16), count)
    bags = len(offsets) - 1
    device_offsets = to_device(offsets)
    generator = torch.Generator(device='cuda').manual_seed(6)
    device_rows = torch.randperm(count, device='cuda', generator=generator).to(torch.int32)
    device_rows[::10] = -1   # 0xFFFFFFFF
    # R2 on the device: compaction of ids and offsets in torch, then the existing call
    keep = device_rows != -1
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device='cuda'), torch.cumsum(keep, 0)])
    dense_offsets = before[device_offsets.to(torch.int64)].to(torch.int32)
    dense_rows = device_rows[keep].contiguous()
    sample = np.sort(np.random.default_rng(7).choice(bags, size=2000, replace=False))
    host_rows = device_rows.cpu().numpy().view(np.uint32)
    sample_rows = np.concatenate([host_rows[offsets[bag]:offsets[bag + 1]] for bag in sample])
    sample_offsets = offsets_of([offsets[bag + 1] - offsets[bag] for bag in sample])
    values = reader.rows_embedding(sample_rows)
    for mode in ('sum', 'mean'):
        got, counts = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, missing='skip', return_counts=True)
        want = reader.bags_embedding_device(dense_rows, dense_offsets, mode=mode)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), mode                       # R2
        assert torch.equal(counts, dense_offsets[1:] - dense_offsets[:-1])
        first, first_counts = sequential_by_the_contract(values, sample_rows, sample_offsets, count, mode, True)    # R1 on the sample
        assert bits_equal(got[torch.from_numpy(sample).cuda()].cpu().numpy(), first), mode
        assert np.array_equal(counts.cpu().numpy()[sample].view(np.uint32), first_counts)
