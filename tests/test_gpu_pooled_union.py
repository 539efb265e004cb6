"""Pooled lookups of a ReadersUnion on the GPU (memb_hip_pooled_union.hip: pool_trained_union, pool_dense; hip_pooled_launch.h:
launchPooledUnion, launchPooledDense; readers_union.py: pooled_rows_device, pooled_sentences_device, pooled_rows).

The oracle everywhere is built on the host: every reader's own fp32 rows from rows_embedding_device -- which
test_gpu_parity.py pins bit for bit to the CPU checker --, merged in numpy float32 by the explicit order of the contract
(include/memb_hip_pooled_union.h: np.add in reader order, one np.divide by R; np.hstack for 'concatenate') and pooled by
the explicit loop of include/memb_hip_pooled.h. Compared with bits_equal: the tolerance is zero."""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import into_a_frame, to_device, union_values
from pooled_reference import ids_with_misses, merged_rows, offsets_of, pooled_by_the_contract, union_ids

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)
N_ROWS = 3000
FUSED, DENSE = 'pool_trained_union<', 'pool_dense<'


def template_arguments(name):
    return name.split('<')[1].split('>')[0].split(', ')


def check_union(union, readers, rows, offsets, context, modes=('sum', 'mean'), col_off=0, spare=0, kernel=None, union_mode='average',
                values=None):
    """Both pooling modes against the contract over the merged rows; the columns around the bags keep their sentinel;
    kernel: what last_pooled_kernel must start with. Returns the result of the first mode."""
    dim = union.dim
    device_rows = [to_device(ids) for ids in rows]
    device_offsets = to_device(offsets)
    if values is None:
        values = union_values(union_mode, readers, rows)
    bags = len(offsets) - 1
    results = {}
    for mode in modes:
        got = into_a_frame(lambda out: union.pooled_rows_device(device_rows, device_offsets, mode=mode, out=out, col_off=col_off),
                           bags, dim, context, col_off, spare, sentinel=SENTINEL).numpy()
        if kernel and bags:
            assert union.last_pooled_kernel.startswith(kernel), (context, union.last_pooled_kernel)
        want = pooled_by_the_contract(values, offsets, mode)
        if not bits_equal(got, want):
            bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            raise AssertionError('{} {}: {} of {} bags differ, first {}'.format(context, mode, len(bad), bags, bad[:8]))
        results[mode] = got
    return results[modes[0]]


def trained_readers(native, make_model, bits, dim=300, count=N_ROWS, **options):
    return [native.Reader(make_model(count, dim, 'trained', width, seed=31 + 7 * position + dim,
                                     distribution='student' if width == 8 else 'normal')[0], **options)
            for position, width in enumerate(bits)]


def nibble_keys(reader):
    """Whether the reader's own decode kernel takes nibble keys (decode_trained<HAS_SUB, MODE, FAST>): at most 16 centroids
    and no code longer than 8 bits, which for a 4-bit model depends on its data"""
    name = reader.info(1)['kernel']
    return name[len('decode_trained<'):-1].split(',')[2].strip() == 'true'


NIBBLE_SEEDS = (338, 345, 11, 22, 81, 91, 71, 5, 6, 7)   # 4-bit models of 3000 rows: most of these have no code beyond 8 bits


def nibble_key_pair(native, make_model):
    """Two 4-bit models of different seeds whose keys are nibbles"""
    readers = []
    for seed in NIBBLE_SEEDS:
        reader = native.Reader(make_model(N_ROWS, 300, 'trained', 4, seed=seed)[0])
        if nibble_keys(reader):
            readers.append(reader)
        if len(readers) == 2:
            return readers
    raise AssertionError('no two 4-bit models with nibble keys among the seeds {}'.format(NIBBLE_SEEDS))


# ---- 1. the fused kernel: bag shapes, per key form ----

@pytest.mark.parametrize('bits,nibbles', [((4, 4), True), ((4, 6), False), ((6, 8), False), ((2, 2), True)])
def test_fused_average_bag_shapes(native, make_model, bits, nibbles):
    import torch
    if bits == (4, 4):
        readers = nibble_key_pair(native, make_model)
    else:
        # (6, 8): two-level tables, forced as test_gpu_pooled.py forces them
        readers = trained_readers(native, make_model, bits, **({'max_direct_decode_bits': 1} if bits == (6, 8) else {}))
    assert all(nibble_keys(reader) for reader in readers) == nibbles, bits
    union = native.ReadersUnion(readers, 'average')
    assert union.last_pooled_kernel == ''
    rng = np.random.default_rng(sum(bits))

    def check(rows, offsets, what):
        return check_union(union, readers, rows, offsets, (bits, what), kernel=FUSED)

    # all bags of one entry: the merged rows themselves, bit for bit
    rows = union_ids(3001, 2, 1, N_ROWS)
    ones = check(rows, np.arange(3002), 'ones')
    assert bits_equal(ones, union_values('average', readers, rows))
    has_sub, fast, count, out_type = template_arguments(union.last_pooled_kernel)
    assert (fast, count, out_type) == ('true' if nibbles else 'false', '2', '0'), union.last_pooled_kernel
    # two-level tables: forced for (6, 8); nibble keys never have them; a mixed union decodes through the byte-key tables, of
    # which the 4-bit model's is one level (16 codes) and the 6-bit model's is what its own kernel says
    own_has_sub = [reader.info(1)['kernel'][len('decode_trained<'):-1].split(',')[0].strip() for reader in readers]
    assert has_sub == {(6, 8): 'true', (4, 6): own_has_sub[1]}.get(bits, 'false'), union.last_pooled_kernel
    # empty bags at the start, in the middle and at the end
    lengths = [0, 0, 0, 5, 1, 0, 12, 0, 0, 3, 64, 0, 9, 0, 0]
    check(union_ids(sum(lengths), 2, 2, N_ROWS), offsets_of(lengths), 'empties')
    # fixed lengths that straddle the 8-word tile
    for length in (7, 8, 9, 17):
        check(union_ids(length * 400, 2, length, N_ROWS), np.arange(0, length * 400 + 1, length), ('fixed', length))
    # seeded geometric lengths
    for mean_length in (3, 16):
        lengths = rng.geometric(1.0 / mean_length, size=500) - (rng.random(500) < 0.05)
        check(union_ids(int(lengths.sum()), 2, mean_length, N_ROWS), offsets_of(lengths), ('geometric', mean_length))
    # one bag that carries across hundreds of tiles, alone and between small ones
    check(union_ids(5000, 2, 5, N_ROWS), [0, 5000], 'one long bag')
    check(union_ids(5020, 2, 6, N_ROWS), offsets_of([3, 0, 7, 5000, 1, 9]), 'long bag among small')
    # every entry missing in every reader
    missing = [np.array([0xFFFFFFFF, N_ROWS, N_ROWS + 1, 0xFFFFFFFF, 0xFFFFFFFE], dtype=np.uint32),
               np.array([N_ROWS, 0xFFFFFFFF, 0xFFFFFFFF, N_ROWS + 7, N_ROWS], dtype=np.uint32)]
    nothing = check(missing, [0, 2, 5], 'all missing')
    assert not nothing.any() and not np.signbit(nothing).any()
    # n = 0: zeros for every bag, no sign bit
    zero = check([np.zeros(0, dtype=np.uint32)] * 2, [0, 0, 0, 0], 'n = 0')
    assert zero.shape == (3, 300) and not zero.any() and not np.signbit(zero).any()
    # bags = 0: nothing is launched, an empty result
    empty = union.pooled_rows_device([to_device(ids) for ids in rows], to_device([len(rows[0])]))
    assert tuple(empty.shape) == (0, 300)
    # offsets that run past n are clamped
    rows = union_ids(1000, 2, 8, N_ROWS)
    check(rows, np.array([0, 10, 25, 40, 5000, 0xFFFFFFFF], dtype=np.int64), 'offsets past n')
    torch.cuda.synchronize()


# ---- 2. three and four readers: the fused kernel takes them ("Pooled unions") ----

@pytest.mark.parametrize('count', [3, 4])
def test_three_and_four_readers(native, make_model, count):
    readers = trained_readers(native, make_model, (4,) * count)
    union = native.ReadersUnion(readers, 'average')
    lengths = np.random.default_rng(count).geometric(1 / 9.0, size=500)
    check_union(union, readers, union_ids(int(lengths.sum()), count, count, N_ROWS), offsets_of(lengths), ('readers', count), kernel=FUSED)
    fast = 'true' if all(nibble_keys(reader) for reader in readers) else 'false'
    assert template_arguments(union.last_pooled_kernel)[1:] == [fast, str(count), '0']
    ones = union_ids(700, count, 40 + count, N_ROWS)
    check_union(union, readers, ones, np.arange(701), ('readers', count, 'ones'), kernel=FUSED)


# ---- 3. dims and strided outputs ----

@pytest.mark.parametrize('dim,fused', [(64, True), (512, True), (4, True), (516, False), (302, False), (7, False), (1, False)])
def test_dims_and_strided_outputs(native, make_model, dim, fused):
    # (dim 4: 2-bit models, whose keys are always nibbles -- a nibble-key and a byte-key model of fewer than 8 columns differ
    # in their symbols per lane, 8 and 4, and cannot share a kernel)
    readers = trained_readers(native, make_model, (2, 2) if dim == 4 else (4, 4), dim=dim, count=700)
    union = native.ReadersUnion(readers, 'average')
    lengths = np.random.default_rng(dim).geometric(1 / 9.0, size=300)
    rows = union_ids(int(lengths.sum()), 2, dim, 700)
    values = union_values('average', readers, rows)
    for col_off, spare in ((0, 0), (4, 4), (2, 1)):
        # a destination that is not aligned to a piece takes the fallback whatever the dim
        kernel = FUSED if fused and col_off % 4 == 0 else DENSE
        check_union(union, readers, rows, offsets_of(lengths), (dim, col_off, spare), col_off=col_off, spare=spare, kernel=kernel,
                    values=values)


# ---- 4. the fallback: every other storage ----

def test_fallback_storages(native, make_model):
    uniform = [native.Reader(make_model(N_ROWS, 300, 'uniform', 8, seed=51 + position)[0]) for position in range(2)]
    full = native.Reader(make_model(N_ROWS, 300, 'full', 8, seed=53)[0])
    trained = trained_readers(native, make_model, (4, 4))
    lengths = np.random.default_rng(4).geometric(1 / 7.0, size=400)
    rows = union_ids(int(lengths.sum()), 2, 4, N_ROWS)
    for readers, what in ((uniform, 'uniform / uniform'), ([full, trained[0]], 'full / trained')):
        union = native.ReadersUnion(readers, 'average')
        check_union(union, readers, rows, offsets_of(lengths), what, kernel=DENSE)
        check_union(union, readers, rows, offsets_of(lengths), (what, 'strided'), col_off=3, spare=2, kernel=DENSE)
    # the switch that keeps a union's decode from its fused kernel keeps its pooled lookups from theirs
    union = native.ReadersUnion(trained, 'average')
    check_union(union, trained, rows, offsets_of(lengths), 'trained / trained', kernel=FUSED)
    trained[0].set_option('union_fused', 0)
    try:
        check_union(union, trained, rows, offsets_of(lengths), 'trained / trained, union_fused = 0', kernel=DENSE)
    finally:
        trained[0].set_option('union_fused', 1)


def test_subnormal_sums_with_mixed_signs(native, tmp_path):
    rng = np.random.default_rng(41)
    count, dim = 500, 300
    readers = []
    for position in range(2):
        # values of both signs between 1e-45 and 1e-40, exact zeros of both signs among them: every merged row and every
        # partial sum is subnormal
        vectors = (rng.integers(-70000, 70000, size=(count, dim)).astype(np.int64)).astype(np.float32) * np.float32(1.4e-45)
        vectors[rng.random((count, dim)) < 0.05] = -0.0
        vectors[0] = -0.0   # the first word in key order: -0.0 in both readers
        assert (np.abs(vectors) < 1.1754944e-38).all() and (vectors != 0).any()
        builder = native.Builder(dim, 'full', 8)
        builder.add_words(['s{:04d}'.format(i) for i in range(count)], vectors)
        path = str(tmp_path / 'subnormal_{}.bin'.format(position))
        builder.save(path)
        readers.append(native.Reader(path))
    union = native.ReadersUnion(readers, 'average')
    lengths = np.concatenate([[1, 1, 2, 2, 3], rng.geometric(1 / 10.0, size=400)])
    rows = [rng.integers(0, count, size=int(lengths.sum())).astype(np.uint32) for _ in range(2)]
    for ids in rows:
        ids[0] = 0
    total = check_union(union, readers, rows, offsets_of(lengths), 'subnormal sums', kernel=DENSE)
    assert (total != 0).any() and (np.abs(total[total != 0]) < 1.1754944e-38).all()
    # (-0.0 + -0.0) / 2 = -0.0 survives a bag of one entry
    assert np.signbit(total[0]).all() and not total[0].any()


def subset_model(native, tmp_path, name, dim, words, seed):
    """A 2-bit trained model (nibble keys whatever the data) of these words"""
    builder = native.Builder(dim, 'trained', 2)
    builder.add_words(words, np.random.default_rng(seed).standard_normal((len(words), dim)).astype(np.float32))
    path = str(tmp_path / name)
    builder.save(path)
    return native.Reader(path)


@pytest.mark.parametrize('dim,count', [(4, 2), (4, 3), (12, 3), (12, 4), (12, 2)])
def test_union_decode_where_a_tile_is_more_than_64_word_model_pairs(native, tmp_path, dim, count):
    # batch_embedding_device itself, nibble keys: one lane per word (dim 4: 64 words per tile) with two and three readers, and
    # two lanes per word (dim 12: 32 words) with three and four -- beside two readers there, which a tile's mask of missing
    # rows holds. Words that one reader lacks, another has: their rows are +0.0 in the one and must stay so in the merge.
    words = ['w{:04d}'.format(i) for i in range(900)]
    readers = [subset_model(native, tmp_path, 'r{}.bin'.format(position), dim, words[position::position + 1] if position else words, 7 + position)
               for position in range(count)]
    batch = words[::-1] + ['nowhere'] + words[:37]
    rows = [reader.batch_embedding_device(batch).cpu().numpy() for reader in readers]
    assert all((piece == 0).all(axis=1).any() for piece in rows[1:]) and not (rows[0][:900] == 0).all(axis=1).any()
    for union_mode in ('average', 'concatenate'):
        merged = native.ReadersUnion(readers, union_mode).batch_embedding_device(batch).cpu().numpy()
        assert bits_equal(merged, merged_rows(union_mode, rows)), (dim, count, union_mode)


# ---- 5. bf16 / fp16 results: the fp32 result rounded once ----

def test_narrow_results(native, make_model, tmp_path):
    import torch
    # a trained pair scaled so that sums of a few rows leave the fp16 range
    rng = np.random.default_rng(60)
    scaled = []
    for position in range(2):
        builder = native.Builder(300, 'trained', 4)
        builder.add_words(['w{:04d}'.format(i) for i in range(600)], (rng.standard_normal((600, 300)) * 30000).astype(np.float32))
        path = str(tmp_path / 'scaled_{}.bin'.format(position))
        builder.save(path)
        scaled.append(native.Reader(path))
    uniform = [native.Reader(make_model(N_ROWS, 300, 'uniform', 8, seed=51 + position)[0]) for position in range(2)]
    lengths = np.random.default_rng(6).geometric(1 / 6.0, size=300)
    overflowed = False
    for readers, n_rows, kernel in ((scaled, 600, FUSED), (trained_readers(native, make_model, (4, 6)), N_ROWS, FUSED),
                                    (uniform, N_ROWS, DENSE)):
        union = native.ReadersUnion(readers, 'average')
        rows = [to_device(ids) for ids in union_ids(int(lengths.sum()), 2, 6, n_rows)]
        offsets = to_device(offsets_of(lengths))
        for mode in ('sum', 'mean'):
            wide = union.pooled_rows_device(rows, offsets, mode=mode)
            assert wide.dtype == torch.float32 and union.last_pooled_kernel.startswith(kernel)
            for dtype in (torch.bfloat16, torch.float16):
                for col_off, spare in ((0, 0), (4, 4)):
                    out = torch.full((len(lengths), col_off + 300 + spare), float(SENTINEL), dtype=dtype, device='cuda')
                    union.pooled_rows_device(rows, offsets, mode=mode, out=out, col_off=col_off, dtype=dtype)
                    torch.cuda.synchronize()
                    assert union.last_pooled_kernel.startswith(kernel), union.last_pooled_kernel
                    want = wide.to(dtype)
                    assert torch.equal(out[:, col_off:col_off + 300].view(torch.int16), want.view(torch.int16)), (kernel, mode, dtype, col_off)
                    guards = torch.cat([out[:, :col_off], out[:, col_off + 300:]], dim=1)
                    assert (guards == float(SENTINEL)).all()
                    overflowed = overflowed or (dtype == torch.float16 and bool(torch.isinf(want).any()) and not bool(torch.isinf(wide).any()))
                fresh = union.pooled_rows_device(rows, offsets, mode=mode, dtype=torch.bfloat16)
                assert fresh.dtype == torch.bfloat16 and tuple(fresh.shape) == (len(lengths), 300)
    assert overflowed


# ---- 6. concatenate: every reader pools into its own columns ----

def test_concatenate(native, make_model):
    import torch
    readers = [native.Reader(make_model(N_ROWS, 300, 'trained', 4, seed=71)[0]), native.Reader(make_model(N_ROWS, 64, 'uniform', 8, seed=72)[0]),
               native.Reader(make_model(N_ROWS, 7, 'full', 8, seed=73)[0])]
    union = native.ReadersUnion(readers, 'concatenate')
    assert union.dim == 371
    lengths = np.random.default_rng(7).geometric(1 / 6.0, size=300) - 1
    rows = union_ids(int(lengths.sum()), 3, 7, N_ROWS)
    values = union_values('concatenate', readers, rows)
    for col_off in (0, 3):
        check_union(union, readers, rows, offsets_of(lengths), ('concatenate', col_off), col_off=col_off, spare=col_off,
                    union_mode='concatenate', values=values)
        device_rows, offsets = [to_device(ids) for ids in rows], to_device(offsets_of(lengths))
        for mode in ('sum', 'mean'):
            wide = union.pooled_rows_device(device_rows, offsets, mode=mode)
            out = torch.full((len(lengths), col_off + 371 + col_off), float(SENTINEL), dtype=torch.bfloat16, device='cuda')
            union.pooled_rows_device(device_rows, offsets, mode=mode, out=out, col_off=col_off, dtype=torch.bfloat16)
            assert torch.equal(out[:, col_off:col_off + 371].view(torch.int16), wide.to(torch.bfloat16).view(torch.int16))
            guards = torch.cat([out[:, :col_off], out[:, col_off + 371:]], dim=1)
            assert (guards == float(SENTINEL)).all()
    assert union.last_pooled_kernel == ''   # (of 'average' launches only)


# ---- 7. [r, r] averaged is r ----

def test_a_reader_averaged_with_itself_pools_like_the_reader(native, make_model):
    reader = native.Reader(make_model(N_ROWS, 300, 'trained', 4, seed=81)[0])
    union = native.ReadersUnion([reader, reader], 'average')
    lengths = np.random.default_rng(8).geometric(1 / 8.0, size=500)
    rows = to_device(ids_with_misses(int(lengths.sum()), N_ROWS, 8))
    offsets = to_device(offsets_of(lengths))
    for mode in ('sum', 'mean'):
        # (v + v) / 2 == v on normal-range data
        pooled = union.pooled_rows_device([rows, rows], offsets, mode=mode)
        assert union.last_pooled_kernel.startswith(FUSED)
        assert bits_equal(pooled.cpu().numpy(), reader.bags_embedding_device(rows, offsets, mode=mode).cpu().numpy())


# ---- 8. words ----

def test_words_and_host_arrays(native, make_model, tmp_path):
    import torch
    path_a, words_a = make_model(N_ROWS, 300, 'trained', 4, seed=91)
    # the second reader knows every other word of the first, and some words of its own
    words_b = words_a[::2] + ['own{:03d}'.format(i) for i in range(50)]
    builder = native.Builder(300, 'trained', 6)
    builder.add_words(words_b, np.random.default_rng(92).standard_normal((len(words_b), 300)).astype(np.float32))
    path_b = str(tmp_path / 'every_other_word.bin')
    builder.save(path_b)
    readers = [native.Reader(path_a), native.Reader(path_b)]
    known_b = set(readers[1].keys())
    only_a = [word for word in words_a if word not in known_b][:40]
    both = [word for word in words_a if word in known_b][:60]
    sentences = [both[:5], [], only_a[:3] + ['no such word'] + both[5:9] + ['own007', 'own049'], ['neither', 'of these'], only_a[3:30],
                 both[9:60] + only_a[30:40]]
    words = [word for sentence in sentences for word in sentence]
    offsets = offsets_of([len(sentence) for sentence in sentences])
    for union_mode in ('average', 'concatenate'):
        union = native.ReadersUnion(readers, union_mode)
        resolved = union.resolve_rows_device(words)
        assert len(resolved) == 2 and all(ids.dtype == torch.int32 for ids in resolved)
        for reader, ids in zip(readers, resolved):
            assert torch.equal(ids, reader.resolve_rows_device(words))
        host_ids = [ids.cpu().numpy().view(np.uint32) for ids in resolved]
        assert (host_ids[0] == 0xFFFFFFFF).any() and (host_ids[1] == 0xFFFFFFFF).any() and (host_ids[0] != host_ids[1]).any()
        for mode in ('sum', 'mean'):
            pooled = union.pooled_sentences_device(sentences, mode=mode)
            assert tuple(pooled.shape) == (len(sentences), union.dim)
            assert torch.equal(pooled.view(torch.int32), union.pooled_rows_device(resolved, to_device(offsets), mode=mode).view(torch.int32))
            assert not pooled[1].any() and not pooled[3].any()
            # host arrays through GPU readers, and the same union decoding on the host
            on_host = native.ReadersUnion([native.Reader(path_a, device='cpu'), native.Reader(path_b, device='cpu')], union_mode)
            through_gpu = union.pooled_rows(host_ids, offsets, mode=mode)
            assert bits_equal(through_gpu, pooled.cpu().numpy())
            assert bits_equal(through_gpu, on_host.pooled_rows(host_ids, offsets, mode=mode))
        narrow = union.pooled_sentences_device(sentences, dtype=torch.float16)
        assert narrow.dtype == torch.float16
    assert tuple(native.ReadersUnion(readers, 'average').pooled_sentences_device([]).shape) == (0, 300)


# ---- 9. refusals: nothing is launched, and a good call afterwards is right ----

def test_refusals(native, make_model):
    import torch
    readers = trained_readers(native, make_model, (4, 4))
    union = native.ReadersUnion(readers, 'average')
    lengths = [3, 0, 5, 9]
    rows = union_ids(sum(lengths), 2, 9, N_ROWS)
    device_rows, offsets = [to_device(ids) for ids in rows], to_device(offsets_of(lengths))
    sentinel = torch.full((4, 300), float(SENTINEL), dtype=torch.float32, device='cuda')

    def refused(error, match, *arguments, **keywords):
        with pytest.raises(error, match=match):
            union.pooled_rows_device(*arguments, **keywords)

    refused(ValueError, 'one row-id tensor per reader', device_rows[:1], offsets, out=sentinel)
    refused(ValueError, 'one row-id tensor per reader', device_rows + device_rows[:1], offsets, out=sentinel)
    refused(ValueError, 'equal length', [device_rows[0], device_rows[1][:-1]], offsets, out=sentinel)
    refused(TypeError, 'int32/uint32', [device_rows[0], device_rows[1].to(torch.int64)], offsets, out=sentinel)
    refused(TypeError, 'int32/uint32', [device_rows[0], device_rows[1].cpu()], offsets, out=sentinel)
    refused(TypeError, 'offsets', device_rows, offsets.cpu(), out=sentinel)
    refused(TypeError, 'offsets', device_rows, offsets.to(torch.int64), out=sentinel)
    refused(ValueError, 'narrower', device_rows, offsets, out=sentinel[:, :299])
    refused(ValueError, 'narrower', device_rows, offsets, out=sentinel, col_off=1)
    refused(TypeError, 'bags, width', device_rows, offsets, out=sentinel[:3])
    refused(ValueError, "'sum' or 'mean'", device_rows, offsets, mode='max', out=sentinel)
    refused(TypeError, 'unless dtype asks', device_rows, offsets, out=sentinel.to(torch.bfloat16))
    refused(TypeError, 'but dtype is', device_rows, offsets, out=sentinel, dtype=torch.float16)
    refused(TypeError, 'dtype must be', device_rows, offsets, dtype=torch.float64)
    with pytest.raises(TypeError):   # no such keywords on a union
        union.pooled_rows_device(device_rows, offsets, missing='skip')
    with pytest.raises(TypeError):
        union.pooled_rows_device(device_rows, offsets, reduction='chunked')
    torch.cuda.synchronize()
    assert (sentinel == float(SENTINEL)).all() and union.last_pooled_kernel == ''

    # the C entry points
    from memb_amd import _memb
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    fused = library.memb_hip_pool_rows_union_device
    fused.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                      ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dense = library.memb_hip_pool_dense_rows_device
    dense.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                      ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    narrow_reader = native.Reader(make_model(700, 64, 'trained', 4, seed=31 + 64)[0])
    for reader in readers + [narrow_reader]:
        reader.info()   # (stages the model)
    contexts = (ctypes.c_void_p * 2)(*[reader._impl.context_handle() for reader in readers])
    pointers = (ctypes.c_void_p * 2)(*[ids.data_ptr() for ids in device_rows])
    n, stream = len(rows[0]), torch.cuda.current_stream().cuda_stream
    invalid, unsupported = 1, 3   # MEMB_HIP_ERR_INVALID, MEMB_HIP_UNSUPPORTED
    assert fused(contexts, pointers, 2, n, None, 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == invalid   # offsets
    assert b'null' in library.memb_hip_last_error()
    assert fused(contexts, pointers, 2, n, offsets.data_ptr(), 4, None, 0, 300, 0, 1, stream) == invalid   # out
    assert fused(contexts, (ctypes.c_void_p * 2)(pointers[0], None), 2, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 1,
                 stream) == invalid
    assert fused(contexts, pointers, 2, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 299, 0, 1, stream) == invalid
    assert b'ld must be' in library.memb_hip_last_error()
    assert fused(contexts, pointers, 2, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 2, stream) == invalid
    assert b'pooling mode' in library.memb_hip_last_error()
    assert fused(contexts, pointers, 2, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 7, 300, 0, 1, stream) == invalid
    assert b'out_type' in library.memb_hip_last_error()
    # models of different dim cannot share the kernel; one model is no union
    different = (ctypes.c_void_p * 2)(readers[0]._impl.context_handle(), narrow_reader._impl.context_handle())
    assert fused(different, pointers, 2, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == unsupported
    assert b'differ' in library.memb_hip_last_error()
    assert fused(contexts, pointers, 1, n, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == unsupported
    values = torch.zeros((n, 300), dtype=torch.float32, device='cuda')
    assert dense(0, None, n, 300, 300, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == invalid
    assert b'null' in library.memb_hip_last_error()
    assert dense(0, values.data_ptr(), n, 300, 300, None, 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == invalid
    assert dense(0, values.data_ptr(), n, 300, 200, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 0, 1, stream) == invalid
    assert dense(0, values.data_ptr(), n, 300, 300, offsets.data_ptr(), 4, sentinel.data_ptr(), 0, 300, 1, 1, stream) == invalid
    torch.cuda.synchronize()
    assert (sentinel == float(SENTINEL)).all() and _memb.pool_union_kernel_name(readers[0]._impl) == ''

    # a good call afterwards, through both kernels
    check_union(union, readers, rows, offsets_of(lengths), 'after the refusals', kernel=FUSED)
    check_union(union, readers, rows, offsets_of(lengths), 'after the refusals, unaligned', col_off=1, kernel=DENSE)
