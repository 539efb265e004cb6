"""The bf16 / fp16 kernels (memb_hip_narrow.hip; outputTileNarrow; hip_decode_launch.h: launchTrained, launchUniform, launchFull) over the
geometry the fp32 path is walked through in test_gpu_parity.py: lanes per word and block sizes, the finer index forced on
and off, key forms and table widths, row layouts, the batch-size edges of the plan, very wide rows, arbitrary prefix
codes, degenerate models, a seeded sweep, threads on streams of their own.

The reference everywhere: the CPU checker's fp32 rows (for C-ABI models the numpy gather of the fp32 test) converted on
the CPU by torch.Tensor.to(dtype); bit for bit, NaN by position. Every batch holds missing rows -- 0xFFFFFFFF and ids
>= n_rows, the first and the last row of the batch among them, and a run of them that covers a whole tile."""
import ctypes
import os
import threading

import numpy as np
import pytest

import oracle
from test_gpu_narrow import SENTINEL, assert_narrow_equal, expected_rows, narrow_types

pytestmark = pytest.mark.gpu

OUT_SCALAR, OUT_VEC4, OUT_FLAT = 0, 1, 2   # hip_trained_kernels.h: OutputMode
WAVE = 64
MISSING_RUN = 2 * WAVE   # consecutive missing rows: a whole tile of them at any number of words per wavefront, wherever tiles start

# (dtype name, 'trained', HAS_SUB, MODE, FAST) and (dtype name, storage, VEC4) of every decode this file ran
REACHED = set()
TRAINED_INSTANCES = {(has_sub, mode, fast) for has_sub, fast in ((False, True), (False, False), (True, False))
                     for mode in (OUT_SCALAR, OUT_VEC4, OUT_FLAT)}   # memb_hip_narrow.hip: NarrowTable
ROWWISE_INSTANCES = {(storage, vec4) for storage in ('uniform', 'full') for vec4 in (False, True)}


def checker_threads():
    return min(16, os.cpu_count() or 1)


def batch_with_misses(count, n_rows, seed, rows=None):
    """`count` row ids (random unless given) with both kinds of missing row sprinkled in, at the first and the last
    position, and MISSING_RUN of them in a row (a third of the batch where it is shorter than 3 * MISSING_RUN)"""
    rng = np.random.default_rng(seed)
    if rows is None:
        rows = rng.integers(0, n_rows, size=count, dtype=np.int64)
    rows = np.array(rows, dtype=np.int64)
    assert len(rows) == count and count >= 1
    rows[::7] = 0xFFFFFFFF
    rows[3::11] = n_rows + 5
    run = min(MISSING_RUN, count // 3)
    start = int(rng.integers(0, count - run + 1))
    rows[start:start + run:2] = 0xFFFFFFFF
    rows[start + 1:start + run:2] = n_rows + np.arange(len(rows[start + 1:start + run:2]))
    rows[0] = n_rows if seed % 2 else 0xFFFFFFFF
    rows[-1] = 0xFFFFFFFF if seed % 2 else n_rows
    return rows.astype(np.uint32)


def expected_of(checker, rows):
    return {dtype: expected_rows(checker, rows, dtype) for dtype in narrow_types()}


def narrow_output_mode(dim, ld, col_off, pointer, words_per_wave):
    """hip_decode_plan.h: outputMode for 2-byte elements, restated"""
    if dim % 4 or ld % 4 or col_off % 4 or pointer % 8:
        return OUT_SCALAR
    dense = ld == dim and col_off == 0 and pointer % 16 == 0
    return OUT_FLAT if dense and (dim % 8 == 0 or words_per_wave % 2 == 0) else OUT_VEC4


def key_form(reader):
    """(HAS_SUB, FAST) of the model's lookup kernels: the template arguments of the decode_trained instance of a small batch"""
    name = reader.info(1)['kernel']
    assert name.startswith('decode_trained<') and name.endswith('>'), name
    has_sub, _, fast = [argument.strip() for argument in name[len('decode_trained<'):-1].split(',')]
    assert has_sub in ('true', 'false') and fast in ('true', 'false'), name
    assert not (has_sub == 'true' and fast == 'true'), name   # nibble keys have a one-level table
    return has_sub == 'true', fast == 'true'


# (name, col_off, spare columns, elements the matrix starts into its buffer)
DENSE = ('dense', 0, 0, 0)
LAYOUTS = (DENSE, ('col_off 4', 4, 4, 0), ('col_off 2', 2, 1, 0), ('dense, 8-byte aligned', 0, 0, 4), ('dense, 2-byte aligned', 0, 0, 1))


def decode_into_sentinels(reader, device_rows, dtype, dim, col_off, spare, shift, context):
    """Rows into columns [col_off, col_off + dim) of an (n, col_off + dim + spare) matrix that starts `shift` elements into a
    buffer of sentinels; everything around the rows must still be sentinels. Returns (rows, pointer, ld)."""
    import torch
    n = device_rows.numel()
    width = col_off + dim + spare
    buffer = torch.full((shift + n * width + 8,), SENTINEL, dtype=torch.int16, device='cuda')
    matrix = buffer[shift:shift + n * width].view(n, width)
    out = reader.rows_embedding_device(device_rows, out=matrix.view(dtype), col_off=col_off)
    torch.cuda.synchronize()
    assert out.data_ptr() == matrix.data_ptr()
    assert bool((buffer[:shift] == SENTINEL).all()) and bool((buffer[shift + n * width:] == SENTINEL).all()), context
    assert bool((matrix[:, :col_off] == SENTINEL).all()) and bool((matrix[:, col_off + dim:] == SENTINEL).all()), context
    return matrix[:, col_off:col_off + dim].view(dtype), matrix.data_ptr(), width


def check_reader(reader, storage, dim, rows, expected, label, fines=(1, 2), layouts=LAYOUTS):
    """Both dtypes into every layout, trained models with the finer index never (1) and always (2) -- so the words per
    wavefront are what info() says -- against `expected` ({dtype: rows}); notes the kernel instance of every decode.
    Every decode is compared before the first mismatch is reported, each with the instance that ran. Returns the modes
    that ran."""
    import torch
    device_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    trained = storage == 'trained'
    modes = set()
    failures = []
    for fine in fines if trained else (None,):
        words_per_wave = 0
        if trained:
            reader.set_option('fine_lanes', fine)
            has_sub, fast = key_form(reader)
            words_per_wave = WAVE // reader.info(len(rows))['lanes_per_word']
        for dtype in narrow_types():
            for name, col_off, spare, shift in layouts:
                context = (label, storage, dim, len(rows), 'fine_lanes', fine, 'words', words_per_wave, dtype, name)
                got, pointer, ld = decode_into_sentinels(reader, device_rows, dtype, dim, col_off, spare, shift, context)
                type_name = str(dtype)
                if trained:
                    mode = narrow_output_mode(dim, ld, col_off, pointer, words_per_wave)
                    modes.add(mode)
                    instance = (type_name, 'trained', has_sub, mode, fast)
                else:
                    vec4 = dim % 4 == 0 and ld % 4 == 0 and col_off % 4 == 0 and pointer % 8 == 0   # launchUniform / launchFull: outputMode != OUT_SCALAR
                    instance = (type_name, storage, vec4)
                REACHED.add(instance)
                try:
                    assert_narrow_equal(got, expected[dtype], context)
                except AssertionError:
                    failures.append('{} {}'.format(instance, context))
    assert not failures, '{} decodes differ from the checker:\n{}'.format(len(failures), '\n'.join(failures[:12]))
    return modes


def set_environment(monkeypatch, **values):
    for key in ('MEMB_HIP_LANES', 'MEMB_HIP_WAVES', 'MEMB_HIP_ROOT_BITS', 'MEMB_HIP_NO_FAST', 'MEMB_HIP_ROW_RECORDS', 'MEMB_HIP_ROW_META'):
        monkeypatch.delenv(key, raising=False)
    for key, value in values.items():
        monkeypatch.setenv(key, str(value))


# ---- 1. tile geometries ----

GEOMETRIES = ((1, 1), (1, 4), (2, 4), (3, 2), (4, 8), (5, 4), (8, 4), (8, 8), (16, 2), (25, 1), (64, 1))   # (lanes, waves)


@pytest.mark.parametrize('bits,distribution', [(4, 'normal'), (8, 'student')])
def test_tile_geometries(native, make_model, monkeypatch, bits, distribution):
    """The (lanes per word, waves per block) list of test_gpu_parity.py::test_tile_geometries_give_identical_rows on a
    nibble-key model and a byte-key model with sub-tables, dense and strided (col_off 4, 4 spare columns). Spare lanes
    (3, 5, 25 lanes), one word per wavefront (64) and the absent ballot of nibble keys shifted by word * lanes."""
    path, _ = make_model(20000, 300, 'trained', bits, distribution=distribution)
    checker = oracle.OracleReader(path)
    rows = batch_with_misses(6667, 20000, bits, rows=np.arange(0, 20000, 3))
    expected = expected_of(checker, rows)
    lanes_seen = set()
    for lanes, waves in GEOMETRIES:
        set_environment(monkeypatch, MEMB_HIP_LANES=lanes, MEMB_HIP_WAVES=waves)
        reader = native.Reader(path)
        has_sub, fast = key_form(reader)
        assert fast == (bits == 4)
        check_reader(reader, 'trained', 300, rows, expected, (bits, lanes, waves), layouts=(DENSE, ('col_off 4', 4, 4, 0)))
        if not fast and not has_sub:
            # the byte-key kernels' first level covers codes of up to 13 bits: sub-tables by a narrower one
            two_level = native.Reader(path, max_direct_decode_bits=6)
            assert key_form(two_level) == (True, False)
            check_reader(two_level, 'trained', 300, rows, expected, (bits, lanes, waves, 'two levels'), layouts=(DENSE, ('col_off 4', 4, 4, 0)))
        reader.set_option('fine_lanes', 1)
        info = reader.info(len(rows))
        assert info['waves_per_block'] == waves
        assert info['lanes_per_word'] * info['segment_symbols'] >= 300
        assert info['lanes_per_word'] == -(-300 // info['segment_symbols'])
        lanes_seen.add(info['lanes_per_word'])
    # one and 64 words per wavefront and spare lanes were run (lanes are rounded to whole groups of symbols: 64 become 38)
    assert 1 in lanes_seen and max(lanes_seen) > WAVE // 2 and any(WAVE % lanes for lanes in lanes_seen), lanes_seen


@pytest.mark.parametrize('bits', [4, 6])
@pytest.mark.parametrize('dim', [300, 304])
def test_the_end_of_a_dense_tile(native, make_model, monkeypatch, bits, dim):
    """Dense rows of dim % 8 == 4 and dim % 8 == 0 at an odd and an even number of words per wavefront, the last tile of
    the batch 1 word, an odd and an even number of words: OUT_FLAT tiles that end in a 16-byte and in an 8-byte store, and
    the OUT_VEC4 fallback (dim % 8 == 4 at an odd number of words, whose tiles do not all start 16-byte aligned)."""
    path, _ = make_model(3000, dim, 'trained', bits)
    checker = oracle.OracleReader(path)
    parities, modes = set(), set()
    for lanes in (3, 8, 5, 64, 7):
        set_environment(monkeypatch, MEMB_HIP_LANES=lanes)
        reader = native.Reader(path)
        for fine in (1, 2):
            reader.set_option('fine_lanes', fine)
            words = WAVE // reader.info(1000)['lanes_per_word']
            parities.add(words % 2)
            odd = words - 1 if words % 2 == 0 else words - 2   # the largest odd / even number of words below a whole tile
            even = words - 2 if words % 2 == 0 else words - 1
            for last in sorted({1, max(odd, 1), max(even, 1) if words > 1 else 1, words}):
                count = 5 * words + last if last < words else 6 * words
                assert WAVE // reader.info(count)['lanes_per_word'] == words
                rows = batch_with_misses(count, 3000, count + lanes)
                ran = check_reader(reader, 'trained', dim, rows, expected_of(checker, rows), (bits, dim, lanes, 'last tile', last),
                                   fines=(fine,), layouts=(DENSE,))
                assert ran == {OUT_FLAT if dim % 8 == 0 or words % 2 == 0 else OUT_VEC4}
                modes |= ran
    assert parities == {0, 1}, parities
    assert modes == ({OUT_FLAT} if dim % 8 == 0 else {OUT_FLAT, OUT_VEC4}), modes


# ---- 3. key forms and tables ----

@pytest.mark.parametrize('bits', [1, 2, 4])
def test_small_codebooks_through_the_byte_key_kernel(native, make_model, monkeypatch, bits):
    # MEMB_HIP_NO_FAST: 2-byte codebook entries (valueLds) for a model that normally takes the pair table
    n_rows = 20000 if bits == 4 else 3000   # (the 4-bit model of 3000 rows has a code of more than 8 bits: byte keys anyway)
    path, _ = make_model(n_rows, 300, 'trained', bits)
    checker = oracle.OracleReader(path)
    rows = batch_with_misses(4001, n_rows, bits)
    expected = expected_of(checker, rows)
    for no_fast in (1, 0):
        set_environment(monkeypatch, **({'MEMB_HIP_NO_FAST': 1} if no_fast else {}))
        reader = native.Reader(path)
        assert key_form(reader)[1] == (not no_fast)
        check_reader(reader, 'trained', 300, rows, expected, (bits, 'no_fast', no_fast))


@pytest.mark.parametrize('bits', [5, 6, 7, 8])
def test_first_level_widths(native, make_model, monkeypatch, bits):
    # MEMB_HIP_ROOT_BITS: the first level of the table the segment indices are built with (the lookup kernels of byte keys
    # size theirs to the longest code, up to 13 bits); max_direct_decode_bits: that of both -- two-level tables in
    # decode_trained_narrow<true, ...>
    path, _ = make_model(3000, 300, 'trained', bits, distribution='student')
    checker = oracle.OracleReader(path)
    rows = batch_with_misses(4001, 3000, bits)
    expected = expected_of(checker, rows)
    forms = set()
    for root_bits, max_direct_bits in ((1, 0), (2, 0), (4, 0), (8, 0), (11, 0), (12, 0), (0, 1), (0, 4), (0, 5), (0, 8)):
        set_environment(monkeypatch, **({'MEMB_HIP_ROOT_BITS': root_bits} if root_bits else {}))
        reader = native.Reader(path, max_direct_decode_bits=max_direct_bits)
        info = reader.info()
        has_sub, fast = key_form(reader)
        # (the 5-bit model keeps 16 centroids and short codes: nibble keys unless its first level is narrowed)
        assert has_sub == (not fast and info['max_code_bits'] > info['root_bits']), info
        forms.add(has_sub)
        check_reader(reader, 'trained', 300, rows, expected, (bits, 'root_bits', root_bits, max_direct_bits), layouts=LAYOUTS[:3])
    assert True in forms, forms


@pytest.mark.parametrize('bits', [3, 5, 7])
@pytest.mark.parametrize('dim', [300, 7, 64])
def test_odd_bit_widths(native, make_model, bits, dim):
    path, _ = make_model(700, dim, 'trained', bits)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_with_misses(1000, 700, bits + dim)
    check_reader(reader, 'trained', dim, rows, expected_of(checker, rows), (bits, dim))


# ---- 4. row layouts ----

@pytest.mark.parametrize('bits,distribution', [(2, 'normal'), (4, 'normal'), (6, 'student'), (8, 'student')])
def test_row_layouts(native, make_model, monkeypatch, bits, distribution):
    # row records, compact streams + rowMeta records, compact streams + the two index arrays: a dump and random rows
    path, _ = make_model(20000, 300, 'trained', bits, distribution=distribution)
    checker = oracle.OracleReader(path)
    rows = batch_with_misses(9000, 20000, bits)
    dump = batch_with_misses(20000, 20000, bits + 1, rows=np.arange(20000))
    expected, expected_dump = expected_of(checker, rows), expected_of(checker, dump)
    layouts = {}
    for name, environment in (('records', {}), ('rowmeta', {'MEMB_HIP_ROW_RECORDS': '0'}), ('arrays', {'MEMB_HIP_ROW_META': '0'})):
        set_environment(monkeypatch, **environment)
        reader = native.Reader(path)
        layouts[name] = reader.info()['row_layout']
        check_reader(reader, 'trained', 300, rows, expected, (bits, name), layouts=(DENSE, ('col_off 4', 4, 4, 0)))
        check_reader(reader, 'trained', 300, dump, expected_dump, (bits, name, 'dump'), layouts=(DENSE,))
    assert layouts['rowmeta'] == 1 and layouts['arrays'] == 0, layouts
    assert layouts['records'] == 2 if distribution == 'normal' else layouts['records'] in (1, 2), (bits, layouts)


# ---- 5. batch-size edges of the narrow plan ----

@pytest.mark.parametrize('bits', [4, 6])
def test_batch_size_edges_of_the_narrow_plan(native, make_model, bits):
    """DEFAULT options, batch sizes on both sides of (a) the edge of the finer index (its tiles fill one round of resident
    wavefronts; the narrow launch sizes LDS with half a codebook, so the edge is worked out for both codebooks), (b) two
    tiles per resident wavefront slot, where oneTileSteps goes to two tiles per wavefront for models with 16 KiB of tables
    (here also forced: option tiles_per_wave), (c) 16 R tiles, from where blocks are eight wavefronts -- rows in key order
    and shuffled, at every size where fp32 runs decode_records_persistent too. The checker's rows of the whole vocabulary,
    converted on the CPU, are gathered and compared on the device."""
    import torch
    n_rows = 530000
    path, _ = make_model(n_rows, 300, 'trained', bits)
    reader = native.Reader(path)
    checker = oracle.OracleReader(path, checker_threads())
    vocabulary = np.append(np.arange(n_rows, dtype=np.uint32), np.uint32(0xFFFFFFFF))   # (the last row: the checker's missing row)
    fp32 = torch.from_numpy(checker.rows_embedding(vocabulary))
    tables = {dtype: fp32.to(dtype).cuda() for dtype in narrow_types()}
    del fp32
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    usual, fine = reader.info(), reader.info(1)
    usual_words, fine_words = WAVE // usual['lanes_per_word'], WAVE // fine['lanes_per_word']
    assert fine_words < usual_words
    codebook_bytes = 2048 if key_form(reader)[1] else 1024   # hip_decode_plan.h: codebookDwords

    def one_round(info, saved):
        # test_gpu_parity.py::test_small_batches_decode_with_the_finer_index; `saved`: what half a codebook leaves out
        waves, lds = info['waves_per_block'], info['lds_bytes_per_block'] - saved
        return cus * waves * min(160 * 1024 // ((lds + 1023) // 1024 * 1024), max(1, 28 // waves))

    counts = set()
    for saved in (0, codebook_bytes // 2):
        edge = one_round(fine, saved) * fine_words
        counts |= {edge - 1, edge, edge + 1, edge + fine_words + 1}
    two_tiles = 2 * 32 * cus * usual_words
    counts |= {two_tiles - usual_words, two_tiles - 3, two_tiles, two_tiles + 5}
    blocks_of_eight = 16 * 16 * cus * usual_words
    counts |= {blocks_of_eight - 3, blocks_of_eight, blocks_of_eight + 1, blocks_of_eight + usual_words + 3}
    lanes_seen, waves_seen = set(), set()

    def check(count, label):
        info = reader.info(count)
        lanes_seen.add(info['lanes_per_word'])
        waves_seen.add(info['waves_per_block'])
        in_order = batch_with_misses(count, n_rows, count, rows=np.arange(count) % n_rows)
        shuffled = np.random.default_rng(count).permutation(in_order)
        shuffled[0], shuffled[-1] = in_order[0], in_order[-1]
        for order, rows in (('key order', in_order), ('shuffled', shuffled)):
            ids = torch.from_numpy(rows.view(np.int32)).cuda()
            index = torch.from_numpy(np.minimum(rows, n_rows).astype(np.int64)).cuda()
            for dtype in narrow_types():
                got = reader.rows_embedding_device(ids, dtype=dtype)
                want = tables[dtype][index]
                nan = torch.isnan(want)
                assert torch.equal(torch.isnan(got), nan), (bits, count, label, order, dtype)
                wrong = int(((got.view(torch.int16) != want.view(torch.int16)) & ~nan).sum())
                assert wrong == 0, (bits, count, label, order, dtype, wrong, info['kernel'], info['lanes_per_word'], info['waves_per_block'])

    for count in sorted(counts):
        check(count, 'default')
    assert len(lanes_seen) == 2 and {4, 8} <= waves_seen, (lanes_seen, waves_seen)   # (what fp32 plans: both sides of (a) and (c))
    reader.set_option('tiles_per_wave', 2)
    for count in (two_tiles - 3, two_tiles + 5, blocks_of_eight + 1):
        check(count, 'two tiles per wavefront')
    reader.set_option('tiles_per_wave', 0)


# ---- 6. wide rows ----

@pytest.mark.parametrize('dim,bits,count', [(4096, 8, 120), (9000, 8, 40), (20000, 4, 30), (60000, 8, 10), (100000, 2, 6)])
def test_very_wide_trained_rows(native, make_model, dim, bits, count):
    # the shapes of test_gpu_parity.py::test_very_wide_rows: up to one word per wavefront, 32-bit segment indices
    path, _ = make_model(count, dim, 'trained', bits, seed=dim)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    info = reader.info()
    assert info['lanes_per_word'] * info['segment_symbols'] >= dim
    rows = batch_with_misses(200, count, dim)
    check_reader(reader, 'trained', dim, rows, expected_of(checker, rows), (dim, bits), layouts=(DENSE, ('col_off 2', 2, 0, 0)))


@pytest.mark.parametrize('storage', ['uniform', 'full'])
@pytest.mark.parametrize('dim', [4096, 4100, 5001, 20000])
def test_very_wide_rowwise_rows(native, make_model, storage, dim):
    # one word per block of the row-wise kernels (rowwiseWordsPerBlock: 4096 / dim), pieceMagic over one row
    path, _ = make_model(40, dim, storage, 8, seed=dim)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_with_misses(300, 40, dim)
    check_reader(reader, storage, dim, rows, expected_of(checker, rows), (storage, dim), layouts=LAYOUTS[:4])


# ---- 7. arbitrary prefix codes ----

def test_arbitrary_prefix_codes_through_the_typed_entry(native):
    # the contexts of test_gpu_parity.py::test_arbitrary_prefix_codes_through_the_c_abi (codes of 15 bits and more, first
    # levels of 0 = default, 1, 5 and 12 bits) through memb_hip_decode_rows_device_typed; expected: that test's numpy gather
    import torch
    from test_gpu_parity import prefix_code_contexts
    longest = 0
    for library, context, label, dim, n_rows, expected, rng, longest in prefix_code_contexts(native):
        for count in (n_rows, min(n_rows, 100)):
            ids = batch_with_misses(count, n_rows, count, rows=rng.permutation(n_rows)[:count])
            want = torch.from_numpy(np.where((ids >= n_rows)[:, None], np.float32(0), expected[np.minimum(ids, n_rows - 1)]))
            device_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            for dtype, code in ((torch.bfloat16, 1), (torch.float16, 2)):
                for col_off, spare in ((0, 0), (4, 4), (1, 2)):
                    width = col_off + dim + spare
                    out = torch.full((count, width), SENTINEL, dtype=torch.int16, device='cuda')
                    status = library.memb_hip_decode_rows_device_typed(
                        context, ctypes.c_void_p(device_ids.data_ptr()), ctypes.c_size_t(count), ctypes.c_void_p(out.data_ptr()),
                        code, ctypes.c_size_t(width), ctypes.c_size_t(col_off), None)
                    assert status == 0, library.memb_hip_last_error()
                    torch.cuda.synchronize()
                    assert_narrow_equal(out[:, col_off:col_off + dim].view(dtype), want.to(dtype), (label, count, dtype, col_off))
                    assert bool((out[:, :col_off] == SENTINEL).all()) and bool((out[:, col_off + dim:] == SENTINEL).all())
    assert longest >= 15


# ---- 8. degenerate models and special values ----

def test_degenerate_models(native, tmp_path):
    # the models of test_gpu_parity.py::test_degenerate_models: batches of one row (present, and missing), of the
    # vocabulary and of 700
    from test_gpu_parity import degenerate_cases
    for index, (storage, bits, names, vectors) in enumerate(degenerate_cases()):
        path = str(tmp_path / 'degenerate_{}.bin'.format(index))
        builder = native.Builder(vectors.shape[1], storage, bits)
        builder.add_words(names, vectors)
        builder.save(path)
        reader, checker = native.Reader(path), oracle.OracleReader(path)
        count, dim = len(names), vectors.shape[1]
        batches = [np.array([count - 1], dtype=np.uint32), np.array([0xFFFFFFFF], dtype=np.uint32), np.array([count], dtype=np.uint32),
                   batch_with_misses(count + 3, count, index, rows=np.arange(count + 3) % count),
                   batch_with_misses(700, count, index)]
        for rows in batches:
            check_reader(reader, storage, dim, rows, expected_of(checker, rows), (index, storage, bits, len(rows)), layouts=LAYOUTS[:3])


# ---- 9. seeded sweep ----

def test_randomized_models_and_batches(native, tmp_path, monkeypatch):
    """The sweep of test_gpu_parity.py::test_randomized_models_and_batches (dimension, vocabulary, storage, bit width, lanes
    per word, first-level width, batch make-up) with a random dtype, finer index, column offset and spare columns, through
    rows_embedding_device(dtype=...); the columns around the rows keep their sentinel."""
    # (MEMB_TEST_SWEEP_TRIALS / MEMB_TEST_SWEEP_SEED: longer one-off sweeps with other seeds)
    import torch
    rng = np.random.default_rng(int(os.environ.get('MEMB_TEST_SWEEP_SEED', 2024)) + 1)
    for trial in range(int(os.environ.get('MEMB_TEST_SWEEP_TRIALS', 40))):
        dim = int(rng.choice([1, 2, 3, 4, 7, 8, 12, 16, 20, 31, 32, 48, 63, 64, 96, 100, 128, 200, 257, 300, 512]))
        count = int(rng.integers(1, 2500))
        storage = str(rng.choice(['trained', 'trained', 'trained', 'uniform', 'full']))
        bits = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8]))
        scale = float(rng.choice([1e-3, 0.4, 50.0]))
        if rng.random() < 0.5:
            vectors = (rng.standard_normal((count, dim)) * scale).astype(np.float32)
        else:
            vectors = (rng.standard_t(3, size=(count, dim)) * scale).astype(np.float32)
        words = ['t{}w{}'.format(trial, i) for i in rng.permutation(count)]
        builder = native.Builder(dim, storage, bits)
        builder.add_words(words, vectors)
        path = tmp_path / 'r{}.bin'.format(trial)
        builder.save(path)

        set_environment(monkeypatch, MEMB_HIP_LANES=int(rng.choice([1, 2, 3, 4, 8, 8, 16, 32])),
                        MEMB_HIP_ROOT_BITS=int(rng.choice([1, 2, 4, 8, 11, 12])))
        reader = native.Reader(path)
        checker = oracle.OracleReader(str(path))
        fine = int(rng.integers(0, 3))
        if storage == 'trained':
            reader.set_option('fine_lanes', fine)

        n = int(rng.choice([1, 2, 5, 64, 65, 300, 1500]))
        miss_rate = float(rng.choice([0.0, 0.1, 0.9]))
        rows = rng.integers(0, count, size=n, dtype=np.int64)
        rows[rng.random(n) < miss_rate] = 0xFFFFFFFF
        rows = batch_with_misses(n, count, trial, rows=rows) if n > 2 else rows.astype(np.uint32)
        dtype = narrow_types()[int(rng.integers(0, 2))]
        col_off = int(rng.choice([0, 1, 2, 4, 8]))
        spare = int(rng.choice([0, 1, 3, 4, 64]))
        context = (trial, dim, count, storage, bits, n, dtype, 'fine_lanes', fine, col_off, spare)
        device_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        got, _, _ = decode_into_sentinels(reader, device_rows, dtype, dim, col_off, spare, 0, context)
        assert_narrow_equal(got, expected_rows(checker, rows, dtype), context)
        other = narrow_types()[0] if dtype == narrow_types()[1] else narrow_types()[1]
        assert_narrow_equal(reader.rows_embedding_device(device_rows, dtype=other), expected_rows(checker, rows, other), context)


# ---- 10. threads and streams ----

@pytest.mark.parametrize('bits,distribution', [(4, 'normal'), (8, 'student')])
def test_six_threads_on_streams_of_their_own(native, make_model, bits, distribution):
    """One fresh Reader, six threads that start behind a barrier, each on a stream of its own: bf16, fp16 and fp32 calls of
    1 .. 100 000 rows mixed, the first narrow launch of the process's per-thread kernel tables (launchKernelAddress) among
    them; every result against the checker."""
    import torch
    path, _ = make_model(20000, 300, 'trained', bits, distribution=distribution)
    checker = oracle.OracleReader(path, checker_threads())
    types = [torch.bfloat16, torch.float16, torch.float32]
    jobs = []
    for thread in range(6):
        mine = []
        for k, size in enumerate((1, 100000, 70, 6000, 1500, 31)):
            rows = batch_with_misses(size, 20000, 100 * thread + k) if size > 2 else np.array([thread], dtype=np.uint32)
            dtype = types[(thread + k) % 3]
            want = torch.from_numpy(checker.rows_embedding(rows))
            mine.append((torch.from_numpy(rows.view(np.int32)).cuda(), dtype, want if dtype == torch.float32 else want.to(dtype)))
        jobs.append(mine)
    torch.cuda.synchronize()
    reader = native.Reader(path)   # nothing launched through it yet
    barrier = threading.Barrier(6)
    failures = []

    def run(thread):
        try:
            stream = torch.cuda.Stream()
            barrier.wait()
            with torch.cuda.stream(stream):
                for repeat in range(3):
                    for ids, dtype, want in jobs[thread]:
                        got = reader.rows_embedding_device(ids, dtype=dtype)
                        stream.synchronize()
                        got = got.cpu()
                        if dtype == torch.float32:
                            same = torch.equal(got.view(torch.int32), want.view(torch.int32))
                        else:
                            same = torch.equal(got.view(torch.int16), want.view(torch.int16))
                        if not same:
                            failures.append((thread, repeat, ids.numel(), dtype))
        except Exception as error:   # (a thread's exception is a failure of the test, not a line on stderr)
            failures.append((thread, repr(error)))

    threads = [threading.Thread(target=run, args=(thread,)) for thread in range(6)]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join()
    assert not failures, failures


# ---- 2. which instance ran ----

def test_every_narrow_instance_is_reached(native, make_model, monkeypatch):
    """info() does not name the narrow kernel: check_reader restates outputMode for every decode and takes HAS_SUB and
    FAST from the model's decode_trained instance. The cases below alone must reach the nine decode_trained_narrow
    instances and the four row-wise ones of each dtype; whatever the other tests of this file ran is counted as well."""
    before = set(REACHED)
    REACHED.clear()
    try:
        cases = [(4, 'normal', {}, 0, (False, True)),                       # nibble keys
                 (4, 'normal', {'MEMB_HIP_NO_FAST': 1}, 0, (False, False)),   # byte keys, one-level table
                 (8, 'student', {}, 4, (True, False))]                        # byte keys, two-level table
        for bits, distribution, environment, max_direct_bits, form in cases:
            path, _ = make_model(20000, 300, 'trained', bits, distribution=distribution)
            set_environment(monkeypatch, **environment)
            reader, checker = native.Reader(path, max_direct_decode_bits=max_direct_bits), oracle.OracleReader(path)
            assert key_form(reader) == form
            rows = batch_with_misses(1001, 20000, bits)
            check_reader(reader, 'trained', 300, rows, expected_of(checker, rows), ('instances', bits, form))
        set_environment(monkeypatch)
        for storage in ('uniform', 'full'):
            path, _ = make_model(700, 300, storage, 8)
            reader, checker = native.Reader(path), oracle.OracleReader(path)
            rows = batch_with_misses(1001, 700, 8)
            check_reader(reader, storage, 300, rows, expected_of(checker, rows), ('instances', storage))
        for dtype in narrow_types():
            trained = {entry[2:] for entry in REACHED if entry[0] == str(dtype) and entry[1] == 'trained'}
            rowwise = {entry[1:] for entry in REACHED if entry[0] == str(dtype) and entry[1] != 'trained'}
            print('{}: decode_trained_narrow<HAS_SUB, MODE, FAST> reached: {}; row-wise (storage, VEC4): {}'.format(
                dtype, sorted(trained), sorted(rowwise)))
            assert trained == TRAINED_INSTANCES, (dtype, TRAINED_INSTANCES - trained)
            assert rowwise == ROWWISE_INSTANCES, (dtype, ROWWISE_INSTANCES - rowwise)
    finally:
        REACHED.update(before)
