"""bf16 / fp16 device rows (include/memb_hip_narrow.h, Reader.rows_embedding_device(dtype=...)) bit for bit against the CPU
checker's fp32 rows converted by torch on the CPU: round to nearest even, once. NaNs compare by position."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from conftest import golden_json

pytestmark = pytest.mark.gpu

SENTINEL = 0x7E55   # a bit pattern no decoded value of these models has (a NaN in bf16 and fp16 alike)


def narrow_types():
    import torch
    return [torch.bfloat16, torch.float16]


def assert_narrow_equal(got, expected, context=''):
    """got, expected: torch tensors of one narrow dtype; the same bits, NaN wherever either is NaN"""
    import torch
    got = got.cpu()
    expected = expected.cpu()
    assert got.shape == expected.shape and got.dtype == expected.dtype, context
    nan_got, nan_expected = torch.isnan(got), torch.isnan(expected)
    assert torch.equal(nan_got, nan_expected), context
    same = got.view(torch.int16) == expected.view(torch.int16)
    assert bool((same | nan_got).all()), (context, int((~(same | nan_got)).sum()))


def expected_rows(checker, rows, dtype):
    import torch
    return torch.from_numpy(checker.rows_embedding(np.ascontiguousarray(rows, dtype=np.uint32))).to(dtype)


def batch_of(count, n_rows, seed, misses=True):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=count, dtype=np.int64).astype(np.uint32)
    if misses and count:
        rows[::7] = 0xFFFFFFFF
        rows[3::11] = np.uint32(n_rows + 5)   # ids >= len: missing too
    return rows


def decode(reader, rows, dtype, **kwargs):
    import torch
    device_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    out = reader.rows_embedding_device(device_rows, dtype=dtype, **kwargs)
    torch.cuda.synchronize()
    return out


# ---- every storage and key form, dims around the vector widths, ragged batch sizes ----

MODELS = [('trained', 1), ('trained', 2), ('trained', 4), ('trained', 6), ('trained', 8), ('uniform', 8), ('full', 8)]


@pytest.mark.parametrize('storage,bits', MODELS)
@pytest.mark.parametrize('dim', [1, 2, 3, 4, 7, 8, 300, 301])
def test_models_and_dims(native, make_model, storage, bits, dim):
    path, _ = make_model(700, dim, storage, bits)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_of(1000, 700, dim)
    for dtype in narrow_types():
        assert_narrow_equal(decode(reader, rows, dtype), expected_rows(checker, rows, dtype), (storage, bits, dim, dtype))


@pytest.mark.parametrize('bits,max_direct_bits', [(4, 0), (6, 0), (8, 0), (6, 3), (8, 4)])
def test_one_and_two_level_tables(native, make_model, bits, max_direct_bits):
    # byte keys with sub-tables (decode_trained_narrow<true, ...>) where the first level is forced narrow
    path, _ = make_model(3000, 300, 'trained', bits, distribution='student')
    reader = native.Reader(path, max_direct_decode_bits=max_direct_bits)
    checker = oracle.OracleReader(path)
    rows = batch_of(5000, 3000, bits)
    for dtype in narrow_types():
        assert_narrow_equal(decode(reader, rows, dtype), expected_rows(checker, rows, dtype), (bits, max_direct_bits, dtype))


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 100000])
def test_batch_sizes(native, make_model, count):
    import torch
    path, _ = make_model(20000, 300, 'trained', 4)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_of(count, 20000, count)
    for dtype in narrow_types():
        out = decode(reader, rows, dtype)
        assert out.dtype == dtype and out.shape == (count, 300)
        assert_narrow_equal(out, expected_rows(checker, rows, dtype), (count, dtype))
    if count == 0:
        empty = torch.empty((0, 300), dtype=torch.bfloat16, device='cuda')
        assert reader.rows_embedding_device(torch.empty(0, dtype=torch.int32, device='cuda'), out=empty) is empty


@pytest.mark.parametrize('bits', [4, 6])
def test_large_batches_in_key_order_and_shuffled(native, make_model, bits):
    import torch
    count = 530000
    path, _ = make_model(count, 300, 'trained', bits)
    reader = native.Reader(path)
    rows = torch.arange(count, dtype=torch.int32, device='cuda')
    rows[::997] = -1
    fp32 = reader.rows_embedding_device(rows)
    shuffled = rows[torch.randperm(count, device='cuda', generator=torch.Generator(device='cuda').manual_seed(bits))]
    fp32_shuffled = reader.rows_embedding_device(shuffled)
    for dtype in narrow_types():
        assert_narrow_equal(reader.rows_embedding_device(rows, dtype=dtype), fp32.to(dtype), (bits, dtype))
        assert_narrow_equal(reader.rows_embedding_device(shuffled, dtype=dtype), fp32_shuffled.to(dtype), (bits, dtype))
    # and against the checker, a slice of each
    checker = oracle.OracleReader(path)
    picked = shuffled[:40000].cpu().numpy().view(np.uint32)
    assert_narrow_equal(reader.rows_embedding_device(shuffled[:40000].contiguous(), dtype=torch.bfloat16),
                        expected_rows(checker, picked, torch.bfloat16), bits)


def test_full_size_dump_in_bf16(native):
    # BASELINE.json's headline: 2 196 017 x 300, 4-bit, the whole vocabulary in key order; every slice against the device's
    # fp32 dump rounded by torch, and the first and last slices against the checker itself
    import torch
    from memb_amd import synthetic
    count = int(os.environ.get('MEMB_TEST_FULL_VOCAB', 2196017))
    path, _ = synthetic.cached_model(count, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = torch.arange(count, dtype=torch.int32, device='cuda')
    out = reader.rows_embedding_device(rows, dtype=torch.bfloat16)
    fp32 = reader.rows_embedding_device(rows)
    torch.cuda.synchronize()
    step = 200000
    for start in range(0, count, step):
        stop = min(count, start + step)
        assert_narrow_equal(out[start:stop], fp32[start:stop].to(torch.bfloat16), (start, stop))
    checker = oracle.OracleReader(path)
    for start in (0, max(0, count - step)):
        stop = min(count, start + step)
        assert_narrow_equal(out[start:stop], expected_rows(checker, np.arange(start, stop, dtype=np.uint32), torch.bfloat16), start)


# ---- conversion edges ----

def test_uniform_expression_vectors(native):
    # every (min, max, value, levels) of tests/golden/uniform_expr.json -- subnormals, infinities, NaN, levels 0 and 1,
    # max < min -- through dequant_uniform_narrow: the golden fp32 result, rounded by torch
    import torch
    cases = golden_json('uniform_expr.json')
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p

    class Row(ctypes.Structure):
        _fields_ = [('values', ctypes.c_void_p), ('n_values', ctypes.c_uint32),
                    ('min_value', ctypes.c_float), ('max_value', ctypes.c_float)]

    class Desc(ctypes.Structure):
        _fields_ = [('dim', ctypes.c_uint32), ('n_rows', ctypes.c_uint64), ('rows', ctypes.c_void_p),
                    ('quantization_levels', ctypes.c_uint8)]

    for levels in (0, 1, 2, 16, 255):
        subset = [c for c in cases if c[3] == levels]
        pairs = sorted({(c[0], c[1]) for c in subset})
        values = sorted({c[2] for c in subset})
        values = values + [values[-1]] * (-len(values) % 4)   # whole 8-byte output pieces: the vector kernels
        payload = np.array(values, dtype=np.uint8)
        rows = (Row * len(pairs))()
        for i, (low, high) in enumerate(pairs):
            rows[i] = Row(payload.ctypes.data, len(values), np.uint32(low).view(np.float32), np.uint32(high).view(np.float32))
        desc = Desc(len(values), len(pairs), ctypes.addressof(rows), levels)
        context = ctypes.c_void_p()
        assert library.memb_hip_ctx_create_uniform(ctypes.byref(context), 0, ctypes.byref(desc)) == 0, library.memb_hip_last_error()
        expected32 = np.empty((len(pairs), len(values)), dtype=np.uint32)
        lookup = {(c[0], c[1], c[2]): c[4] for c in subset}
        for i, (low, high) in enumerate(pairs):
            for j, value in enumerate(values):
                expected32[i, j] = lookup[(low, high, value)]
        ids = torch.arange(len(pairs), dtype=torch.int32, device='cuda')
        for dtype, code in ((torch.bfloat16, 1), (torch.float16, 2)):
            out = torch.empty((len(pairs), len(values)), dtype=dtype, device='cuda')
            status = library.memb_hip_decode_rows_device_typed(
                context, ctypes.c_void_p(ids.data_ptr()), ctypes.c_size_t(len(pairs)), ctypes.c_void_p(out.data_ptr()),
                code, ctypes.c_size_t(len(values)), ctypes.c_size_t(0), None)
            assert status == 0, library.memb_hip_last_error()
            torch.cuda.synchronize()
            assert_narrow_equal(out, torch.from_numpy(expected32.view(np.float32)).to(dtype), (levels, dtype))
        library.memb_hip_ctx_destroy(context)


def test_values_beyond_the_fp16_range_and_subnormals(native, tmp_path):
    # overflow to +-inf in fp16, fp16 subnormals and zeros below 2^-24, bf16 subnormals from fp32 subnormals, signed zeros
    import torch
    rng = np.random.default_rng(3)
    special = np.array([1e5, -1e5, 65504.0, 65520.0, -65520.0, 3e38, -3e38, 2.0 ** -24, 2.0 ** -25, 3.0 * 2.0 ** -26,
                        -2.0 ** -30, 1e-40, -1e-40, 1.5e-39, -0.0, 0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9], dtype=np.float32)
    words = ['w%03d' % i for i in range(64)]
    for storage, bits in (('full', 8), ('trained', 4), ('trained', 8), ('uniform', 8)):
        vectors = rng.choice(special, size=(64, 24)).astype(np.float32)
        if storage == 'uniform':
            vectors = (rng.standard_normal((64, 24)) * rng.choice([1e-41, 1e-6, 7e4, 1e37], size=(64, 1))).astype(np.float32)
        path = str(tmp_path / 'edges_{}_{}.bin'.format(storage, bits))
        builder = native.Builder(24, storage, bits)
        builder.add_words(words, vectors)
        builder.save(path)
        reader, checker = native.Reader(path), oracle.OracleReader(path)
        rows = batch_of(300, 64, bits)
        for dtype in narrow_types():
            assert_narrow_equal(decode(reader, rows, dtype), expected_rows(checker, rows, dtype), (storage, bits, dtype))
    # the NaNs and infinities of a full model stay where they are
    nan_words = ['a', 'b']
    nan_vectors = np.array([[np.nan, np.inf, -np.inf, 1.0], [-np.nan, 0.5, -0.0, 7e4]], dtype=np.float32)
    path = str(tmp_path / 'nan.bin')
    builder = native.Builder(4, 'full', 8)
    builder.add_words(nan_words, nan_vectors)
    builder.save(path)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = np.array([0, 1, 0xFFFFFFFF, 1, 0], dtype=np.uint32)
    for dtype in narrow_types():
        out = decode(reader, rows, dtype)
        assert_narrow_equal(out, expected_rows(checker, rows, dtype), dtype)
        assert bool(torch.isnan(out[0, 0])) and bool(torch.isnan(out[1, 0]))


# ---- strided output: columns [col_off, col_off + dim) of a wider tensor, nothing else touched ----

@pytest.mark.parametrize('storage,bits,dim', [('trained', 4, 300), ('trained', 8, 300), ('trained', 4, 7), ('trained', 6, 8),
                                              ('uniform', 8, 300), ('uniform', 8, 5), ('full', 8, 12)])
@pytest.mark.parametrize('col_off,extra', [(0, 0), (1, 0), (3, 2), (4, 4), (8, 1), (5, 7)])
def test_strided_output_keeps_the_sentinel(native, make_model, storage, bits, dim, col_off, extra):
    import torch
    path, _ = make_model(1000, dim, storage, bits)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_of(777, 1000, col_off + extra)
    width = col_off + dim + extra
    for dtype in narrow_types():
        wide = torch.full((len(rows), width), SENTINEL, dtype=torch.int16, device='cuda').view(dtype)
        out = decode(reader, rows, dtype, out=wide, col_off=col_off)
        assert out is wide
        assert_narrow_equal(wide[:, col_off:col_off + dim], expected_rows(checker, rows, dtype), (col_off, extra, dtype))
        bits_view = wide.view(torch.int16)
        assert bool((bits_view[:, :col_off] == SENTINEL).all()) and bool((bits_view[:, col_off + dim:] == SENTINEL).all())


def test_a_two_byte_aligned_slice(native, make_model):
    # out starting one element into a buffer (2-byte but not 4-byte aligned), rows of an odd stride
    import torch
    path, _ = make_model(1000, 300, 'trained', 4)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = batch_of(513, 1000, 5)
    for dtype in narrow_types():
        buffer = torch.full((len(rows) * 303 + 2,), SENTINEL, dtype=torch.int16, device='cuda').view(dtype)
        view = buffer[1:1 + len(rows) * 303].view(len(rows), 303)
        assert view.data_ptr() % 4 == 2
        decode(reader, rows, dtype, out=view, col_off=2)
        assert_narrow_equal(view[:, 2:302], expected_rows(checker, rows, dtype), dtype)
        bits_view = buffer.view(torch.int16)
        assert int(bits_view[0]) == SENTINEL and int(bits_view[-1]) == SENTINEL
        assert bool((view.view(torch.int16)[:, :2] == SENTINEL).all()) and bool((view.view(torch.int16)[:, 302:] == SENTINEL).all())


# ---- refusals, order hint, word API, graphs ----

def test_refusals_launch_nothing(native, make_model):
    import torch
    from memb_amd import _memb
    path, _ = make_model(1000, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = torch.arange(10, dtype=torch.int32, device='cuda')
    out = torch.full((10, 300), SENTINEL, dtype=torch.int16, device='cuda').view(torch.bfloat16)
    with pytest.raises(ValueError):
        reader.rows_embedding_device(rows, out=out, accumulate=True)
    with pytest.raises(ValueError):
        reader.rows_embedding_device(rows, out=out, divisor=2.0)
    with pytest.raises(ValueError):
        reader.rows_embedding_device(rows, dtype=torch.float16, accumulate=True)
    with pytest.raises(TypeError):
        reader.rows_embedding_device(rows, out=out, dtype=torch.float16)
    with pytest.raises(TypeError):
        reader.rows_embedding_device(rows, out=out, dtype=torch.float32)
    with pytest.raises(TypeError):
        reader.rows_embedding_device(rows, dtype=torch.float64)
    with pytest.raises(TypeError):
        reader.rows_embedding_device(rows, out=torch.zeros((10, 300), dtype=torch.float64, device='cuda'))
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all())
    # the C entry: misaligned out, ld too small, unknown type -- MEMB_HIP_ERR_INVALID with a message
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    assert library.memb_hip_decode_rows_device_typed(None, None, ctypes.c_size_t(0), None, 1, ctypes.c_size_t(300),
                                                     ctypes.c_size_t(0), None) == 1
    assert b'null' in library.memb_hip_last_error()
    with pytest.raises(RuntimeError):
        reader._impl.rows_to_device_typed(rows.data_ptr(), 10, out.data_ptr() + 1, 1, 300, 0, 0)
    with pytest.raises(RuntimeError):
        reader._impl.rows_to_device_typed(rows.data_ptr(), 10, out.data_ptr(), 1, 299, 0, 0)
    with pytest.raises(RuntimeError):
        reader._impl.rows_to_device_typed(rows.data_ptr(), 10, out.data_ptr(), 7, 300, 0, 0)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all())
    # fp32 through the typed entry: the same bits as the plain call
    fp32 = torch.empty((10, 300), dtype=torch.float32, device='cuda')
    reader._impl.rows_to_device_typed(rows.data_ptr(), 10, fp32.data_ptr(), _memb.OUT_F32, 300, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(fp32.view(torch.int32), reader.rows_embedding_device(rows).view(torch.int32))


def test_a_narrow_batch_leaves_the_order_word_alone(native, make_model):
    import torch
    count = 530000
    path, _ = make_model(count, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = torch.arange(count, dtype=torch.int32, device='cuda')
    reader.rows_embedding_device(rows)
    torch.cuda.synchronize()
    before = reader.info(600000)['waves_per_block']
    shuffled = rows[torch.randperm(count, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))]
    reader.rows_embedding_device(shuffled, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert reader.info(600000)['waves_per_block'] == before


def test_words_and_tokenizer_in_bf16(native, make_model):
    import torch
    path, words = make_model(5000, 300, 'trained', 4)
    reader = native.Reader(path)
    batch = words[::3] + ['not a word', ''] + words[:100]
    for dtype in narrow_types():
        got = reader.batch_embedding_device(batch, dtype=dtype)
        assert got.dtype == dtype
        assert torch.equal(got.view(torch.int16), reader.batch_embedding_device(batch).to(dtype).view(torch.int16))

    class Tokenizer:
        word_index = {word: index + 1 for index, word in enumerate(words[:50])}
        num_words = None

    weights = reader.tokenizer_embedding_device(Tokenizer(), dtype=torch.bfloat16)
    assert torch.equal(weights.view(torch.int16), reader.tokenizer_embedding_device(Tokenizer()).to(torch.bfloat16).view(torch.int16))


def test_captured_into_a_graph(native, make_model):
    import torch
    path, _ = make_model(5000, 300, 'trained', 4)
    reader, checker = native.Reader(path), oracle.OracleReader(path)
    rows = torch.from_numpy(batch_of(4096, 5000, 9).view(np.int32)).cuda()
    out = torch.empty((4096, 300), dtype=torch.bfloat16, device='cuda')
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        reader.rows_embedding_device(rows, out=out)   # (warm-up: stages the model, configures the kernel)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        reader.rows_embedding_device(rows, out=out)
    out.zero_()
    rows.copy_(torch.from_numpy(batch_of(4096, 5000, 10).view(np.int32)).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert_narrow_equal(out, expected_rows(checker, rows.cpu().numpy().view(np.uint32), torch.bfloat16))
