"""Pooled lookups straight into bf16 / fp16 tensors (memb_hip_pooled_narrow.hip: pool_trained_narrow, pool_uniform_narrow,
pool_full_narrow; hip_pooled_launch.h: launchPooled with a narrow outType).

The contract (include/memb_hip_pooled.h): a narrow value is the float32 pooled value rounded ONCE to nearest even. Two
oracles, which must agree with each other before the device is asked:
  (a) the reader's own float32 bags_embedding_device result (pinned by test_gpu_pooled.py), .cpu().to(dtype)
  (b) the contract's explicit float32 loop over rows_embedding_device(rows) (pooled_reference.pooled_by_the_contract),
      then the same cast
Compared as 16-bit patterns (narrow_bits): the tolerance is zero."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import (KEY_FORM_CASES, for_every_key_form, into_a_frame, narrow_bits, run_on_two_streams, set_environment,
                           sweep_options, to_device)
from pooled_reference import ids_with_misses, offsets_of, pooled_by_the_contract

pytestmark = pytest.mark.gpu

SENTINEL = -1536.0   # exact in bf16 and fp16
N_ROWS = 3000
MODES = ('sum', 'mean')


def narrow_dtypes():
    import torch
    return (torch.bfloat16, torch.float16)


def expected(reader, rows, offsets):
    """{mode: float32 CPU tensor}: oracle (a), checked bit for bit against oracle (b)"""
    import torch
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    values = reader.rows_embedding_device(device_rows).cpu().numpy() if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)
    want = {}
    for mode in MODES:
        want[mode] = reader.bags_embedding_device(device_rows, device_offsets, mode=mode).cpu()
        assert bits_equal(want[mode].numpy(), pooled_by_the_contract(values, offsets, mode)), mode
    torch.cuda.synchronize()
    return want


def check_narrow(reader, rows, offsets, context, want=None, col_off=0, spare=0, shifted=False):
    """Both dtypes and both modes against the oracles; the columns around the bags keep their sentinel. shifted: `out` is
    a view that starts one element into a larger buffer (2-byte aligned only). Returns {(mode, dtype): CPU tensor}."""
    dim = reader.dim
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    want = want or expected(reader, rows, offsets)
    bags = len(offsets) - 1
    results = {}
    for mode in MODES:
        for dtype in narrow_dtypes():
            got = into_a_frame(
                lambda out: reader.bags_embedding_device(device_rows, device_offsets, mode=mode, out=out, col_off=col_off, dtype=dtype),
                bags, dim, (context, mode, dtype), col_off, spare, dtype, SENTINEL, shifted)
            same = narrow_bits(got) == narrow_bits(want[mode].to(dtype))
            if not same.all():
                bad = np.nonzero(~same.all(axis=1))[0]
                raise AssertionError('{} {} {}: {} of {} bags differ, first {}'.format(context, mode, dtype, len(bad), bags, bad[:8]))
            results[mode, dtype] = got
    return results


# ---- 1. bag shapes, per storage ----

@pytest.mark.parametrize('storage,bits_per_value', [('trained', 2), ('trained', 4), ('trained', 6), ('trained', 8), ('uniform', 8), ('full', 8)])
def test_bag_shapes(native, make_model, storage, bits_per_value):
    import torch
    path, _ = make_model(N_ROWS, 300, storage, bits_per_value, distribution='student' if bits_per_value == 8 else 'normal')
    reader = native.Reader(path)
    rng = np.random.default_rng(bits_per_value)
    context = (storage, bits_per_value)
    # all bags of one entry: the narrow rows themselves, -0.0 and missing rows included
    rows = ids_with_misses(1001, N_ROWS, 1)
    ones = check_narrow(reader, rows, np.arange(len(rows) + 1), context + ('ones',))
    for dtype in narrow_dtypes():
        decoded = reader.rows_embedding_device(to_device(rows), dtype=dtype).cpu()
        for mode in MODES:
            assert (narrow_bits(ones[mode, dtype]) == narrow_bits(decoded)).all(), (context, mode, dtype)
    # empty bags at the start, in the middle and at the end
    lengths = [0, 0, 0, 5, 1, 0, 12, 0, 0, 3, 64, 0, 9, 0, 0]
    empties = check_narrow(reader, ids_with_misses(sum(lengths), N_ROWS, 2), offsets_of(lengths), context + ('empties',))
    for result in empties.values():
        assert not narrow_bits(result[[0, 1, 2, 5, 7, 8, 11, 13, 14]]).any()   # +0.0
    # fixed lengths that straddle the 8-word tile
    for length in (7, 8, 9, 17):
        count = 2000 // length
        check_narrow(reader, ids_with_misses(length * count, N_ROWS, length), np.arange(0, length * count + 1, length),
                     context + ('fixed', length))
    # seeded geometric lengths
    for mean_length in (3, 16):
        lengths = rng.geometric(1.0 / mean_length, size=400) - (rng.random(400) < 0.05)
        check_narrow(reader, ids_with_misses(int(lengths.sum()), N_ROWS, mean_length), offsets_of(lengths),
                     context + ('geometric', mean_length))
    # one long bag among small ones
    check_narrow(reader, ids_with_misses(5020, N_ROWS, 6), offsets_of([3, 0, 7, 5000, 1, 9]), context + ('long bag among small',))
    # every entry a missing row
    missing = check_narrow(reader, np.array([0xFFFFFFFF, N_ROWS, N_ROWS + 5, 0xFFFFFFFF, 0xFFFFFFFE], dtype=np.uint32), [0, 2, 5],
                           context + ('all missing',))
    for result in missing.values():
        assert not narrow_bits(result).any()
    for dtype in narrow_dtypes():
        # bags = 0: nothing is launched, an empty result
        empty = reader.bags_embedding_device(to_device(rows), to_device([len(rows)]), dtype=dtype)
        assert tuple(empty.shape) == (0, 300) and empty.dtype == dtype
    # n = 0: +0.0 for every bag
    zero = check_narrow(reader, np.zeros(0, dtype=np.uint32), [0, 0, 0, 0], context + ('n = 0',))
    for result in zero.values():
        assert tuple(result.shape) == (3, 300) and not narrow_bits(result).any()
    torch.cuda.synchronize()


# ---- 2. geometries ----

@pytest.mark.parametrize('dim', [300, 64, 512, 516, 302, 1030, 7, 3, 1])
@pytest.mark.parametrize('storage,bits_per_value', [('trained', 4), ('trained', 6), ('uniform', 8), ('full', 8)])
def test_dims_and_strided_outputs(native, make_model, storage, bits_per_value, dim):
    # multiples of 4 (8-byte pieces: one and two per lane), past the piece form (516), = 2 mod 4, odd and below 4; 516 and
    # 1030 are more than one block of 512 columns in the column form. Bags of mean length 9 span tiles there too. Dense, and
    # ld > dim with col_off > 0 (aligned to a piece and not) between guard columns; and an `out` one element into a buffer.
    path, _ = make_model(700, dim, storage, bits_per_value, seed=dim)
    reader = native.Reader(path)
    lengths = np.random.default_rng(dim).geometric(1 / 9.0, size=300)
    rows = ids_with_misses(int(lengths.sum()), 700, dim)
    offsets = offsets_of(lengths)
    want = expected(reader, rows, offsets)
    for col_off, spare in ((0, 0), (4, 4), (2, 1), (1, 2)):
        check_narrow(reader, rows, offsets, (storage, bits_per_value, dim, col_off, spare), want=want, col_off=col_off, spare=spare)
    check_narrow(reader, rows, offsets, (storage, bits_per_value, dim, 'shifted'), want=want, shifted=True)
    check_narrow(reader, rows, offsets, (storage, bits_per_value, dim, 'shifted', 3, 1), want=want, col_off=3, spare=1, shifted=True)


# ---- 3. the order of rounding ----

ROUNDING_ROWS = {
    'one': 1.0, 'bf_half': 2.0 ** -8, 'bf_quarter': 2.0 ** -9, 'bf_odd': 1 + 2.0 ** -7,
    'h_half': 2.0 ** -11, 'h_quarter': 2.0 ** -12, 'h_odd': 1 + 2.0 ** -10,
    'big': 40000.0, 'minus_big': -40000.0, 'tiny': 2.0 ** -20, 'minus_zero': -0.0, 'tenth': 0.1, 'seven': 7.0,
}
# (bag, mode, {dtype name: the bits of every column}); None: whatever the oracle says
ROUNDING_BAGS = [
    # 1 + 2^-7 exactly: accumulating in bf16, or narrowing per entry, gives 1.0 (0x3F80)
    (['one', 'bf_half', 'bf_half'], 'sum', {'bfloat16': 0x3F81}),
    # 1 + 2^-8: a bf16 tie, to even = 1.0
    (['one', 'bf_quarter', 'bf_quarter'], 'sum', {'bfloat16': 0x3F80}),
    # 1 + 2^-7 + 2^-8: a tie that rounds up, to 1 + 2^-6
    (['bf_odd', 'bf_quarter', 'bf_quarter'], 'sum', {'bfloat16': 0x3F82}),
    # the same three one fp16 ulp (2^-10) up
    (['one', 'h_half', 'h_half'], 'sum', {'float16': 0x3C01}),
    (['one', 'h_quarter', 'h_quarter'], 'sum', {'float16': 0x3C00}),
    (['h_odd', 'h_quarter', 'h_quarter'], 'sum', {'float16': 0x3C02}),
    # means whose float32 quotient is inexact
    (['one', 'tenth', 'bf_half'], 'mean', {}),
    (['seven', 'one', 'one'], 'mean', {}),
    (['one', 'bf_half', 'bf_half'], 'mean', {}),
    # beyond the fp16 range: +-inf; bf16 keeps 80000 (1.220703125 * 2^16 -> 0x479C)
    (['big', 'big'], 'sum', {'float16': 0x7C00, 'bfloat16': 0x479C}),
    (['minus_big', 'minus_big'], 'sum', {'float16': 0xFC00, 'bfloat16': 0xC79C}),
    # 2^-19: subnormal in fp16 (32 units of 2^-24), normal in bf16
    (['tiny', 'tiny'], 'sum', {'float16': 0x0020, 'bfloat16': 0x3600}),
    # a lone -0.0 keeps its sign; with +0.0 from a missing row it does not
    (['minus_zero'], 'sum', {'float16': 0x8000, 'bfloat16': 0x8000}),
    (['minus_zero'], 'mean', {'float16': 0x8000, 'bfloat16': 0x8000}),
    (['minus_zero', None], 'sum', {'float16': 0x0000, 'bfloat16': 0x0000}),
]


def test_the_value_is_rounded_once(native, tmp_path):
    import torch
    dim = 8
    names = sorted(ROUNDING_ROWS)
    vectors = np.repeat(np.array([ROUNDING_ROWS[name] for name in names], dtype=np.float32)[:, None], dim, axis=1)
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(names, vectors)
    path = str(tmp_path / 'rounding.bin')
    builder.save(path)
    reader = native.Reader(path)
    row_of = dict(zip(names, reader.resolve_rows(names)))
    rows = np.array([row_of[name] if name else 0xFFFFFFFF for bag, _, _ in ROUNDING_BAGS for name in bag], dtype=np.uint32)
    offsets = offsets_of([len(bag) for bag, _, _ in ROUNDING_BAGS])
    want = expected(reader, rows, offsets)
    for col_off, shifted in ((0, False), (1, False), (0, True)):   # 8-byte pieces, and single elements
        results = check_narrow(reader, rows, offsets, ('rounding', col_off, shifted), want=want, col_off=col_off, shifted=shifted)
        for index, (bag, mode, pinned) in enumerate(ROUNDING_BAGS):
            for dtype in narrow_dtypes():
                name = str(dtype).split('.')[1]
                if name in pinned:
                    value = np.uint16(pinned[name])
                    # the oracle says so, and the device (check_narrow: equal to the oracle) with it
                    assert (narrow_bits(want[mode][index].to(dtype)) == value).all(), (bag, mode, name, 'oracle')
                    assert (narrow_bits(results[mode, dtype][index]) == value).all(), (bag, mode, name)
    # the traps are traps: per-entry narrowing gives other bits for the first bag
    stepwise = torch.tensor(1.0, dtype=torch.bfloat16)
    for _ in range(2):
        stepwise = (stepwise.float() + 2.0 ** -8).to(torch.bfloat16)
    assert int(narrow_bits(stepwise.reshape(1))[0]) == 0x3F80


# ---- 4. launch geometry and key forms never change a result ----

@pytest.mark.parametrize('bits_per_value', [4, 6])
def test_results_do_not_depend_on_options(native, make_model, bits_per_value):
    path, _ = make_model(N_ROWS, 300, 'trained', bits_per_value)
    reader = native.Reader(path)
    lengths = np.random.default_rng(bits_per_value).geometric(1 / 16.0, size=500)
    rows, offsets = ids_with_misses(int(lengths.sum()), N_ROWS, 3), offsets_of(lengths)
    want = expected(reader, rows, offsets)

    def run(waves, tiles):
        check_narrow(reader, rows, offsets, (bits_per_value, waves, tiles), want=want)
        check_narrow(reader, rows, offsets, (bits_per_value, waves, tiles, 'columns'), want=want, col_off=1, spare=1)

    sweep_options(reader, run, ((1, 1), (2, 64), (4, 2), (7, 5), (8, 1)))


def test_key_forms_tables_and_row_layouts(native, make_model, monkeypatch):
    lengths = np.random.default_rng(1).geometric(1 / 12.0, size=300)
    rows, offsets = ids_with_misses(int(lengths.sum()), N_ROWS, 9), offsets_of(lengths)
    models = [(4, 'normal'), (6, 'student')]
    set_environment(monkeypatch)
    want = {bits_per_value: expected(native.Reader(make_model(N_ROWS, 300, 'trained', bits_per_value, distribution=distribution)[0]),
                                     rows, offsets)
            for bits_per_value, distribution in models}

    def check(reader, context):
        check_narrow(reader, rows, offsets, context, want=want[context[0]])
        check_narrow(reader, rows, offsets, context + ('columns',), want=want[context[0]], col_off=1, spare=1)

    # (seven of the ten cases: what the key forms themselves do is pinned in fp32, by test_gpu_pooled.py)
    cases = [case for case in KEY_FORM_CASES
             if case not in (({}, 0), ({'MEMB_HIP_LANES': 1, 'MEMB_HIP_WAVES': 1}, 0), ({'MEMB_HIP_LANES': 5, 'MEMB_HIP_WAVES': 8}, 1))]
    for_every_key_form(native, make_model, monkeypatch, N_ROWS, check, models, cases, all_forms=False)


# ---- 5. two callers at once ----

def test_two_threads_on_two_streams(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    jobs = []
    for thread, dtype in enumerate(narrow_dtypes()):
        lengths = np.random.default_rng(thread).geometric(1 / 16.0, size=2000)
        rows, offsets = ids_with_misses(int(lengths.sum()), N_ROWS, thread), offsets_of(lengths)
        want = expected(reader, rows, offsets)
        jobs.append((to_device(rows), to_device(offsets), dtype, {mode: narrow_bits(want[mode].to(dtype)) for mode in MODES}))

    def call(thread, repeat):
        device_rows, device_offsets, dtype, want = jobs[thread]
        mode = MODES[repeat % 2]
        got = reader.bags_embedding_device(device_rows, device_offsets, mode=mode, dtype=dtype)
        return (got,), (want[mode],), mode

    run_on_two_streams(jobs, call, repeats=10)


# ---- 6. the Python surface ----

def test_python_entry_points_and_their_errors(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    vocabulary = sorted(words)
    sentences = [vocabulary[:5], [], ['not-in-the-model'], vocabulary[100:117] + ['nor-this'], [vocabulary[7]]]
    rows = reader.resolve_rows([word for sentence in sentences for word in sentence])
    offsets = offsets_of([len(sentence) for sentence in sentences])
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    for mode in MODES:
        fp32 = reader.sentences_embedding_device(sentences, mode=mode)
        assert fp32.dtype == torch.float32
        assert bits_equal(reader.bags_embedding_device(device_rows, device_offsets, mode=mode, dtype=torch.float32).cpu().numpy(),
                          fp32.cpu().numpy())
        for dtype in narrow_dtypes():
            got = reader.sentences_embedding_device(sentences, mode=mode, dtype=dtype)
            assert got.dtype == dtype and tuple(got.shape) == (5, 300)
            assert (narrow_bits(got.cpu()) == narrow_bits(fp32.cpu().to(dtype))).all(), (mode, dtype)
    for dtype in narrow_dtypes():
        assert reader.sentences_embedding_device([], dtype=dtype).dtype == dtype
        out = torch.empty((5, 300), dtype=dtype, device='cuda')
        returned = reader.bags_embedding_device(device_rows, device_offsets, out=out, dtype=dtype)
        assert returned.data_ptr() == out.data_ptr() and returned.dtype == dtype
        with pytest.raises(TypeError):   # out / dtype mismatch, either way
            reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((5, 300), device='cuda'), dtype=dtype)
        with pytest.raises(TypeError):
            reader.bags_embedding_device(device_rows, device_offsets, out=out, dtype=torch.float32)
        with pytest.raises(TypeError, match='float32'):   # a narrow result is asked for by name
            reader.bags_embedding_device(device_rows, device_offsets, out=out)
        with pytest.raises(ValueError):
            reader.bags_embedding_device(device_rows, device_offsets, mode='max', dtype=dtype)
        with pytest.raises(ValueError):
            reader.sentences_embedding_device(sentences, mode='max', dtype=dtype)
        with pytest.raises(TypeError):
            reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((4, 300), dtype=dtype, device='cuda'), dtype=dtype)
        with pytest.raises(ValueError):
            reader.bags_embedding_device(device_rows, device_offsets, out=out, col_off=4, dtype=dtype)
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows, device_offsets, dtype=torch.float64)
    with pytest.raises(TypeError):
        reader.bags_embedding_device(device_rows, device_offsets, out=torch.empty((5, 300), dtype=torch.float64, device='cuda'),
                                     dtype=torch.float64)
    host_reader = native.Reader(path, device='cpu')
    with pytest.raises(RuntimeError, match='host'):
        host_reader.bags_embedding_device(device_rows, device_offsets, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='host'):
        host_reader.sentences_embedding_device(sentences, dtype=torch.float16)
    assert reader.bags_embedding(rows, offsets).dtype == np.float32   # the numpy entry point stays float32


def test_typed_algorithmic_bytes(native, make_model):
    # test_gpu_pooled.test_pooled_algorithmic_bytes with two bytes per stored element
    from memb_amd import _memb
    rows = np.array([0, 5, 0xFFFFFFFF, 9, 700, 3, 3, 8], dtype=np.uint32)
    offsets = np.array([0, 2, 2, 7, 9], dtype=np.uint32)
    present_in_bags = 6
    for storage, per_row in (('uniform', 12 + 300), ('full', 4 + 4 * 300)):
        path, _ = make_model(700, 300, storage, 8)
        reader = native.Reader(path)
        reader.info()   # (stages the model)
        read = 8 * 4 + present_in_bags * per_row
        assert reader._impl.pooled_algorithmic_bytes(rows, offsets, _memb.OUT_F32) == read + 4 * (8 + 4 * 300), storage
        assert reader._impl.pooled_algorithmic_bytes(rows, offsets) == read + 4 * (8 + 4 * 300), storage
        for out_type in (_memb.OUT_BF16, _memb.OUT_F16):
            assert reader._impl.pooled_algorithmic_bytes(rows, offsets, out_type) == read + 4 * (8 + 2 * 300), (storage, out_type)
            assert reader._impl.pooled_algorithmic_bytes(rows, offsets, out_type=out_type) == read + 4 * (8 + 2 * 300)
        with pytest.raises(RuntimeError, match='out_type'):
            reader._impl.pooled_algorithmic_bytes(rows, offsets, 3)
