"""Row norms and unit rows on the GPU (memb_hip_norms.hip: norms_trained, unit_trained, norms_dense, unit_dense;
hip_norms_launch.h).

The oracle everywhere: the contract of include/memb_hip_norms.h in numpy (tests/norms_reference.py) over the reader's own
fp32 rows from reader.rows_embedding. Compared bit for bit: the tolerance is zero, whichever kernel ran."""
import numpy as np
import pytest

from conftest import bits_equal
from norms_reference import check_special_rows, ids_with_misses, special_model, unit_rows_by_the_contract
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, into_a_frame, kernel_form, same_bits, to_device

pytestmark = pytest.mark.gpu

N_ROWS = 3000
KEY_FORM_ROWS = 20000   # the models of tests/test_gpu_pooled.py (built once per session): at 3000 rows the 4-bit model has
                        # a 9-bit code and never takes nibble keys
SENTINEL = np.float32(-1234.5)


def words_per_wave(reader):
    """rows a wavefront of the trained kernels decodes at a time; uniform and full storage: the rows of a block of the dense
    kernels, one per wavefront"""
    lanes = reader.info()['lanes_per_word']
    return 64 // lanes if lanes else 4


def check_norms(reader, rows, context, kernels, col_off=0, spare=0):
    """row_norms_device and unit_rows_embedding_device, with and without return_norms, against the contract; what lies
    around the norms and around the unit rows' columns keeps its sentinel; last_norms_kernel is kernels = (norms, unit)."""
    import torch
    rows = np.asarray(rows, dtype=np.uint32)
    n, dim = len(rows), reader.dim
    values = reader.rows_embedding(rows) if n else np.zeros((0, dim), dtype=np.float32)
    want_unit, want_norms = unit_rows_by_the_contract(values)
    device_rows = to_device(rows)

    norms = reader.row_norms_device(device_rows)
    assert norms.dtype == torch.float32 and tuple(norms.shape) == (n,) and norms.is_cuda, context
    assert same_bits(norms, want_norms), (context, 'norms')
    assert reader.last_norms_kernel == kernels[0], (context, reader.last_norms_kernel)
    # into a caller's tensor between two sentinels
    buffer = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
    returned = reader.row_norms_device(device_rows, out=buffer[1:n + 1])
    assert returned.data_ptr() == buffer[1:n + 1].data_ptr(), context
    host = buffer.cpu().numpy()
    assert host[0] == SENTINEL and host[-1] == SENTINEL and bits_equal(host[1:n + 1], want_norms), (context, 'norms out')

    got = into_a_frame(lambda out: reader.unit_rows_embedding_device(device_rows, out=out, col_off=col_off),
                       n, dim, context, col_off, spare, sentinel=SENTINEL).numpy()
    assert reader.last_norms_kernel == kernels[1], (context, reader.last_norms_kernel)
    if not bits_equal(got, want_unit):
        bad = np.nonzero((got.view(np.uint32) != want_unit.view(np.uint32)).any(axis=1))[0]
        raise AssertionError('{}: {} of {} unit rows differ, first {}'.format(context, len(bad), n, bad[:8]))
    with_norms = []

    def run(out):
        unit, norms = reader.unit_rows_embedding_device(device_rows, out=out, col_off=col_off, return_norms=True)
        with_norms.append(norms)
        return unit

    got = into_a_frame(run, n, dim, context, col_off, spare, sentinel=SENTINEL).numpy()
    assert bits_equal(got, want_unit), (context, 'unit rows beside norms')
    assert with_norms[0].dtype == torch.float32 and tuple(with_norms[0].shape) == (n,), context
    assert same_bits(with_norms[0], want_norms), (context, 'norms beside unit rows')
    return want_norms


def batch_sizes(reader):
    words = words_per_wave(reader)
    return sorted({0, 1, max(words - 1, 1), words, words + 1, 1000})


def check_sizes_and_orders(reader, context, kernels, col_off=0, spare=0):
    for n in batch_sizes(reader):
        check_norms(reader, np.arange(n, dtype=np.uint32) % N_ROWS, (context, 'key order', n), kernels, col_off, spare)
        check_norms(reader, ids_with_misses(n, N_ROWS, n), (context, 'shuffled', n), kernels, col_off, spare)


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        FORMS_REACHED.add(kernel_form(reader))
        norms = check_norms(reader, ids_with_misses(1000, KEY_FORM_ROWS, context[0]), context, ('norms_trained', 'unit_trained'))
        assert (norms > 0).any()
        words = words_per_wave(reader)
        check_norms(reader, np.arange(words + 1, dtype=np.uint32), (context, 'a tile and a word'), ('norms_trained', 'unit_trained'))

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    # (the models and cases above must between them run nibble keys, byte keys and two-level tables)
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


# ---- 2. the fused path ----

@pytest.mark.parametrize('dim', (4, 256, 260, 300, 512))
@pytest.mark.parametrize('bits', (4, 6))
def test_fused_dims(native, make_model, dim, bits):
    path, _ = make_model(N_ROWS, dim, 'trained', bits)
    reader = native.Reader(path)
    check_sizes_and_orders(reader, (dim, bits), ('norms_trained', 'unit_trained'))
    # a wider out whose rows stay aligned to 16 bytes: still the fused kernel
    check_norms(reader, ids_with_misses(333, N_ROWS, 4), (dim, bits, 'wider'), ('norms_trained', 'unit_trained'), col_off=8, spare=4)


def test_launch_options_never_change_a_bit(native, make_model):
    from pooled_device import sweep_options
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(1000, N_ROWS, 12)
    sweep_options(reader, lambda waves, tiles: check_norms(reader, rows, (waves, tiles), ('norms_trained', 'unit_trained')),
                  pairs=[(1, 1), (2, 5), (7, 2), (8, 64)])


# ---- 3. the fallback path: the plain decode and the dense kernels ----

@pytest.mark.parametrize('storage,bits,dim', [('trained', 4, 7), ('trained', 6, 516), ('trained', 4, 1028), ('uniform', 8, 300),
                                              ('full', 8, 300), ('uniform', 8, 7), ('full', 8, 1028)])
def test_fallback_models(native, make_model, storage, bits, dim):
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    check_sizes_and_orders(reader, (storage, bits, dim), ('norms_dense', 'unit_dense'))
    check_norms(reader, ids_with_misses(333, N_ROWS, 5), (storage, bits, dim, 'col_off'), ('norms_dense', 'unit_dense'), col_off=1, spare=2)


def test_unaligned_columns_take_the_dense_kernel_in_place(native, make_model):
    # a model the fused kernels take, but unit rows that do not start on 16 bytes: decode, then unit_dense in place
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    check_sizes_and_orders(reader, 'col_off 1', ('norms_trained', 'unit_dense'), col_off=1, spare=3)
    check_norms(reader, ids_with_misses(500, N_ROWS, 6), 'odd ld', ('norms_trained', 'unit_dense'), col_off=0, spare=1)


def test_norms_without_a_fused_kernel_decode_in_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_DEVICE_SLICE', 128)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    check_norms(reader, ids_with_misses(128 * 3 + 17, N_ROWS, 8), 'slices', ('norms_dense', 'unit_dense'))


# ---- 4. words, host arrays, special rows ----

def test_words_and_host_arrays_take_the_rows_path(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    asked = [words[5], 'no such word é', words[0], words[5], words[N_ROWS - 1]] + list(words[100:400])
    rows = reader.resolve_rows(asked)
    assert rows[1] == 0xFFFFFFFF
    want_unit, want_norms = unit_rows_by_the_contract(reader.rows_embedding(rows))
    got = reader.unit_batch_embedding_device(asked)
    assert same_bits(got, want_unit) and not got[1].any()
    assert same_bits(got, reader.unit_rows_embedding_device(to_device(rows)))
    assert bits_equal(reader.row_norms(rows), want_norms) and bits_equal(reader.unit_rows_embedding(rows), want_unit)


def test_subnormal_sums_and_signed_zero_rows(native, tmp_path):
    path, vectors = special_model(native, tmp_path)
    reader = native.Reader(path)
    rows = to_device(np.arange(6, dtype=np.uint32))
    assert same_bits(reader.rows_embedding_device(rows), vectors)
    unit, norms = reader.unit_rows_embedding_device(rows, return_norms=True)
    assert same_bits(reader.row_norms_device(rows), norms)
    check_special_rows(vectors, norms.cpu().numpy(), unit.cpu().numpy())
    # the same rows through the aligned dense form (dim 300 at col_off 0) and the scalar one (col_off 1)
    shifted = reader.unit_rows_embedding_device(rows, col_off=1)
    assert same_bits(shifted[:, 1:], unit)


def test_dense_entry_points_any_dim_and_in_place(native):
    import torch
    from memb_amd import _memb
    rng = np.random.default_rng(11)
    for dim, ld, shift in ((1, 1, 0), (3, 5, 0), (256, 256, 0), (257, 260, 1), (1028, 1028, 0), (2049, 2051, 1)):
        n = 37
        values = (rng.standard_normal((n, ld)) * 3).astype(np.float32)
        want_unit, want_norms = unit_rows_by_the_contract(values[:, :dim])
        buffer = torch.zeros((n * ld + 1,), dtype=torch.float32, device='cuda')
        matrix = buffer[shift:shift + n * ld].view(n, ld)
        matrix.copy_(torch.from_numpy(values))
        norms = torch.full((n,), float(SENTINEL), dtype=torch.float32, device='cuda')
        _memb.dense_row_norms_to_device(0, matrix.data_ptr(), n, dim, ld, norms.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert same_bits(norms, want_norms), (dim, ld, shift)
        norms.fill_(float(SENTINEL))
        _memb.dense_unit_rows_to_device(0, matrix.data_ptr(), n, dim, ld, matrix.data_ptr(), ld, 0, norms.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        assert same_bits(norms, want_norms), (dim, ld, shift, 'in place')
        host = matrix.cpu().numpy()
        assert bits_equal(host[:, :dim], want_unit) and bits_equal(host[:, dim:], values[:, dim:]), (dim, ld, shift)


# ---- 5. callers at once ----

def test_two_streams_at_once(native, make_model):
    from pooled_device import run_on_two_streams
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    other, _ = make_model(N_ROWS, 300, 'uniform', 8)
    readers = [native.Reader(path), native.Reader(other)]
    jobs = []
    for thread, reader in enumerate(readers):
        rows = ids_with_misses(1000, N_ROWS, 20 + thread)
        want_unit, want_norms = unit_rows_by_the_contract(reader.rows_embedding(rows))
        jobs.append((reader, to_device(rows), want_unit, want_norms))

    def call(thread, repeat):
        reader, rows, want_unit, want_norms = jobs[thread]
        unit, norms = reader.unit_rows_embedding_device(rows, return_norms=True)
        alone = reader.row_norms_device(rows)
        return (unit, norms, alone), (want_unit, want_norms, want_norms), (thread, repeat)

    run_on_two_streams(jobs, call, repeats=5)


# ---- 6. what Python refuses ----

def test_python_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(10, dtype=np.uint32))
    for call in (reader.row_norms_device, reader.unit_rows_embedding_device):
        with pytest.raises(TypeError, match='rows must be'):
            call(rows.cpu())                                   # wrong device
        with pytest.raises(TypeError, match='rows must be'):
            call(rows.to(torch.int64))                         # wrong dtype
        with pytest.raises(TypeError, match='rows must be'):
            call(to_device(np.arange(20, dtype=np.uint32))[::2])   # not contiguous
    with pytest.raises(ValueError, match='narrower'):
        reader.unit_rows_embedding_device(rows, out=torch.empty((10, 299), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='narrower'):
        reader.unit_rows_embedding_device(rows, out=torch.empty((10, 300), dtype=torch.float32, device='cuda'), col_off=4)
    with pytest.raises(TypeError, match='float32'):
        reader.unit_rows_embedding_device(rows, out=torch.empty((10, 300), dtype=torch.bfloat16, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        reader.unit_rows_embedding_device(rows, out=torch.empty((9, 300), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='must be on cuda'):
        reader.unit_rows_embedding_device(rows, out=torch.empty((10, 300), dtype=torch.float32))
    with pytest.raises(TypeError, match='float32'):
        reader.row_norms_device(rows, out=torch.empty((10,), dtype=torch.float16, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        reader.row_norms_device(rows, out=torch.empty((11,), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='must be on cuda'):
        reader.row_norms_device(rows, out=torch.empty((10,), dtype=torch.float32))
    # nothing was launched by a refused call; the reader still answers
    assert same_bits(reader.row_norms_device(rows), unit_rows_by_the_contract(reader.rows_embedding(np.arange(10, dtype=np.uint32)))[1])
