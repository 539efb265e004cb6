"""Cosine similarity of row pairs on the GPU (memb_hip_pairs.hip: pairs_trained, pairs_dense; hip_pairs_launch.h).

The oracle everywhere: the contract of include/memb_hip_pairs.h in numpy (tests/pairs_reference.py) over the reader's own
fp32 rows from reader.rows_embedding. Compared bit for bit: the tolerance is zero, whichever kernel ran."""
import os

import numpy as np
import pytest

from conftest import bits_equal
from norms_reference import ids_with_misses, special_model
from pairs_reference import pairs_by_the_contract
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, sweep_options, to_device

pytestmark = pytest.mark.gpu

N_ROWS = 3000
KEY_FORM_ROWS = 20000   # the models of tests/test_gpu_pooled.py (built once per session)
SENTINEL = np.float32(-1234.5)


def words_per_wave(reader):
    lanes = reader.info()['lanes_per_word']
    return 64 // lanes if lanes else 4


def fused_kernel(reader):
    """the kernel a reader of a trained model with a fused dim takes: the fused one unless a wavefront holds one word"""
    return 'pairs_trained' if words_per_wave(reader) >= 2 else 'pairs_dense'


def check_pairs(reader, rows_a, rows_b, context, kernel):
    """pair_similarity_device in every output combination and both input forms against the contract; `out` between two
    sentinels; norms[:, 0] is row_norms_device(rows_a); last_pairs_kernel is `kernel`."""
    import torch
    rows_a, rows_b = np.asarray(rows_a, dtype=np.uint32), np.asarray(rows_b, dtype=np.uint32)
    n, dim = len(rows_a), reader.dim
    empty = np.zeros((0, dim), dtype=np.float32)
    want = pairs_by_the_contract(reader.rows_embedding(rows_a) if n else empty, reader.rows_embedding(rows_b) if n else empty)
    a, b = to_device(rows_a), to_device(rows_b)
    both = to_device(np.stack((rows_a, rows_b), axis=1))
    assert tuple(both.shape) == (n, 2)

    cosines = reader.pair_similarity_device(a, b)
    assert cosines.dtype == torch.float32 and tuple(cosines.shape) == (n,) and cosines.is_cuda, context
    assert reader.last_pairs_kernel == kernel, (context, reader.last_pairs_kernel)
    if not same_bits(cosines, want[0]):
        bad = np.nonzero(cosines.cpu().numpy().view(np.uint32) != want[0].view(np.uint32))[0]
        raise AssertionError('{}: {} of {} cosines differ, first {}'.format(context, len(bad), n, bad[:8]))
    assert same_bits(reader.pair_similarity_device(both), want[0]), (context, '(n, 2)')
    # every combination of outputs
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.pair_similarity_device(both, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and same_bits(got[0], want[0]), (context, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms), (context, dots, norms)
        if dots:
            assert tuple(got[1].shape) == (n,) and same_bits(got[1], want[1]), (context, dots, norms, 'dots')
        if norms:
            assert tuple(got[2].shape) == (n, 2) and same_bits(got[2], want[2]), (context, dots, norms, 'norms')
            assert same_bits(got[2][:, 0].contiguous(), reader.row_norms_device(a)), (context, 'row_norms_device')
    # dots alone, norms alone: the C entry point with the other pointers null
    stream = torch.cuda.current_stream().cuda_stream
    if kernel == 'pairs_trained' and n:
        alone = torch.full((2 * n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
        assert reader._impl.pair_similarity_to_device(both.data_ptr(), n, 0, alone[1:n + 1].data_ptr(), 0, stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:n + 1], want[1]) and (host[n + 1:] == SENTINEL).all() and host[0] == SENTINEL, (context, 'dots alone')
        alone.fill_(float(SENTINEL))
        assert reader._impl.pair_similarity_to_device(both.data_ptr(), n, 0, 0, alone[1:2 * n + 1].data_ptr(), stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:2 * n + 1], want[2].reshape(-1)) and host[0] == SENTINEL and host[-1] == SENTINEL, (context, 'norms alone')
    # into a caller's tensor between two sentinels
    buffer = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
    returned = reader.pair_similarity_device(a, b, out=buffer[1:n + 1])
    assert returned.data_ptr() == buffer[1:n + 1].data_ptr(), context
    host = buffer.cpu().numpy()
    assert host[0] == SENTINEL and host[-1] == SENTINEL and bits_equal(host[1:n + 1], want[0]), (context, 'out')
    return want


def pair_counts(reader):
    pairs = max(words_per_wave(reader) // 2, 1)   # P: pairs per tile
    return sorted({0, 1, max(pairs - 1, 1), pairs, pairs + 1, 2 * pairs + 1, 1000})


def check_sizes_and_orders(reader, context, kernel, n_rows=N_ROWS):
    for n in pair_counts(reader):
        in_order = np.arange(2 * n, dtype=np.uint32) % n_rows
        check_pairs(reader, in_order[0::2], in_order[1::2], (context, 'key order', n), kernel)
        check_pairs(reader, ids_with_misses(n, n_rows, n), ids_with_misses(n, n_rows, n + 1), (context, 'shuffled', n), kernel)


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        kernel = fused_kernel(reader)
        if kernel == 'pairs_trained':
            FORMS_REACHED.add(kernel_form(reader))
        else:
            assert context[1].get('MEMB_HIP_LANES') == 64 and reader._impl.pairs_kernel_name() == ''
        want = check_pairs(reader, ids_with_misses(1000, KEY_FORM_ROWS, context[0]), ids_with_misses(1000, KEY_FORM_ROWS, context[0] + 1),
                           context, kernel)
        assert (want[0] != 0).any()
        words = words_per_wave(reader)
        in_order = np.arange(2 * (words + 1), dtype=np.uint32)
        check_pairs(reader, in_order[0::2], in_order[1::2], (context, 'a tile and two words'), kernel)

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    # (the models and cases above must between them run nibble keys, byte keys and two-level tables through pairs_trained)
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


# ---- 2. the fused path ----

@pytest.mark.parametrize('dim', (4, 256, 260, 300, 512))
@pytest.mark.parametrize('bits', (4, 6))
def test_fused_dims(native, make_model, dim, bits):
    path, _ = make_model(N_ROWS, dim, 'trained', bits)
    reader = native.Reader(path)
    assert reader._impl.pairs_kernel_name() == 'pairs_trained'
    check_sizes_and_orders(reader, (dim, bits), 'pairs_trained')


def test_an_odd_number_of_words_per_wavefront(native, make_model, monkeypatch):
    # asked for nine lanes per word, dims 324 .. 360 get 40-symbol segments and nine lanes: seven words per wavefront, tiles
    # of six words (test_every_key_form has 21 words per wavefront among its cases)
    from pooled_device import set_environment
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    words = words_per_wave(reader)
    assert words % 2 == 1 and words == 7, (words, reader.info()['lanes_per_word'])
    check_sizes_and_orders(reader, 'odd words per wavefront', 'pairs_trained')
    rows = ids_with_misses(2 * 777, N_ROWS, 3)
    sweep_options(reader, lambda waves, tiles: check_pairs(reader, rows[0::2], rows[1::2], ('odd', waves, tiles), 'pairs_trained'),
                  pairs=[(1, 1), (7, 2)])


def test_launch_options_never_change_a_bit(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows_a, rows_b = ids_with_misses(1000, N_ROWS, 12), ids_with_misses(1000, N_ROWS, 13)
    sweep_options(reader, lambda waves, tiles: check_pairs(reader, rows_a, rows_b, (waves, tiles), 'pairs_trained'),
                  pairs=[(1, 1), (2, 5), (7, 2), (8, 64)])


# ---- 3. the fallback path: the plain decode and the dense kernel ----

@pytest.mark.parametrize('storage,bits,dim', [('uniform', 8, 300), ('full', 8, 300), ('trained', 4, 7), ('trained', 4, 302),
                                              ('trained', 6, 516)])
def test_fallback_models(native, make_model, storage, bits, dim):
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    assert reader._impl.pairs_kernel_name() == ''
    # the C entry point says MEMB_HIP_UNSUPPORTED (the binding: False) and launches nothing
    import torch
    guard = torch.full((8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    assert reader._impl.pair_similarity_to_device(to_device(np.arange(8)).data_ptr(), 4, guard.data_ptr(), 0, 0, 0) is False
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    check_sizes_and_orders(reader, (storage, bits, dim), 'pairs_dense')


def test_pairs_without_a_fused_kernel_decode_in_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_DEVICE_SLICE', 64)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    n = 32 * 3 + 17
    check_pairs(reader, ids_with_misses(n, N_ROWS, 8), ids_with_misses(n, N_ROWS, 9), 'slices', 'pairs_dense')


def test_dense_entry_point_any_dim_ld_and_alignment(native):
    import torch
    from memb_amd import _memb
    rng = np.random.default_rng(11)
    for dim, ld, shift in ((1, 1, 0), (3, 5, 0), (256, 256, 0), (300, 304, 1), (257, 260, 1), (1028, 1028, 0), (2049, 2051, 1)):
        n = 19
        values = (rng.standard_normal((2 * n, ld)) * 3).astype(np.float32)
        values[4] = values[5]
        values[6] = -values[7]
        values[8] = 0
        want = pairs_by_the_contract(values[0::2, :dim], values[1::2, :dim])
        buffer = torch.zeros((2 * n * ld + 4,), dtype=torch.float32, device='cuda')
        assert buffer.data_ptr() % 16 == 0
        matrix = buffer[shift:shift + 2 * n * ld].view(2 * n, ld)   # shift 1: one float past 16-byte alignment
        matrix.copy_(torch.from_numpy(values))
        out = torch.full((4 * n + 3,), float(SENTINEL), dtype=torch.float32, device='cuda')
        _memb.dense_pair_similarity_to_device(0, matrix.data_ptr(), n, dim, ld, out[1:n + 1].data_ptr(), out[n + 1:2 * n + 1].data_ptr(),
                                              out[2 * n + 1:4 * n + 1].data_ptr(), torch.cuda.current_stream().cuda_stream)
        host = out.cpu().numpy()
        assert host[0] == SENTINEL and (host[4 * n + 1:] == SENTINEL).all(), (dim, ld, shift)
        assert bits_equal(host[1:n + 1], want[0]), (dim, ld, shift, 'cosines')
        assert bits_equal(host[n + 1:2 * n + 1], want[1]), (dim, ld, shift, 'dots')
        assert bits_equal(host[2 * n + 1:4 * n + 1], want[2].reshape(-1)), (dim, ld, shift, 'norms')
        assert same_bits(matrix, values)   # the matrix is read only
    assert _memb.dense_pairs_kernel_name() == 'pairs_dense'


# ---- 4. special rows, words, host arrays, the byte count ----

def test_special_rows(native, tmp_path):
    path, vectors = special_model(native, tmp_path)
    reader = native.Reader(path)
    rows_a = np.array([0, 0, 2, 3, 2, 5, 4, 5, 0xFFFFFFFF, 9, 1], dtype=np.uint32)
    rows_b = np.array([0, 1, 3, 3, 2, 5, 5, 77, 0xFFFFFFFF, 0, 5], dtype=np.uint32)
    assert same_bits(reader.rows_embedding_device(to_device(np.arange(6))), vectors)
    cosines, dots, norms = check_pairs(reader, rows_a, rows_b, 'special rows', 'pairs_dense')
    # 300 products of 2^-140 sum to 300 * 2^-140, below the smallest normal float32: a flush would give 0; both norms are
    # below 1e-12, so the cosine is the dot over 1e-12 * 1e-12
    assert dots[0] == np.float32(300 * 2.0 ** -140) and 0 < dots[0] < np.float32(1.1754944e-38)
    assert cosines[0] == dots[0] / (np.float32(1e-12) * np.float32(1e-12)) and cosines[1] == -cosines[0] and cosines[0] > 0
    minus_zero = np.float32(-0.0).tobytes()
    assert dots[2].tobytes() == minus_zero and cosines[2].tobytes() == minus_zero            # +0.0 . -0.0
    assert dots[3].tobytes() == np.float32(0.0).tobytes() and dots[4].tobytes() == np.float32(0.0).tobytes()
    assert abs(float(cosines[5]) - 1) <= 2.0 ** -22 and norms[5, 0] == norms[5, 1]                 # a row with itself
    assert not cosines[7:10].any() and not dots[7:10].any() and not norms[8].any()          # one and two missing ids
    # a row with its negation: a second model that holds -vectors[5]
    negated = np.concatenate([vectors, -vectors[5:6]])
    builder = native.Builder(300, 'full', 8)
    builder.add_words(['t{}'.format(i) for i in range(len(negated))], negated)
    second = os.path.join(str(tmp_path), 'special_negated.bin')
    builder.save(second)
    reader = native.Reader(second)
    cosines, dots, norms = check_pairs(reader, np.array([5, 6, 5], dtype=np.uint32), np.array([6, 5, 5], dtype=np.uint32),
                                       'negation', 'pairs_dense')
    assert cosines[0] == -cosines[2] and cosines[1] == cosines[0] and dots[0] == -dots[2] and norms[0, 0] == norms[0, 1]
    assert abs(float(cosines[0]) + 1) <= 2.0 ** -22


def test_words_and_host_arrays_take_the_rows_path(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    words_a = [words[5], 'no such word é', words[0], words[5], words[N_ROWS - 1]] + list(words[100:400])
    words_b = [words[6], words[7], 'nor this one', words[5], words[0]] + list(words[300:600])
    rows_a, rows_b = reader.resolve_rows(words_a), reader.resolve_rows(words_b)
    assert rows_a[1] == 0xFFFFFFFF and rows_b[2] == 0xFFFFFFFF
    want = pairs_by_the_contract(reader.rows_embedding(rows_a), reader.rows_embedding(rows_b))
    got = reader.similarity_device(words_a, words_b)
    assert same_bits(got, want[0]) and same_bits(got, reader.pair_similarity_device(to_device(rows_a), to_device(rows_b)))
    assert got[1] == 0 and got[2] == 0 and abs(float(got[3]) - 1) <= 2.0 ** -22
    # numpy to numpy on the GPU reader and on a device='cpu' reader: the same bits
    host = native.Reader(path, device='cpu')
    on_gpu = reader.pair_similarity(rows_a, rows_b, return_dots=True, return_norms=True)
    on_cpu = host.pair_similarity(rows_a, rows_b, return_dots=True, return_norms=True)
    assert all(isinstance(part, np.ndarray) for part in on_gpu)
    assert all(bits_equal(one, other) for one, other in zip(on_gpu, on_cpu))
    assert all(bits_equal(one, other) for one, other in zip(on_gpu, want))
    assert bits_equal(reader.pair_similarity(rows_a, rows_b), want[0])


def test_pairs_algorithmic_bytes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    pairs = np.arange(20, dtype=np.uint32).reshape(10, 2) * 7
    pairs[3, 1] = 0xFFFFFFFF
    pairs[8, 0] = N_ROWS + 1
    known = pairs.reshape(-1)[pairs.reshape(-1) < N_ROWS]
    # per entry its id, and for a row of the model its compressed bytes: what the norms' count of that row alone holds
    # beside the id when neither a unit row nor a norm is stored
    read = sum(int(reader._impl.norms_algorithmic_bytes(np.array([row], dtype=np.uint32), False, False)) - 4 for row in known)
    entries = 20 * 4 + read
    assert len(known) == 18 and read > 18 * 8
    count = reader._impl.pairs_algorithmic_bytes
    assert count(pairs) == entries + 10 * 4
    assert count(pairs, True, True, True) == entries + 10 * 16
    assert count(pairs, False, True, False) == entries + 10 * 4
    assert count(pairs, cosines=False, dots=False, norms=True) == entries + 10 * 8
    assert count(np.zeros((0, 2), dtype=np.uint32)) == 0


# ---- 5. other streams ----

def test_another_stream_and_no_allocation(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(2000, N_ROWS, 31)
    want = pairs_by_the_contract(reader.rows_embedding(rows[0::2]), reader.rows_embedding(rows[1::2]))
    both = to_device(rows.reshape(1000, 2))
    out = torch.empty((1000,), dtype=torch.float32, device='cuda')
    reader.pair_similarity_device(both, out=out)   # (warm: the model is staged, the kernel loaded)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out.fill_(float(SENTINEL))
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        returned = reader.pair_similarity_device(both, out=out)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before   # the (n, 2) form with `out`: nothing allocated
        stream.synchronize()
    assert returned.data_ptr() == out.data_ptr() and same_bits(out, want[0]) and reader.last_pairs_kernel == 'pairs_trained'


def test_two_streams_at_once(native, make_model):
    from pooled_device import run_on_two_streams
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    other, _ = make_model(N_ROWS, 300, 'uniform', 8)
    jobs = []
    for thread, reader in enumerate([native.Reader(path), native.Reader(other)]):
        rows = ids_with_misses(2000, N_ROWS, 40 + thread)
        want = pairs_by_the_contract(reader.rows_embedding(rows[0::2]), reader.rows_embedding(rows[1::2]))
        jobs.append((reader, to_device(rows.reshape(1000, 2)), want))

    def call(thread, repeat):
        reader, both, want = jobs[thread]
        return reader.pair_similarity_device(both, return_dots=True, return_norms=True), want, (thread, repeat)

    run_on_two_streams(jobs, call, repeats=5)


# ---- 6. what Python refuses ----

def test_python_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(10, dtype=np.uint32))
    with pytest.raises(TypeError, match='rows must be'):
        reader.pair_similarity_device(rows.cpu(), rows)                    # wrong device
    with pytest.raises(TypeError, match='rows must be'):
        reader.pair_similarity_device(rows, rows.to(torch.int64))          # wrong dtype
    with pytest.raises(TypeError, match='rows must be'):
        reader.pair_similarity_device(to_device(np.arange(20, dtype=np.uint32))[::2], rows)   # not contiguous
    with pytest.raises(TypeError, match=r'\(n, 2\)'):
        reader.pair_similarity_device(rows)                                # one tensor that holds no pairs
    with pytest.raises(TypeError, match='one dtype'):
        reader.pair_similarity_device(rows, rows[:9].contiguous())
    with pytest.raises(TypeError, match='float32'):
        reader.pair_similarity_device(rows, rows, out=torch.empty((10,), dtype=torch.float16, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        reader.pair_similarity_device(rows, rows, out=torch.empty((11,), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='must be on cuda'):
        reader.pair_similarity_device(rows, rows, out=torch.empty((10,), dtype=torch.float32))
    # nothing was launched by a refused call; the reader still answers
    assert (np.abs(reader.pair_similarity_device(rows, rows).cpu().numpy() - 1) <= 2.0 ** -22).all()
