"""Cosine similarity of pairs of bags on the GPU (memb_hip_bag_pairs.hip: bag_pairs_trained; hip_bag_pairs_launch.h).

The oracle everywhere: the contract of include/memb_hip_bag_pairs.h in numpy (tests/bag_pairs_reference.py) over the
reader's own fp32 rows from reader.rows_embedding; the second oracle the two-step path on the same reader,
bags_embedding_device and the dense pair kernel. Compared bit for bit: the tolerance is zero, whichever kernel ran."""
import numpy as np
import pytest

from bag_pairs_reference import SELF_PAIR, bag_pairs_batch, bag_pairs_by_the_contract, entry_values
from conftest import bits_equal
from norms_reference import norms_by_the_contract, special_model
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, sweep_options, to_device
from pooled_reference import ids_with_misses, offsets_of, signed_zero_model

pytestmark = pytest.mark.gpu

N_ROWS = 3000
KEY_FORM_ROWS = 20000   # the models of tests/test_gpu_pooled.py (built once per session)
SENTINEL = np.float32(-1234.5)
FUSED = 'bag_pairs_trained'
DENSE = 'pairs_dense'
MODES = ('sum', 'mean')
POOL_CODE = {'sum': 0, 'mean': 1}   # MEMB_HIP_POOL_SUM, MEMB_HIP_POOL_MEAN


def words_per_wave(reader):
    lanes = reader.info()['lanes_per_word']
    return 64 // lanes if lanes else 4


def check_bag_pairs(reader, rows, offsets, mode, context, kernel, want=None):
    """bag_pair_similarity_device in every output combination against the contract; dots alone and norms alone through the
    raw binding between sentinels; `out` between two sentinels; norms[:, 0] is the norm contract over
    bags_embedding_device(...)[0::2]; the whole result is bags_embedding_device + the dense pair kernel on the same reader;
    last_bag_pairs_kernel is `kernel`. Returns the contract's (cosines, dots, norms)."""
    import torch
    from memb_amd import _memb
    rows = np.asarray(rows, dtype=np.uint32)
    offsets = np.asarray(offsets)
    n, dim = len(offsets) // 2, reader.dim
    if want is None:
        want = bag_pairs_by_the_contract(entry_values(reader, rows), offsets, mode)
    on_device, cut = to_device(rows), to_device(offsets)

    cosines = reader.bag_pair_similarity_device(on_device, cut, mode)
    assert cosines.dtype == torch.float32 and tuple(cosines.shape) == (n,) and cosines.is_cuda, context
    assert reader.last_bag_pairs_kernel == kernel, (context, reader.last_bag_pairs_kernel)
    if not same_bits(cosines, want[0]):
        bad = np.nonzero(cosines.cpu().numpy().view(np.uint32) != want[0].view(np.uint32))[0]
        raise AssertionError('{}: {} of {} cosines differ, first {}'.format(context, len(bad), n, bad[:8]))
    # every combination of outputs
    pooled = reader.bags_embedding_device(on_device, cut, mode=mode)
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.bag_pair_similarity_device(on_device, cut, mode=mode, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and same_bits(got[0], want[0]), (context, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms), (context, dots, norms)
        if dots:
            assert tuple(got[1].shape) == (n,) and same_bits(got[1], want[1]), (context, dots, norms, 'dots')
        if norms:
            assert tuple(got[2].shape) == (n, 2) and same_bits(got[2], want[2]), (context, dots, norms, 'norms')
            assert bits_equal(got[2][:, 0].cpu().numpy(), norms_by_the_contract(pooled[0::2].cpu().numpy())), (context, 'norms of the pooled rows')
    # the second oracle: the pooled rows of this reader through the dense pair kernel
    stream = torch.cuda.current_stream().cuda_stream
    if n:
        second = torch.empty((4 * n,), dtype=torch.float32, device='cuda')
        _memb.dense_pair_similarity_to_device(
            0, pooled.data_ptr(), n, dim, dim, second[:n].data_ptr(), second[n:2 * n].data_ptr(), second[2 * n:].data_ptr(), stream)
        assert same_bits(second[:n], want[0]) and same_bits(second[n:2 * n], want[1]), (context, 'two steps')
        assert same_bits(second[2 * n:], want[2].reshape(-1)), (context, 'two steps, norms')
    # dots alone, norms alone: the C entry point with the other pointers null
    if kernel == FUSED and n:
        alone = torch.full((2 * n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
        arguments = (on_device.data_ptr(), len(rows), cut.data_ptr(), n, POOL_CODE[mode])
        assert reader._impl.bag_pair_similarity_to_device(*arguments, 0, alone[1:n + 1].data_ptr(), 0, stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:n + 1], want[1]) and (host[n + 1:] == SENTINEL).all() and host[0] == SENTINEL, (context, 'dots alone')
        alone.fill_(float(SENTINEL))
        assert reader._impl.bag_pair_similarity_to_device(*arguments, 0, 0, alone[1:2 * n + 1].data_ptr(), stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:2 * n + 1], want[2].reshape(-1)) and host[0] == SENTINEL and host[-1] == SENTINEL, (context, 'norms alone')
    # into a caller's tensor between two sentinels
    buffer = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
    returned = reader.bag_pair_similarity_device(on_device, cut, mode, out=buffer[1:n + 1])
    assert returned.data_ptr() == buffer[1:n + 1].data_ptr(), context
    host = buffer.cpu().numpy()
    assert host[0] == SENTINEL and host[-1] == SENTINEL and bits_equal(host[1:n + 1], want[0]), (context, 'out')
    return want


def check_pair_counts(reader, context, kernel, n_rows=N_ROWS, counts=(0, 1, 2, 3, 200), modes=MODES):
    words = words_per_wave(reader)
    for pairs in counts:
        rows, offsets = bag_pairs_batch(words, pairs, n_rows, 7 + pairs)
        values = entry_values(reader, rows)
        for mode in modes:
            want = check_bag_pairs(reader, rows, offsets, mode, (context, pairs, mode), kernel,
                                   want=bag_pairs_by_the_contract(values, offsets, mode))
            if pairs > SELF_PAIR:
                assert (want[0] != 0).any() and abs(float(want[0][SELF_PAIR]) - 1) <= 2.0 ** -22, (context, pairs, mode)
                assert want[2][SELF_PAIR, 0] == want[2][SELF_PAIR, 1]
            elif pairs:
                assert (want[0] != 0).any(), (context, pairs, mode)


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.bag_pairs_kernel_name() == FUSED, context   # one word per wavefront (MEMB_HIP_LANES=64) included
        FORMS_REACHED.add(kernel_form(reader))
        rows, offsets = bag_pairs_batch(words_per_wave(reader), 60, KEY_FORM_ROWS, context[0])
        values = entry_values(reader, rows)
        for mode in MODES:
            want = check_bag_pairs(reader, rows, offsets, mode, (context, mode), FUSED, want=bag_pairs_by_the_contract(values, offsets, mode))
            assert (want[0] != 0).any()

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    # (the models and cases above must between them run nibble keys, byte keys and two-level tables through the kernel)
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


# ---- 2. the fused path ----

@pytest.mark.parametrize('dim', (4, 256, 260, 300, 512))
@pytest.mark.parametrize('bits', (4, 6))
def test_fused_dims(native, make_model, dim, bits):
    path, _ = make_model(N_ROWS, dim, 'trained', bits)
    reader = native.Reader(path)
    assert reader._impl.bag_pairs_kernel_name() == FUSED
    check_pair_counts(reader, (dim, bits), FUSED)


def test_one_word_per_wavefront_runs_fused(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=64)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 1 and reader._impl.pairs_kernel_name() == '' and reader._impl.bag_pairs_kernel_name() == FUSED
    check_pair_counts(reader, 'one word per wavefront', FUSED, counts=(1, 3, 200))


def test_an_odd_number_of_words_per_wavefront(native, make_model, monkeypatch):
    # asked for nine lanes per word, dims 324 .. 360 get 40-symbol segments and nine lanes: seven words per wavefront
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7, reader.info()['lanes_per_word']
    check_pair_counts(reader, 'seven words per wavefront', FUSED, counts=(1, 2, 200))


def test_launch_options_never_change_a_bit(native, make_model):
    # blocks of 1, 2, 7 and 8 wavefronts and runs of 1 .. 64 tiles' worth of bags: a run of bags starts at every parity of
    # the wave index, and the results are the contract's every time
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bag_pairs_batch(words_per_wave(reader), 400, N_ROWS, 12)
    values = entry_values(reader, rows)
    wants = {mode: bag_pairs_by_the_contract(values, offsets, mode) for mode in MODES}
    on_device, cut = to_device(rows), to_device(offsets)

    def run(waves, tiles):
        for mode in MODES:
            got = reader.bag_pair_similarity_device(on_device, cut, mode, return_dots=True, return_norms=True)
            assert all(same_bits(one, other) for one, other in zip(got, wants[mode])), (waves, tiles, mode)
            assert reader.last_bag_pairs_kernel == FUSED

    sweep_options(reader, run, pairs=[(1, 1), (2, 5), (7, 2), (8, 64)])


# ---- 3. the fallback path: the pooled lookup and the dense kernel ----

@pytest.mark.parametrize('storage,bits,dim', [('uniform', 8, 300), ('full', 8, 300), ('trained', 4, 7), ('trained', 4, 302),
                                              ('trained', 6, 516)])
def test_fallback_models(native, make_model, storage, bits, dim):
    import torch
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    assert reader._impl.bag_pairs_kernel_name() == ''
    # the C entry point says MEMB_HIP_UNSUPPORTED (the binding: False) and launches nothing
    guard = torch.full((8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    rows, offsets = to_device(np.arange(8)), to_device(np.arange(9))
    assert reader._impl.bag_pair_similarity_to_device(rows.data_ptr(), 8, offsets.data_ptr(), 4, 1, guard.data_ptr(), 0, 0, 0) is False
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    check_pair_counts(reader, (storage, bits, dim), DENSE)


def test_without_a_fused_kernel_bags_are_pooled_in_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_DEVICE_SLICE', 64)   # slices of 32 pairs, offsets rebased per slice
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    rows, offsets = bag_pairs_batch(4, 32 * 3 + 17, N_ROWS, 8)
    for mode in MODES:
        check_bag_pairs(reader, rows, offsets, mode, ('slices', mode), DENSE)


# ---- 4. special rows, offsets that overrun or descend, words, host arrays, the byte count ----

def test_special_rows(native, tmp_path):
    path, vectors = special_model(native, tmp_path)
    reader = native.Reader(path)
    missing = 0xFFFFFFFF
    # bags:      0: 2^-70 | 0: 2^-70    +0.0 +0.0 | -0.0 -0.0   5 5 4 | 5 5 4    missing x 2 | 5    missing | missing
    bags = [[0], [0], [2, 2], [3, 3], [5, 5, 4], [5, 5, 4], [missing, 77], [5], [missing], [missing, missing]]
    rows = np.array([row for bag in bags for row in bag], dtype=np.uint32)
    offsets = offsets_of([len(bag) for bag in bags])
    cosines, dots, norms = check_bag_pairs(reader, rows, offsets, 'sum', 'special rows', DENSE)
    # 300 products of 2^-140 sum to 300 * 2^-140, below the smallest normal float32: a flush would give 0
    assert dots[0] == np.float32(300 * 2.0 ** -140) and 0 < dots[0] < np.float32(1.1754944e-38)
    assert cosines[0] == dots[0] / (np.float32(1e-12) * np.float32(1e-12))
    minus_zero = np.float32(-0.0).tobytes()
    assert dots[1].tobytes() == minus_zero and cosines[1].tobytes() == minus_zero   # a bag of +0.0 rows . a bag of -0.0 rows
    assert abs(float(cosines[2]) - 1) <= 2.0 ** -22 and norms[2, 0] == norms[2, 1] and norms[2, 0] > 0   # a bag with itself
    assert not cosines[3:].any() and not dots[3:].any() and not norms[4].any() and norms[3, 1] > 0   # missing-only bags
    check_bag_pairs(reader, rows, offsets, 'mean', 'special rows, mean', DENSE)


def test_signed_zero_bags(native, tmp_path):
    path, count = signed_zero_model(native, tmp_path)
    reader = native.Reader(path)
    # row 0 is all -0.0; rows 1 and 2 are subnormal, -0.0 in their first columns
    bags = [[0, 0, 0], [1, 2], [1, 2, 1], [2, 1], [0], []]
    rows = np.array([row for bag in bags for row in bag], dtype=np.uint32)
    offsets = offsets_of([len(bag) for bag in bags])
    for mode in MODES:
        cosines, dots, norms = check_bag_pairs(reader, rows, offsets, mode, ('signed zeros', mode), DENSE)
        assert norms[0, 0] == 0 and dots[0] == 0 and cosines[0] == 0     # -0.0 rows against subnormal rows: a signed zero
        assert dots[2].tobytes() == np.float32(-0.0).tobytes()           # a bag of -0.0 against the empty bag's +0.0


def test_offsets_that_overrun_or_descend(native, make_model):
    # read as the pooled kernels read them: clamped to n, a backwards range empty; nothing outside [0, n) is read (the ids
    # sit at the very end of their allocation's used part, and the results are the reference's)
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(90, N_ROWS, 21)
    for name, offsets in (('overrun', [0, 10, 20, 50, 80, 95, 200, 0xFFFFFFFF, 0xFFFFFFFF]),
                          ('descending', [0, 30, 10, 40, 40, 5, 90, 60, 90]),
                          ('all beyond n', [500, 600, 700]),
                          ('overlapping', [0, 90, 0, 90, 45])):
        for mode in MODES:
            check_bag_pairs(reader, rows, np.array(offsets, dtype=np.int64), mode, (name, mode), FUSED)
    # n == 0: every bag is empty
    want = check_bag_pairs(reader, np.zeros(0, dtype=np.uint32), np.array([0, 0, 5, 9, 9]), 'mean', 'no entries', FUSED)
    assert not want[0].any() and not want[2].any()


def test_sentences_and_host_arrays_take_the_rows_path(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    sentences_a = [[words[5], 'no such word é', words[0]], [], list(words[100:140]), [words[7]], ['nor this one']]
    sentences_b = [[words[6], words[7]], [words[3]], list(words[120:150]), [words[7]], [words[1], words[2]]]
    interleaved = [sentence for pair in zip(sentences_a, sentences_b) for sentence in pair]
    rows = reader.resolve_rows([word for sentence in interleaved for word in sentence])
    offsets = offsets_of([len(sentence) for sentence in interleaved])
    host = native.Reader(path, device='cpu')
    for mode in MODES:
        want = bag_pairs_by_the_contract(reader.rows_embedding(rows), offsets, mode)
        got = reader.sentence_similarity_device(sentences_a, sentences_b, mode)
        assert same_bits(got, want[0]) and got[1] == 0 and got[4] == 0 and abs(float(got[3]) - 1) <= 2.0 ** -22
        # numpy to numpy on the GPU reader and on a device='cpu' reader: the same bits
        on_gpu = reader.bag_pair_similarity(rows, offsets, mode, return_dots=True, return_norms=True)
        on_cpu = host.bag_pair_similarity(rows, offsets, mode, return_dots=True, return_norms=True)
        assert all(isinstance(part, np.ndarray) for part in on_gpu)
        assert all(bits_equal(one, other) for one, other in zip(on_gpu, on_cpu))
        assert all(bits_equal(one, other) for one, other in zip(on_gpu, want))
        assert bits_equal(reader.bag_pair_similarity(rows, offsets, mode), want[0])
    assert same_bits(reader.sentence_similarity_device([], []), np.zeros(0, dtype=np.float32))


def test_bag_pairs_algorithmic_bytes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bag_pairs_batch(4, 10, N_ROWS, 3)
    pooled = int(reader._impl.pooled_algorithmic_bytes(rows, offsets.astype(np.uint32)))
    read = pooled - 20 * 4 * 300   # without the 4 * dim stored per bag
    count = reader._impl.bag_pairs_algorithmic_bytes
    cut = offsets.astype(np.uint32)
    assert count(rows, cut) == read + 10 * 4
    assert count(rows, cut, True, True, True) == read + 10 * 16
    assert count(rows, cut, False, True, False) == read + 10 * 4
    assert count(rows, cut, cosines=False, dots=False, norms=True) == read + 10 * 8
    assert count(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32)) == 0
    with pytest.raises(ValueError, match='2 \\* pairs \\+ 1'):
        count(rows, cut[:-1])


# ---- 5. other streams ----

def test_another_stream_and_no_allocation(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bag_pairs_batch(4, 500, N_ROWS, 31)
    want = bag_pairs_by_the_contract(reader.rows_embedding(rows), offsets, 'mean')
    on_device, cut = to_device(rows), to_device(offsets)
    out = torch.empty((500,), dtype=torch.float32, device='cuda')
    reader.bag_pair_similarity_device(on_device, cut, out=out)   # (warm: the model is staged, the kernel loaded)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out.fill_(float(SENTINEL))
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        returned = reader.bag_pair_similarity_device(on_device, cut, out=out)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before   # rows, offsets and out on the device: nothing allocated
        stream.synchronize()
    assert returned.data_ptr() == out.data_ptr() and same_bits(out, want[0]) and reader.last_bag_pairs_kernel == FUSED


def test_two_streams_at_once(native, make_model):
    from pooled_device import run_on_two_streams
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    other, _ = make_model(N_ROWS, 300, 'uniform', 8)
    jobs = []
    for thread, reader in enumerate([native.Reader(path), native.Reader(other)]):
        rows, offsets = bag_pairs_batch(4, 300, N_ROWS, 40 + thread)
        want = bag_pairs_by_the_contract(reader.rows_embedding(rows), offsets, 'mean')
        jobs.append((reader, to_device(rows), to_device(offsets), want))

    def call(thread, repeat):
        reader, rows, offsets, want = jobs[thread]
        return reader.bag_pair_similarity_device(rows, offsets, return_dots=True, return_norms=True), want, (thread, repeat)

    run_on_two_streams(jobs, call, repeats=5)


# ---- 6. what Python and the C entry point refuse ----

def test_python_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(10, dtype=np.uint32))
    offsets = to_device(np.array([0, 2, 4, 7, 10]))
    with pytest.raises(TypeError, match='rows must be'):
        reader.bag_pair_similarity_device(rows.cpu(), offsets)                     # wrong device
    with pytest.raises(TypeError, match='rows must be'):
        reader.bag_pair_similarity_device(rows.to(torch.int64), offsets)           # wrong dtype
    with pytest.raises(TypeError, match='rows must be'):
        reader.bag_pair_similarity_device(to_device(np.arange(20, dtype=np.uint32))[::2], offsets)   # not contiguous
    with pytest.raises(TypeError, match='offsets must be'):
        reader.bag_pair_similarity_device(rows, offsets.cpu())
    with pytest.raises(TypeError, match='offsets must be'):
        reader.bag_pair_similarity_device(rows, offsets.to(torch.int64))
    with pytest.raises(ValueError, match='odd number'):
        reader.bag_pair_similarity_device(rows, offsets[:4].contiguous())          # three bags
    with pytest.raises(ValueError, match="'sum' or 'mean'"):
        reader.bag_pair_similarity_device(rows, offsets, 'max')
    with pytest.raises(TypeError, match='float32'):
        reader.bag_pair_similarity_device(rows, offsets, out=torch.empty((2,), dtype=torch.float16, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        reader.bag_pair_similarity_device(rows, offsets, out=torch.empty((3,), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='must be on cuda'):
        reader.bag_pair_similarity_device(rows, offsets, out=torch.empty((2,), dtype=torch.float32))
    with pytest.raises(ValueError, match='same length'):
        reader.sentence_similarity_device([['a']], [])
    # the C entry point's own refusals, with a staged model: nothing is launched (the sentinels stay)
    guard = torch.full((8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    call = reader._impl.bag_pair_similarity_to_device
    for arguments, word in (((0, 10, offsets.data_ptr(), 2, 1, guard.data_ptr(), 0, 0, 0), 'null argument'),
                            ((rows.data_ptr(), 10, 0, 2, 1, guard.data_ptr(), 0, 0, 0), 'null argument'),
                            ((rows.data_ptr(), 10, offsets.data_ptr(), 2, 1, 0, 0, 0, 0), 'at least one'),
                            ((rows.data_ptr(), 10, offsets.data_ptr(), 2, 2, guard.data_ptr(), 0, 0, 0), 'unknown pooling mode'),
                            ((rows.data_ptr(), 10, offsets.data_ptr(), 2, 1, guard.data_ptr() + 2, 0, 0, 0), 'aligned'),
                            ((rows.data_ptr(), 10, offsets.data_ptr(), 2, 1, 0, 0, guard.data_ptr() + 1, 0), 'aligned'),
                            ((rows.data_ptr(), 10, offsets.data_ptr(), 2 ** 35 + 1, 1, guard.data_ptr(), 0, 0, 0), 'too large')):
        with pytest.raises(RuntimeError, match=word):
            call(*arguments)
    assert call(0, 0, 0, 0, 1, 0, 0, 0, 0) is True   # pairs == 0: a no-op
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    # nothing was launched by a refused call; the reader still answers
    same = to_device(np.array([0, 5, 10]))
    both = to_device(np.concatenate([np.arange(5), np.arange(5)]))
    assert abs(float(reader.bag_pair_similarity_device(both, same)[0]) - 1) <= 2.0 ** -22
