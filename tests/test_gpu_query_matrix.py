"""Cosine similarity of many query vectors against ONE shared candidate list on the GPU (memb_hip_query_matrix.hip:
query_matrix_trained; hip_query_matrix_launch.h).

Every check compares bits against three things: (i) the contract of include/memb_hip_query_matrix.h in numpy
(tests/query_matrix_reference.py) over the reader's own fp32 rows from reader.rows_embedding; (ii) query_similarity_device
on the candidate ids repeated once per query; (iii) rows_embedding_device and the dense pair kernel over (query, row) side
by side. The tolerance is zero, whichever kernel ran. A result never depends on Q or n, so each of the three is computed
once per reader for the largest Q and n and sliced."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, to_device
from pooled_reference import ids_with_misses, signed_zero_model
from query_matrix_reference import matrix_by_the_contract
from test_gpu_queries import KEY_FORM_ROWS, N_ROWS, SENTINEL, TILES_PER_WAVE, queries_to_device, words_per_wave

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained'
DENSE = 'pairs_dense'


def block():
    """B: the queries the kernel holds in registers at once (hip_query_matrix.h: QUERY_BLOCK)"""
    from memb_amd import _memb
    return _memb.QUERY_MATRIX_BLOCK


def per_store(reader):
    """S: the queries whose results one store instruction writes, floor(64 / W)"""
    return 64 // words_per_wave(reader)


def sweep_sizes(reader):
    words, b, s = words_per_wave(reader), block(), per_store(reader)
    counts = sorted({count for count in (1, 2, b - 1, b, b + 1, 2 * b + 1, s, s + 1) if count >= 1})
    sizes = sorted({n for n in (1, words - 1, words, words + 1, 3 * words + 1) if n >= 1})
    return counts, sizes


def planned_run(n, count, words, tiles=TILES_PER_WAVE):
    """hip_query_matrix_launch.h's planQueryMatrixGrid at the reader's default options: planQueryGrid's run of one query
    shared out among the queries, never below a tile; several tiles only where one block and one store hold every query"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one = max(1, min(tiles * words, n // (cus * 28), 1 << 16))
    tile = min(words, one)
    return max(tile, one // count) if count <= min(block(), 64 // words) else tile


def repeated_queries(reader, vectors, on_device):
    """(ii): query_similarity_device over the ids repeated once per query, offsets [0, n, 2n, ..]: (cosines, dots, norms) (Q, n)"""
    count, n = vectors.shape[0], on_device.numel()
    got = reader.query_similarity_device(
        vectors, on_device.repeat(count), to_device(np.arange(count + 1, dtype=np.int64) * n), return_dots=True, return_norms=True)
    return got[0].view(count, n), got[1].view(count, n), got[2][1].view(count, n)


def two_steps(reader, vectors, on_device):
    """(iii): the candidates decoded once, every (query, row) side by side through the dense pair kernel"""
    import torch
    from memb_amd import _memb
    count, n, dim = vectors.shape[0], on_device.numel(), reader.dim
    decoded = reader.rows_embedding_device(on_device)
    side_by_side = torch.stack((vectors.unsqueeze(1).expand(count, n, dim), decoded.unsqueeze(0).expand(count, n, dim)), dim=2).contiguous()
    scalars = torch.empty((4, count * n), dtype=torch.float32, device='cuda')
    _memb.dense_pair_similarity_to_device(
        0, side_by_side.data_ptr(), count * n, dim, dim, scalars[0].data_ptr(), scalars[1].data_ptr(), scalars[2:].data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    return scalars[0].view(count, n), scalars[1].view(count, n), scalars[2:].reshape(-1).view(count, n, 2)[:, :, 1]


def three_references(reader, queries, rows, vectors=None):
    """the three oracles for the whole (Q, n) problem, on the host, checked against one another"""
    on_device = to_device(rows)
    vectors = queries_to_device(queries) if vectors is None else vectors
    want = matrix_by_the_contract(queries, reader.rows_embedding(rows))
    second = [part.cpu().numpy() for part in repeated_queries(reader, vectors, on_device)]
    third = [part.cpu().numpy() for part in two_steps(reader, vectors, on_device)]
    for other in (second, third):
        assert bits_equal(other[0], want[0]) and bits_equal(other[1], want[1]), 'the oracles disagree'
        assert all(bits_equal(other[2][q], want[2]) for q in range(len(queries)))
    return want


def check_matrix(reader, queries, rows, want, context, kernel, ld=None, shift=0, alone=True):
    """similarity_matrix_device on the first Q queries and n rows of a problem whose references are `want` (sliced): the
    three outputs, last_query_matrix_kernel, `out` with a row stride > n between sentinels and above a guard row, and each
    output alone through the raw binding"""
    import torch
    count, n, dim = len(queries), len(rows), reader.dim
    cosines, dots, norms = want[0][:count, :n], want[1][:count, :n], want[2][:n]
    on_device, vectors = to_device(rows), queries_to_device(queries, ld, shift)
    got = reader.similarity_matrix_device(vectors, on_device, return_dots=True, return_norms=True)
    assert reader.last_query_matrix_kernel == kernel, (context, reader.last_query_matrix_kernel)
    assert tuple(got[0].shape) == (count, n) and got[0].dtype == torch.float32 and got[0].is_cuda, context
    if not same_bits(got[0], cosines):
        bad = np.argwhere(got[0].cpu().numpy().view(np.uint32) != np.ascontiguousarray(cosines).view(np.uint32))
        raise AssertionError('{}: {} of {} cosines differ, first {}'.format(context, len(bad), count * n, bad[:6].tolist()))
    assert same_bits(got[1], dots), (context, 'dots')
    assert tuple(got[2][1].shape) == (n,) and same_bits(got[2][1], norms), (context, 'norms')
    from norms_reference import norms_by_the_contract
    assert tuple(got[2][0].shape) == (count,) and same_bits(got[2][0], norms_by_the_contract(queries)), (context, 'query norms')
    # cosines alone into a caller's tensor: rows ld_out = n + 3 floats apart, the padding and a guard row keep the sentinel
    frame = torch.full((count + 1, n + 3), float(SENTINEL), dtype=torch.float32, device='cuda')
    returned = reader.similarity_matrix_device(vectors, on_device, out=frame[:count, :n])
    assert returned.data_ptr() == frame.data_ptr(), context
    host = frame.cpu().numpy()
    assert bits_equal(host[:count, :n], cosines) and (host[:count, n:] == SENTINEL).all() and (host[count] == SENTINEL).all(), (context, 'out')
    if alone and kernel == FUSED:
        stream = torch.cuda.current_stream().cuda_stream
        raw = reader._impl.query_matrix_to_device
        arguments = (vectors.data_ptr(), count, vectors.stride(0) if count > 1 else dim, on_device.data_ptr(), n)
        frame.fill_(float(SENTINEL))
        assert raw(*arguments, 0, frame.data_ptr(), n + 3, 0, stream)   # dots alone
        host = frame.cpu().numpy()
        assert bits_equal(host[:count, :n], dots) and (host[:count, n:] == SENTINEL).all() and (host[count] == SENTINEL).all(), (context, 'dots alone')
        frame.fill_(float(SENTINEL))
        assert raw(*arguments, 0, 0, 0, frame[0, 1:].data_ptr(), stream)   # norms alone: ld_out is not looked at
        host = frame.cpu().numpy().reshape(-1)
        assert bits_equal(host[1:n + 1], norms) and host[0] == SENTINEL and (host[n + 1:] == SENTINEL).all(), (context, 'norms alone')


def problem(reader, n_rows, seed, counts, sizes):
    queries = np.random.default_rng(seed + 77).standard_normal((max(counts), reader.dim)).astype(np.float32)
    rows = ids_with_misses(max(sizes), n_rows, seed)
    rows[0] %= np.uint32(n_rows)   # (a known row in front: no batch is all zeros)
    if len(rows) > 2:
        rows[1] = 0xFFFFFFFF       # a missing row and an id beyond the model in every batch of three and more
        rows[2] = n_rows
    return queries, rows


def check_sizes(reader, n_rows, context, kernel=FUSED, alone_at=None):
    """Q in {1, 2, B - 1, B, B + 1, 2B + 1, S, S + 1} x n in {1, W - 1, W, W + 1, 3W + 1}, missing ids among the candidates"""
    counts, sizes = sweep_sizes(reader)
    queries, rows = problem(reader, n_rows, 13, counts, sizes)
    want = three_references(reader, queries, rows)
    assert (want[0] != 0).any() and (len(rows) < 3 or not want[2][1:3].any())
    for count in counts:
        for n in sizes:
            check_matrix(reader, queries[:count], rows[:n], want, (context, count, n), kernel, alone=(count, n) == (counts[-1], sizes[-1]))


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form_and_size(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.query_matrix_kernel_name() == FUSED, context
        FORMS_REACHED.add(kernel_form(reader))
        check_sizes(reader, KEY_FORM_ROWS, context)

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


# ---- 2. dims, wavefront shapes, several tiles per wavefront ----

@pytest.mark.parametrize('dim', (4, 256, 260, 300, 512))
@pytest.mark.parametrize('bits', (4, 6))
def test_fused_dims(native, make_model, dim, bits):
    path, _ = make_model(N_ROWS, dim, 'trained', bits)
    reader = native.Reader(path)
    assert reader._impl.query_matrix_kernel_name() == FUSED
    check_sizes(reader, N_ROWS, (dim, bits))


def test_one_word_per_wavefront(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=64)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 1 and per_store(reader) == 64
    check_sizes(reader, N_ROWS, 'one word per wavefront')


def test_an_odd_number_of_words_per_wavefront(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7 and per_store(reader) == 9
    check_sizes(reader, N_ROWS, 'seven words per wavefront')


LONG_RUN_CASES = [({}, KEY_FORM_ROWS, 300, (False, True)), ({'MEMB_HIP_NO_FAST': 1}, KEY_FORM_ROWS, 300, (False, False)),
                  ({'MEMB_HIP_LANES': 9}, N_ROWS, 340, None)]


@pytest.mark.parametrize('environment,n_rows,dim,form', LONG_RUN_CASES)
def test_a_wavefront_walks_several_tiles(native, make_model, monkeypatch, environment, n_rows, dim, form):
    # The batches above give every wavefront at most one tile. This is the smallest n for which the plan gives a wavefront
    # more than a tile with Q = 2: a run of W + 1 candidates, a full tile and a tile of one word, the queries' norms kept
    # across the two.
    import torch
    path, _ = make_model(n_rows, dim, 'trained', 4, distribution='normal')
    set_environment(monkeypatch, **environment)
    reader = native.Reader(path)
    assert reader._impl.query_matrix_kernel_name() == FUSED
    assert form is None or kernel_form(reader) == form, kernel_form(reader)
    words = words_per_wave(reader)
    assert words == (7 if 'MEMB_HIP_LANES' in environment else words) and words > 1 and block() >= 2 and per_store(reader) >= 2
    count = 2
    n = count * (words + 1) * torch.cuda.get_device_properties(0).multi_processor_count * 28
    owned = planned_run(n, count, words)
    assert owned == words + 1 and planned_run(n - 1, count, words) == words, (n, owned, words)
    rows = ids_with_misses(n, n_rows, 23)
    queries = np.random.default_rng(24).standard_normal((count, dim)).astype(np.float32)
    on_device, vectors = to_device(rows), queries_to_device(queries, ld=dim + 3, shift=1)
    got = reader.similarity_matrix_device(vectors, on_device, return_dots=True, return_norms=True)
    assert reader.last_query_matrix_kernel == FUSED
    # (ii) in full
    second = repeated_queries(reader, vectors, on_device)
    assert torch.equal(got[0].view(torch.int32), second[0].view(torch.int32)), 'cosines against repeated queries'
    assert torch.equal(got[1].view(torch.int32), second[1].view(torch.int32)), 'dots against repeated queries'
    assert torch.equal(got[2][1].view(torch.int32), second[2][0].view(torch.int32)), 'norms against repeated queries'
    # (i) on a seeded sample of 4 096 (query, candidate) positions plus the first and the last tile
    sample = np.unique(np.concatenate([np.random.default_rng(25).integers(0, n, size=4096), np.arange(words), np.arange(n - words, n)]))
    want = matrix_by_the_contract(queries, reader.rows_embedding(rows[sample]))
    host = [got[0].cpu().numpy(), got[1].cpu().numpy(), got[2][1].cpu().numpy()]
    picked = np.random.default_rng(26).integers(0, count, size=len(sample))
    columns = np.arange(len(sample))
    assert bits_equal(host[0][picked, sample], want[0][picked, columns]) and bits_equal(host[1][picked, sample], want[1][picked, columns])
    for tile in (sample < words, sample >= n - words):
        assert bits_equal(host[0][:, sample[tile]], want[0][:, tile]) and bits_equal(host[1][:, sample[tile]], want[1][:, tile])
    assert bits_equal(host[2][sample], want[2]) and (want[0] != 0).any()
    # ONE query takes a path of its own (the word's dot and bb in one block): the first half of the candidates is the
    # smallest batch whose runs exceed a tile with Q = 1; against (ii), and against the rows of the matrix above
    half = n // 2
    assert planned_run(half, 1, words) == words + 1 and planned_run(half - 1, 1, words) == words
    one = reader.similarity_matrix_device(vectors[1:2], on_device[:half], return_dots=True, return_norms=True)
    alone = reader.query_similarity_device(vectors[1], on_device[:half], return_dots=True, return_norms=True)
    for mine, theirs, above in ((one[0][0], alone[0], got[0][1, :half]), (one[1][0], alone[1], got[1][1, :half]), (one[2][1], alone[2][1], got[2][1][:half])):
        assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32)) and torch.equal(mine.view(torch.int32), above.view(torch.int32))


# ---- 3. odd layouts ----

def test_strided_and_unaligned_queries(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    counts, sizes = sweep_sizes(reader)
    queries, rows = problem(reader, N_ROWS, 19, counts, sizes)
    want = three_references(reader, queries, rows)
    # ld_queries = dim + 3: every row at another alignment; a matrix one float behind a 16-byte boundary; both
    for ld, shift in ((303, 0), (300, 1), (303, 1), (304, 0)):
        check_matrix(reader, queries, rows, want, ('ld', ld, 'shift', shift), FUSED, ld=ld, shift=shift)


# ---- 4. signed zeros ----

def test_signed_zeros_through_the_fused_kernel(native, make_model):
    # a trained model decodes no -0.0, the query brings it: -0.0 against a missing row's +0.0, dims with one and two pieces per lane
    for dim in (4, 256, 300):
        path, _ = make_model(N_ROWS, dim, 'trained', 4)
        reader = native.Reader(path)
        rows = np.array([0xFFFFFFFF, 5, N_ROWS, 6, 5], dtype=np.uint32)
        queries = np.full((3, dim), -0.0, dtype=np.float32)
        queries[1] = reader.rows_embedding(rows[1:2])[0]   # a query equal to a candidate row: whatever the contract says
        queries[2] = np.random.default_rng(dim).standard_normal(dim)
        want = three_references(reader, queries, rows)
        check_matrix(reader, queries, rows, want, ('minus zero', dim), FUSED)
        # every lane holds a piece of -0.0 from 64 pieces on; below that the lanes without a piece add their +0.0
        zero = np.float32(-0.0 if dim >= 256 else 0.0).tobytes()
        assert want[1][0, 0].tobytes() == zero and want[1][0, 2].tobytes() == zero and want[0][0, 0].tobytes() == zero
        assert want[2][1] > 0 and want[2][0] == 0 and abs(float(want[0][1, 1]) - 1) <= 2.0 ** -22


def test_signed_zero_rows(native, tmp_path):
    path, _ = signed_zero_model(native, tmp_path)
    reader = native.Reader(path)
    rows = np.array([0, 1, 2, 0xFFFFFFFF, 0, 1], dtype=np.uint32)   # row 0 is all -0.0; rows 1 and 2 are subnormal
    queries = np.zeros((3, 300), dtype=np.float32)
    queries[0] = -0.0
    queries[2] = reader.rows_embedding(np.array([1], dtype=np.uint32))[0]
    want = three_references(reader, queries, rows)
    check_matrix(reader, queries, rows, want, 'signed zeros', reader._impl.query_matrix_kernel_name() or DENSE)
    minus_zero = np.float32(-0.0).tobytes()
    assert want[1][0, 0].tobytes() == np.float32(0.0).tobytes() and want[1][0, 3].tobytes() == minus_zero and want[1][1, 0].tobytes() == minus_zero


# ---- 5. the fallback path ----

@pytest.mark.parametrize('storage,bits,dim', [('uniform', 8, 300), ('full', 8, 300), ('trained', 4, 7), ('trained', 4, 302),
                                              ('trained', 6, 516)])
def test_fallback_models(native, make_model, storage, bits, dim):
    import torch
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    assert reader._impl.query_matrix_kernel_name() == ''
    guard = torch.full((16,), float(SENTINEL), dtype=torch.float32, device='cuda')
    rows = to_device(np.arange(8))
    query = torch.ones((2, dim), dtype=torch.float32, device='cuda')
    raw = reader._impl.query_matrix_to_device
    assert raw(query.data_ptr(), 2, dim, rows.data_ptr(), 8, guard.data_ptr(), 0, 8, 0, 0) is False   # MEMB_HIP_UNSUPPORTED
    assert raw(query.data_ptr(), 2, dim, 0, 0, guard.data_ptr(), 0, 0, 0, 0) is True                   # no candidates: a no-op
    assert raw(0, 0, dim, rows.data_ptr(), 8, guard.data_ptr(), 0, 8, 0, 0) is True                    # no queries: a no-op
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    check_sizes(reader, N_ROWS, (storage, bits, dim), kernel=DENSE)


def test_without_a_fused_kernel_candidates_are_decoded_in_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 16)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    queries = np.random.default_rng(8).standard_normal((3, 300)).astype(np.float32)
    rows = ids_with_misses(53, N_ROWS, 8)
    want = three_references(reader, queries, rows)
    check_matrix(reader, queries, rows, want, 'slices', DENSE, ld=303, shift=1)


# ---- 6. words, host arrays, the byte count ----

def test_words_and_host_arrays(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    words_a = [words[5], 'no such word é', words[9]]
    words_b = [words[6], 'nor this one', words[5], words[7]] + list(words[100:110])
    matrix = reader.words_similarity_matrix_device(words_a, words_b)
    assert tuple(matrix.shape) == (3, 14) and reader.last_query_matrix_kernel == FUSED
    want = matrix_by_the_contract(reader.rows_embedding(reader.resolve_rows(words_a)), reader.rows_embedding(reader.resolve_rows(words_b)))
    assert same_bits(matrix, want[0])
    got = matrix.cpu().numpy()
    assert not got[1].any() and not got[:, 1].any() and abs(float(got[0, 2]) - 1) <= 2.0 ** -22 and (got[2, 3:] != 0).all()
    assert tuple(reader.words_similarity_matrix_device([], words_b).shape) == (0, 14)
    assert tuple(reader.words_similarity_matrix_device(words_a, []).shape) == (3, 0)
    # numpy to numpy on the GPU reader and on a device='cpu' reader: the same bits
    host = native.Reader(path, device='cpu')
    queries = np.random.default_rng(5).standard_normal((5, 300)).astype(np.float32)
    rows = ids_with_misses(40, N_ROWS, 5)
    on_gpu = reader.similarity_matrix(queries, rows, return_dots=True, return_norms=True)
    on_cpu = host.similarity_matrix(queries, rows, return_dots=True, return_norms=True)
    reference = matrix_by_the_contract(queries, reader.rows_embedding(rows))
    for one, other, wanted in zip((on_gpu[0], on_gpu[1], on_gpu[2][1]), (on_cpu[0], on_cpu[1], on_cpu[2][1]), reference):
        assert isinstance(one, np.ndarray) and bits_equal(one, other) and bits_equal(one, wanted)
    assert bits_equal(on_gpu[2][0], on_cpu[2][0])
    assert bits_equal(reader.similarity_matrix(queries[0], rows), host.similarity_matrix(queries[0], rows))


def test_query_matrix_algorithmic_bytes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(45, N_ROWS, 3)
    # a count made here: the candidates as ONE bag of the pooled count without its 8 bytes of offsets and the 4 * dim stored
    candidates = int(reader._impl.pooled_algorithmic_bytes(rows, np.array([0, 45], dtype=np.uint32))) - 8 - 4 * 300
    count = reader._impl.query_matrix_algorithmic_bytes
    missing = np.full(3, 0xFFFFFFFF, dtype=np.uint32)   # by hand where no compressed byte is read: three ids, five queries
    assert count(missing, 5) == 3 * 4 + 5 * 4 * 300 + 5 * 3 * 4
    assert count(rows, 7) == candidates + 7 * 1200 + 7 * 45 * 4
    assert count(rows, 7, True, True, True) == candidates + 7 * 1200 + 2 * 7 * 45 * 4 + 45 * 4
    assert count(rows, 7, False, True, False) == candidates + 7 * 1200 + 7 * 45 * 4
    assert count(rows, 7, cosines=False, dots=False, norms=True) == candidates + 7 * 1200 + 45 * 4
    assert count(rows, 1) == candidates + 1200 + 45 * 4 and count(rows, 0) == candidates
    assert count(np.zeros(0, dtype=np.uint32), 0) == 0
    with pytest.raises(RuntimeError, match='too large'):
        count(rows, 2 ** 16 + 1)


# ---- 7. another stream, no allocation ----

def test_another_stream_and_no_allocation(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    queries = np.random.default_rng(31).standard_normal((5, 300)).astype(np.float32)
    rows = ids_with_misses(70, N_ROWS, 31)
    want = matrix_by_the_contract(queries, reader.rows_embedding(rows))
    on_device, vectors = to_device(rows), queries_to_device(queries)
    out = torch.empty((5, 70), dtype=torch.float32, device='cuda')
    reader.similarity_matrix_device(vectors, on_device, out=out)   # (warm: the model is staged, the kernel loaded)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out.fill_(float(SENTINEL))
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        for _ in range(3):
            returned = reader.similarity_matrix_device(vectors, on_device, out=out)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before   # everything on the device: nothing allocated
        stream.synchronize()
    assert returned.data_ptr() == out.data_ptr() and same_bits(out, want[0]) and reader.last_query_matrix_kernel == FUSED


# ---- 8. what Python and the C entry point refuse ----

def test_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(10, dtype=np.uint32))
    queries = torch.ones((2, 300), dtype=torch.float32, device='cuda')
    call = reader.similarity_matrix_device
    with pytest.raises(TypeError, match='rows must be'):
        call(queries, rows.cpu())
    with pytest.raises(TypeError, match='rows must be'):
        call(queries, rows.to(torch.int64))
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.to(torch.float64), rows)
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.cpu(), rows)
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.cpu().numpy(), rows)
    with pytest.raises(ValueError, match='shape'):
        call(queries[:, :296], rows)
    with pytest.raises(ValueError, match='shape'):
        call(queries.unsqueeze(0), rows)
    with pytest.raises(ValueError, match='contiguous last dimension'):
        call(torch.ones((2, 600), dtype=torch.float32, device='cuda')[:, ::2], rows)
    with pytest.raises(ValueError, match='row stride'):
        call(torch.ones((1, 300), dtype=torch.float32, device='cuda').expand(2, 300), rows)
    with pytest.raises(TypeError, match='float32'):
        call(queries, rows, out=torch.empty((2, 10), dtype=torch.float16, device='cuda'))
    with pytest.raises(TypeError, match=r'\(Q, n\)'):
        call(queries, rows, out=torch.empty((2, 9), dtype=torch.float32, device='cuda'))
    with pytest.raises(TypeError, match=r'\(Q, n\)'):
        call(queries, rows, out=torch.empty((20,), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='row stride'):
        call(queries, rows, out=torch.empty((1, 10), dtype=torch.float32, device='cuda').expand(2, 10))
    with pytest.raises(ValueError, match='contiguous last dimension'):
        call(queries, rows, out=torch.empty((2, 20), dtype=torch.float32, device='cuda')[:, ::2])
    with pytest.raises(ValueError, match='must be on cuda'):
        call(queries, rows, out=torch.empty((2, 10), dtype=torch.float32))
    # the C entry point's own refusals, with a staged model: nothing is launched (the sentinels stay)
    guard = torch.full((24,), float(SENTINEL), dtype=torch.float32, device='cuda')
    raw = reader._impl.query_matrix_to_device
    q, r, g = queries.data_ptr(), rows.data_ptr(), guard.data_ptr()
    for arguments, word in (((0, 2, 300, r, 10, g, 0, 10, 0, 0), 'null argument'),
                            ((q, 2, 300, 0, 10, g, 0, 10, 0, 0), 'null argument'),
                            ((q, 2, 300, r, 10, 0, 0, 10, 0, 0), 'at least one'),
                            ((q, 2, 299, r, 10, g, 0, 10, 0, 0), 'ld_queries'),
                            ((q, 2, 300, r, 10, g, 0, 9, 0, 0), 'ld_out'),
                            ((q, 2, 300, r, 10, 0, g, 9, 0, 0), 'ld_out'),
                            ((q, 2, 300, r, 10, g + 2, 0, 10, 0, 0), 'aligned'),
                            ((q + 1, 2, 300, r, 10, g, 0, 10, 0, 0), 'aligned'),
                            ((q, 2, 300, r, 10, 0, 0, 10, g + 1, 0), 'aligned'),
                            ((q, 2, 300, r, 2 ** 36 + 1, g, 0, 2 ** 36 + 1, 0, 0), 'too large'),
                            ((q, 2 ** 16 + 1, 300, r, 10, g, 0, 10, 0, 0), 'too large')):
        with pytest.raises(RuntimeError, match=word):
            raw(*arguments)
    assert raw(q, 2, 300, 0, 0, g, 0, 0, 0, 0) is True     # n == 0: a no-op
    assert raw(0, 0, 300, r, 10, g, 0, 10, 0, 0) is True   # n_queries == 0: a no-op
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    # nothing was launched by a refused call; the reader still answers
    itself = reader.rows_embedding_device(rows[:1])
    assert abs(float(reader.similarity_matrix_device(itself, rows)[0, 0]) - 1) <= 2.0 ** -22
