"""The k nearest candidates of every query on the GPU (memb_hip_query_topk.hip: topk_select, topk_merge;
hip_query_topk_launch.h).

Zero tolerance: values are compared as bits and positions must be equal, against tests/query_topk_reference.py's
topk_by_the_contract -- over matrices built here for the dense selection, over similarity_matrix_device's own result for
the fused call, whatever the workspace, the slices and the segments."""
import numpy as np
import pytest

from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, to_device
from pooled_reference import ids_with_misses
from query_topk_reference import rows_of_every_kind, same_topk, topk_by_the_contract
from test_gpu_queries import KEY_FORM_ROWS, N_ROWS, queries_to_device, words_per_wave

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained+topk_select+topk_merge'
DENSE = 'pairs_dense+topk_select+topk_merge'
SENTINEL = -1234.5
SENTINEL_POSITION = -77


def memb():
    from memb_amd import _memb
    return _memb


def dense_topk(matrix, k, ld=None, base=0, held=None, spare=2):
    """_memb.dense_topk_to_device on a host matrix: rows ld floats apart on the device, the outputs ld_out = k + spare apart
    between sentinels and above a guard row, which must all survive; held: (values, positions) on the host to merge into"""
    import torch
    count, n = matrix.shape
    ld = n if ld is None else ld
    on_device = torch.full((count, ld), float('nan'), dtype=torch.float32, device='cuda')
    on_device[:, :n] = torch.from_numpy(np.ascontiguousarray(matrix)).cuda()
    values = torch.full((count + 1, k + spare), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((count + 1, k + spare), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    if held is not None:
        values[:count, :k] = torch.from_numpy(held[0]).cuda()
        positions[:count, :k] = torch.from_numpy(held[1]).cuda()
    needed = memb().dense_topk_workspace_bytes(count, n, k)
    workspace = torch.full((needed // 4 + 2,), 0x7FC00001, dtype=torch.int32, device='cuda')   # (dirty: NaNs, columns in range)
    memb().dense_topk_to_device(
        0, on_device.data_ptr(), count, n, ld, base, k, held is not None, values.data_ptr(), positions.data_ptr(), k + spare,
        workspace.data_ptr() if needed else 0, needed, torch.cuda.current_stream().cuda_stream)
    got_values, got_positions = values.cpu().numpy(), positions.cpu().numpy()
    assert (got_values[:count, k:] == np.float32(SENTINEL)).all() and (got_values[count] == np.float32(SENTINEL)).all()
    assert (got_positions[:count, k:] == SENTINEL_POSITION).all() and (got_positions[count] == SENTINEL_POSITION).all()
    assert (workspace[needed // 4:].cpu().numpy() == 0x7FC00001).all()
    return np.ascontiguousarray(got_values[:count, :k]), np.ascontiguousarray(got_positions[:count, :k])


def dense_sizes(k):
    segment = memb().QUERY_TOPK_MIN_SEGMENT
    return sorted({n for n in (1, k - 1, k, k + 1, 63, 64, 65, 2 * segment - 1, 2 * segment, 2 * segment + 1) if n >= 1})


# ---- 1. the selection kernels alone ----

@pytest.mark.parametrize('k', (1, 2, 63, 64))
def test_dense_selection(native, k):
    for n in dense_sizes(k):
        kinds = rows_of_every_kind(n, seed=k)
        matrix = np.stack([row for _, row in kinds])
        want = topk_by_the_contract(matrix, k, base=1000)
        for ld in (n, n + 3):
            got = dense_topk(matrix, k, ld=ld, base=1000)
            if not same_topk(got, want):
                bad = [kinds[q][0] for q in range(len(kinds))
                       if not same_topk((got[0][q:q + 1], got[1][q:q + 1]), (want[0][q:q + 1], want[1][q:q + 1]))]
                raise AssertionError('k {} n {} ld {}: rows {} differ'.format(k, n, ld, bad))


@pytest.mark.parametrize('k', (1, 2, 63, 64))
def test_slices_merge_to_the_same_bits_in_any_order(native, k):
    segment = memb().QUERY_TOPK_MIN_SEGMENT
    for n in (3, k + 1, 200, 2 * segment + 70):
        matrix = np.stack([row for _, row in rows_of_every_kind(n, seed=100 + k)])
        want = topk_by_the_contract(matrix, k, base=0)
        cuts = [0, n // 3, n - n // 4, n]
        slices = [(cuts[i], cuts[i + 1]) for i in range(3)]
        results = []
        for order in (slices, slices[::-1]):
            held = None
            for start, stop in order:
                held = dense_topk(matrix[:, start:stop], k, ld=stop - start + 1, base=start, held=held)
            results.append(held)
        assert same_topk(results[0], want) and same_topk(results[1], want), (k, n)


def test_no_columns_and_no_rows(native):
    import torch
    empty = dense_topk(np.zeros((3, 0), dtype=np.float32), 5)
    assert (empty[1] == -1).all() and np.isneginf(empty[0]).all()
    # merging nothing into what is held: the held entries, in order
    held = topk_by_the_contract(np.array([[1, np.nan, -np.inf, 1]], dtype=np.float32), 5, base=40)
    shuffled = (np.ascontiguousarray(held[0][:, ::-1]), np.ascontiguousarray(held[1][:, ::-1]))
    assert same_topk(dense_topk(np.zeros((1, 0), dtype=np.float32), 5, held=shuffled), held)
    guard = torch.full((8,), SENTINEL, dtype=torch.float32, device='cuda')
    memb().dense_topk_to_device(0, 0, 0, 0, 0, 0, 3, False, guard.data_ptr(), guard.data_ptr(), 3, 0, 0, 0)   # no rows: a no-op
    assert (guard.cpu().numpy() == np.float32(SENTINEL)).all()


# ---- 2. the fused call ----

def tied_candidates(n, n_rows, seed):
    """ids with misses of which only 37 are distinct: every cosine repeats about n / 37 times, across every boundary of a
    slice (64 candidates with the minimal workspace) and of a segment"""
    rows = ids_with_misses(n, n_rows, seed)
    rows[0] %= np.uint32(n_rows)
    rows[1], rows[2] = 0xFFFFFFFF, n_rows
    return np.ascontiguousarray(rows[np.arange(n) % 37])


def topk_with_workspace(reader, vectors, on_device, k, minimal, spare=2):
    """the raw call with a workspace of exactly the minimal or the recommended size, outputs between sentinels"""
    import torch
    count, n = vectors.shape[0], on_device.numel()
    needed = reader._impl.query_topk_workspace_bytes(count, n, k, minimal)
    workspace = torch.full((needed // 4 + 2,), 0x7FC00001, dtype=torch.int32, device='cuda')
    values = torch.full((count + 1, k + spare), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((count + 1, k + spare), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    assert reader._impl.query_topk_to_device(
        vectors.data_ptr(), count, vectors.stride(0) if count > 1 else reader.dim, on_device.data_ptr(), n, k, values.data_ptr(),
        positions.data_ptr(), k + spare, workspace.data_ptr(), needed, torch.cuda.current_stream().cuda_stream)
    got_values, got_positions = values.cpu().numpy(), positions.cpu().numpy()
    assert (got_values[:count, k:] == np.float32(SENTINEL)).all() and (got_values[count] == np.float32(SENTINEL)).all()
    assert (got_positions[:count, k:] == SENTINEL_POSITION).all() and (got_positions[count] == SENTINEL_POSITION).all()
    assert (workspace[needed // 4:].cpu().numpy() == 0x7FC00001).all()
    return np.ascontiguousarray(got_values[:count, :k]), np.ascontiguousarray(got_positions[:count, :k])


def check_fused(reader, n_rows, context):
    block, per_store = memb().QUERY_MATRIX_BLOCK, 64 // words_per_wave(reader)
    counts = sorted({1, block, block + 1, per_store + 1})
    n = memb().QUERY_TOPK_MIN_SEGMENT + 76   # two segments under the recommended workspace, eighteen slices under the minimal
    rows = tied_candidates(n, n_rows, 41)
    queries = np.random.default_rng(42).standard_normal((max(counts), reader.dim)).astype(np.float32)
    on_device, vectors = to_device(rows), queries_to_device(queries)
    matrix = reader.similarity_matrix_device(vectors, on_device).cpu().numpy()
    assert (matrix != 0).any() and not matrix[:, 1:3].any()
    for count in counts:
        for k in (10, 64) if count == counts[-1] else (10,):
            want = topk_by_the_contract(matrix[:count], k)
            assert len(np.unique(want[0][0])) < k   # (ties among the best)
            least = topk_with_workspace(reader, vectors[:count], on_device, k, minimal=True)
            recommended = topk_with_workspace(reader, vectors[:count], on_device, k, minimal=False)
            assert same_topk(least, recommended), (context, count, k, 'minimal against recommended workspace')
            assert same_topk(least, want), (context, count, k)
    # through Python, fewer candidates than k
    got = reader.similarity_topk_device(vectors[:2], on_device[:7], 10)
    assert reader.last_query_topk_kernel == FUSED, context
    assert same_topk((got[0].cpu().numpy(), got[1].cpu().numpy()), topk_by_the_contract(matrix[:2, :7], 10)), context


FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.query_topk_kernel_name() == FUSED, context
        FORMS_REACHED.add(kernel_form(reader))
        check_fused(reader, KEY_FORM_ROWS, context)

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


def test_seven_words_per_wavefront(native, make_model, monkeypatch):
    from pooled_device import set_environment
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7
    check_fused(reader, N_ROWS, 'seven words per wavefront')


def test_one_candidate_more_than_the_recommended_slice(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    count, k = 64, 10
    lists = reader._impl.query_topk_workspace_bytes(count, 1, k) - 4 * count
    slice_size = (reader._impl.query_topk_workspace_bytes(count, 1 << 30, k) - lists) // (4 * count)
    assert slice_size == (32 << 20) // (4 * count)
    n = slice_size + 1                      # two slices: the recommended one and a single candidate
    on_device = (torch.arange(n, dtype=torch.int32, device='cuda') % N_ROWS).contiguous()
    vectors = reader.rows_embedding_device(on_device[5:5 + count].contiguous())   # each query's own row repeats n / N_ROWS times
    got = reader.similarity_topk_device(vectors, on_device, k)
    assert reader.last_query_topk_kernel == FUSED
    matrix = reader.similarity_matrix_device(vectors, on_device)
    want = topk_by_the_contract(matrix.cpu().numpy(), k)
    assert same_topk((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
    assert (want[1][3, :k] % N_ROWS == 8).all() and (np.diff(want[1][3]) == N_ROWS).all()


def test_byte_count_and_workspace_sizes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(45, N_ROWS, 3)
    without_matrix = int(reader._impl.query_matrix_algorithmic_bytes(rows, 7, False, False, False))
    assert reader._impl.query_topk_algorithmic_bytes(rows, 7, 10) == without_matrix + 7 * 120
    assert reader._impl.query_topk_algorithmic_bytes(rows, 7, 64) == without_matrix + 7 * 768
    with pytest.raises(RuntimeError, match='k must'):
        reader._impl.query_topk_algorithmic_bytes(rows, 7, 65)
    size = reader._impl.query_topk_workspace_bytes
    assert size(64, 2196017, 10) == 64 * 128 * 10 * 8 + 4 * 64 * 131072 == size(64, 1 << 36, 10)
    assert size(64, 2196017, 10, True) == 64 * 128 * 10 * 8 + 4 * 64 * 64
    assert size(0, 5, 3) == 0 and size(5, 0, 3) == 0 and size(5, 5, 65) == 0


# ---- 3. without a fused kernel ----

def test_a_uniform_model_through_the_fallback(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 64)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    assert reader._impl.query_topk_kernel_name() == ''
    rows = tied_candidates(200, N_ROWS, 9)
    queries = np.random.default_rng(10).standard_normal((3, 300)).astype(np.float32)
    on_device, vectors = to_device(rows), queries_to_device(queries, ld=303, shift=1)
    matrix = reader.similarity_matrix_device(vectors, on_device).cpu().numpy()
    for k in (1, 10, 64):
        got = reader.similarity_topk_device(vectors, on_device, k)
        assert reader.last_query_topk_kernel == DENSE
        assert same_topk((got[0].cpu().numpy(), got[1].cpu().numpy()), topk_by_the_contract(matrix, k)), k
    none = reader.similarity_topk_device(vectors, on_device[:0], 4)
    assert (none[1].cpu().numpy() == -1).all() and np.isneginf(none[0].cpu().numpy()).all()
    assert reader.last_query_topk_kernel == 'topk_merge'   # (no candidate: the empty slots are all there is to write)
    assert tuple(reader.similarity_topk_device(vectors[:0], on_device, 4)[1].shape) == (0, 4) and reader.last_query_topk_kernel == ''
    host = reader.similarity_topk(queries, rows, 10)
    assert same_topk(host, topk_by_the_contract(matrix, 10))


def test_a_shorter_last_slice_needs_more_lists_than_a_full_one(native, make_model, monkeypatch):
    # 228 queries are cut into at most 36 segments: a slice of 37 120 columns into 29 of 1 280, the last slice of 29 952 into
    # 30 of 1 024. The fallback reuses one buffer of lists for both and must size it for the larger
    import memb_amd.reader
    import torch
    count, slice_size, tail, k = 228, 37120, 29952, 10
    need = memb().dense_topk_workspace_bytes
    assert need(count, tail, k) > need(count, slice_size, k)
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', slice_size)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    n = slice_size + tail
    on_device = (torch.arange(n, dtype=torch.int32, device='cuda') * 7 % N_ROWS).contiguous()   # every row repeats: ties
    vectors = reader.rows_embedding_device((torch.arange(count, dtype=torch.int32, device='cuda') % N_ROWS).contiguous())
    got = reader.similarity_topk_device(vectors, on_device, k)
    assert reader.last_query_topk_kernel == DENSE
    matrix = reader.similarity_matrix_device(vectors, on_device)
    # every row against the stable sort on the device, which tests/test_query_topk_host.py ties to the contract ...
    ordered = torch.sort(matrix, dim=1, descending=True, stable=True)
    assert torch.equal(got[1], ordered.indices[:, :k]) and torch.equal(got[0].view(torch.int32), ordered.values[:, :k].view(torch.int32))
    # ... and four of them against the contract in numpy
    picked = [0, 1, count // 2, count - 1]
    want = topk_by_the_contract(matrix[picked].cpu().numpy(), k)
    assert same_topk((got[0][picked].cpu().numpy(), got[1][picked].cpu().numpy()), want)
    assert (np.diff(want[1][0]) > 0).all() and len(np.unique(want[0][0])) == 1   # (ties among the best, lower position first)


# ---- 4. words ----

def test_most_similar(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    asked = [words[5], 'no such word é', words[9], words[5]]
    values, rows = (part.cpu().numpy() for part in reader.most_similar_device(asked, k=6))
    assert reader.last_query_topk_kernel == FUSED and values.shape == (4, 6) and rows.dtype == np.int64
    own = reader.resolve_rows(asked).astype(np.int64)
    everything = to_device(np.arange(N_ROWS))
    matrix = reader.similarity_matrix_device(reader.rows_embedding_device(to_device(own[[0, 2]])), everything).cpu().numpy()
    full = topk_by_the_contract(matrix, 7)
    for line, q in ((0, 0), (2, 1), (3, 0)):
        assert full[1][q, 0] == own[line]    # (a row is its own nearest neighbour in this model)
        assert np.array_equal(rows[line], full[1][q, 1:]) and np.array_equal(values[line].view(np.uint32), full[0][q, 1:].view(np.uint32))
        assert own[line] not in rows[line]
    assert (rows[1] == -1).all() and np.isneginf(values[1]).all()       # an unknown word: empty slots
    included = reader.most_similar_device(asked[:1], k=7, exclude_self=False)
    assert same_topk((included[0].cpu().numpy(), included[1].cpu().numpy()), (full[0][:1], full[1][:1]))
    # on the host: the same pairs as a device='cpu' reader gives
    pairs = reader.most_similar(asked, k=6)
    vocabulary = reader.keys()
    assert pairs[1] == [] and pairs[0] == pairs[3] == [(vocabulary[row], float(value)) for value, row in zip(values[0], rows[0])]
    assert pairs == native.Reader(path, device='cpu').most_similar(asked, k=6)
    with pytest.raises(ValueError, match='63'):
        reader.most_similar_device(asked, k=64)
    assert reader.most_similar_device(asked, k=64, exclude_self=False)[1].shape == (4, 64)


# ---- 5. refusals ----

def test_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(200, dtype=np.uint32))
    queries = torch.ones((2, 300), dtype=torch.float32, device='cuda')
    call = reader.similarity_topk_device
    for k in (0, 65):
        with pytest.raises(ValueError, match='64'):
            call(queries, rows, k)
    with pytest.raises(TypeError, match='rows must be'):
        call(queries, rows.cpu(), 3)
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.cpu(), rows, 3)
    with pytest.raises(ValueError, match='shape'):
        call(queries[:, :296], rows, 3)
    with pytest.raises(TypeError, match='workspace'):
        call(queries, rows, 3, workspace=torch.empty((1 << 20,), dtype=torch.float32, device='cuda'))
    with pytest.raises(RuntimeError, match='workspace too small'):
        call(queries, rows, 3, workspace=torch.empty((16,), dtype=torch.uint8, device='cuda'))
    # the C entry point's own refusals, with a staged model: nothing is launched (the sentinels stay)
    least = reader._impl.query_topk_workspace_bytes(2, 200, 10, True)
    workspace = torch.empty((least + 8,), dtype=torch.uint8, device='cuda')
    values = torch.full((24,), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((24,), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    raw = reader._impl.query_topk_to_device
    q, r, v, p, w = queries.data_ptr(), rows.data_ptr(), values.data_ptr(), positions.data_ptr(), workspace.data_ptr()
    for arguments, word in (((0, 2, 300, r, 200, 10, v, p, 10, w, least, 0), 'null argument'),
                            ((q, 2, 300, 0, 200, 10, v, p, 10, w, least, 0), 'null argument'),
                            ((q, 2, 300, r, 200, 10, 0, p, 10, w, least, 0), 'null argument'),
                            ((q, 2, 300, r, 200, 10, v, 0, 10, w, least, 0), 'null argument'),
                            ((q, 2, 300, r, 200, 0, v, p, 10, w, least, 0), 'k must'),
                            ((q, 2, 300, r, 200, 65, v, p, 65, w, least, 0), 'k must'),
                            ((q, 2, 300, r, 200, 10, v, p, 9, w, least, 0), 'ld_out'),
                            ((q, 2, 299, r, 200, 10, v, p, 10, w, least, 0), 'ld_queries'),
                            ((q + 2, 2, 300, r, 200, 10, v, p, 10, w, least, 0), 'aligned'),
                            ((q, 2, 300, r, 200, 10, v + 2, p, 10, w, least, 0), 'aligned'),
                            ((q, 2, 300, r, 200, 10, v, p + 4, 10, w, least, 0), 'aligned'),
                            ((q, 2, 300, r, 200, 10, v, p, 10, w + 4, least, 0), 'aligned'),
                            ((q, 2, 300, r, 200, 10, v, p, 10, w, least - 1, 0), 'workspace too small'),
                            ((q, 2, 300, r, 200, 10, v, p, 10, 0, least, 0), 'workspace too small'),
                            ((q, 2, 300, r, 2 ** 36 + 1, 10, v, p, 10, w, least, 0), 'too large'),
                            ((q, 2 ** 16 + 1, 300, r, 200, 10, v, p, 10, w, least, 0), 'too large')):
        with pytest.raises(RuntimeError, match=word):
            raw(*arguments)
    assert raw(0, 0, 300, r, 200, 10, v, p, 10, 0, 0, 0) is True   # n_queries == 0: a no-op
    torch.cuda.synchronize()
    assert (values.cpu().numpy() == np.float32(SENTINEL)).all() and (positions.cpu().numpy() == SENTINEL_POSITION).all()
    assert raw(q, 2, 300, 0, 0, 10, v, p, 12, 0, 0, 0) is True     # n == 0: the empty slots, the padding untouched
    filled = positions.cpu().numpy()
    assert (filled[:10] == -1).all() and (filled[10:12] == SENTINEL_POSITION).all() and (filled[12:22] == -1).all() and (filled[22:] == SENTINEL_POSITION).all()
    # the reader still answers
    itself = reader.rows_embedding_device(rows[:1])
    assert int(reader.similarity_topk_device(itself, rows, 1)[1][0, 0]) == 0


# ---- 6. a captured graph ----

def graph_case(native, make_model, seed):
    """(reader, host reader, candidates, their ids on the device, five other queries): 1100 tied candidates -- five slices
    of 256 under the workspace of slices_of_256 --, the other queries rows of the model that are candidates themselves"""
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    rows = tied_candidates(1100, N_ROWS, seed)
    host = native.Reader(path, device='cpu')
    return native.Reader(path), host, rows, to_device(rows), host.rows_embedding(np.unique(rows[rows < N_ROWS])[:5])


def slices_of_256(minimal_bytes, matrix_rows):
    """a workspace for slices of 256 candidates where the minimal one holds slices of 64"""
    import torch
    return torch.empty((minimal_bytes + 4 * matrix_rows * 192,), dtype=torch.uint8, device='cuda')


def capture(call):
    """call() once on a side stream, then captured on that one stream (a single chain of launches): (graph, what it returned)"""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call()   # (warm-up)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        returned = call()
    return graph, returned


def test_captured_into_a_graph(native, make_model):
    """similarity_topk_device with a caller's workspace allocates nothing but its results: captured, then replayed once over
    other queries written in place; the answer is the host reader's for those"""
    import torch
    reader, host, rows, on_device, others = graph_case(native, make_model, 71)
    count, k = 5, 10
    queries = torch.from_numpy(np.random.default_rng(72).standard_normal((count, 300)).astype(np.float32)).cuda()
    workspace = slices_of_256(reader._impl.query_topk_workspace_bytes(count, rows.size, k, True), count)
    graph, (values, positions) = capture(lambda: reader.similarity_topk_device(queries, on_device, k, workspace=workspace))
    assert reader.last_query_topk_kernel == FUSED
    queries.copy_(torch.from_numpy(others))
    values.fill_(SENTINEL)
    positions.fill_(SENTINEL_POSITION)
    graph.replay()
    torch.cuda.synchronize()
    want = host.similarity_topk(others, rows, k)
    assert len(np.unique(want[0][0])) == 1 and (np.diff(want[1][0]) > 0).all()   # (bit-equal best, lower position first)
    assert same_topk((values.cpu().numpy(), positions.cpu().numpy()), want)
