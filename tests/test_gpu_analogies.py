"""Analogies on the GPU: the selection with exclusion lists alone over a dense matrix (between sentinels), the fused call in
every key form and geometry against the reference over similarity_matrix_device's matrix and against the parent path
(k + E, then the stable-sort drop), the weighted sums against the reference over unit_rows_embedding_device's output, the
word-level calls against their pieces and against a device='cpu' reader, a uniform model through the fallback, and the
refusals. Every comparison is bit for bit."""
import numpy as np
import pytest

from analogies_reference import drop_by_stable_sort, topk_excluding_by_the_contract, weighted_rows_sum_reference
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, to_device
from pooled_reference import ids_with_misses
from query_topk_reference import rows_of_every_kind, same_topk, topk_by_the_contract
from test_gpu_queries import KEY_FORM_ROWS, N_ROWS, queries_to_device, words_per_wave
from test_gpu_query_topk import SENTINEL, SENTINEL_POSITION, dense_topk, memb, tied_candidates

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained+topk_select_excluding+topk_merge'
DENSE = 'pairs_dense+topk_select_excluding+topk_merge'
PLAIN = 'query_matrix_trained+topk_select+topk_merge'
LIST_SENTINEL = 5   # a real column: a kernel that read beyond a row's `width` entries would exclude it


def lists_to_device(lists, spare=2):
    """the (count, width) int64 lists on the device, rows width + spare entries apart, LIST_SENTINEL around them; width 0
    with spare 0: no list at all"""
    import torch
    count, width = lists.shape
    if width + spare == 0:
        return None, 0, 0
    buffer = torch.full((count + 1, width + spare), LIST_SENTINEL, dtype=torch.int64, device='cuda')
    buffer[:count, :width] = torch.from_numpy(np.ascontiguousarray(lists, dtype=np.int64)).cuda()
    return buffer, buffer.data_ptr(), width + spare


def dense_topk_excluding(matrix, k, lists, ld=None, base=0, held=None, spare=2, list_spare=2):
    """_memb.dense_topk_excluding_to_device on a host matrix, as test_gpu_query_topk.dense_topk calls its sibling: the
    outputs between sentinels and above a guard row, a dirty workspace of exactly the size asked for"""
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
    keep, pointer, ld_excluded = lists_to_device(lists, list_spare)
    memb().dense_topk_excluding_to_device(
        0, on_device.data_ptr(), count, n, ld, base, k, held is not None, pointer, lists.shape[1], ld_excluded, values.data_ptr(),
        positions.data_ptr(), k + spare, workspace.data_ptr() if needed else 0, needed, torch.cuda.current_stream().cuda_stream)
    got_values, got_positions = values.cpu().numpy(), positions.cpu().numpy()
    assert (got_values[:count, k:] == np.float32(SENTINEL)).all() and (got_values[count] == np.float32(SENTINEL)).all()
    assert (got_positions[:count, k:] == SENTINEL_POSITION).all() and (got_positions[count] == SENTINEL_POSITION).all()
    assert (workspace[needed // 4:].cpu().numpy() == 0x7FC00001).all()
    return np.ascontiguousarray(got_values[:count, :k]), np.ascontiguousarray(got_positions[:count, :k])


def two_segments():
    return memb().QUERY_TOPK_MIN_SEGMENT + 76


@pytest.fixture(scope='module')
def kinds():
    n = two_segments()
    named = rows_of_every_kind(n, seed=14)
    return [name for name, _ in named], np.stack([row for _, row in named])


# ---- 1. the selection kernel alone ----

@pytest.mark.parametrize('k', (1, 10, 64))
def test_dense_selection_with_lists(native, kinds, k):
    names, matrix = kinds
    count, n = matrix.shape
    base = 1000
    plain = dense_topk(matrix, k, base=base)
    # (a) no list, a list of width 0 and an all -1 list: the bits of the plain call
    assert same_topk(dense_topk_excluding(matrix, k, np.zeros((count, 0), dtype=np.int64), list_spare=0, base=base), plain)
    assert same_topk(dense_topk_excluding(matrix, k, np.zeros((count, 0), dtype=np.int64), base=base), plain)
    assert same_topk(dense_topk_excluding(matrix, k, np.full((count, 7), -1, dtype=np.int64), ld=n + 3, base=base), plain)
    best = topk_by_the_contract(matrix, 64, base=base)[1]
    segment = memb().QUERY_TOPK_MIN_SEGMENT
    boundaries = base + np.array([0, segment - 1, segment, n - 1], dtype=np.int64)
    ignored = np.array([-1, base - 1, base + n, base + n + 5, best[0, 0], best[0, 0], -1, best[0, 1], -(1 << 62), 1 << 62], dtype=np.int64)
    cases = [('own best 1', best[:, :1]), ('own best 3', best[:, :3]), ('own best 64', best),                  # (b)
             ('boundaries', np.broadcast_to(boundaries, (count, 4))),                                              # (c)
             ('duplicates and entries outside', np.broadcast_to(ignored, (count, ignored.size)))]                  # (d)
    for label, lists in cases:
        want = topk_excluding_by_the_contract(matrix, k, lists, base=base)
        got = dense_topk_excluding(matrix, k, lists, base=base)
        if not same_topk(got, want):
            bad = [names[q] for q in range(count)
                   if not same_topk((got[0][q:q + 1], got[1][q:q + 1]), (want[0][q:q + 1], want[1][q:q + 1]))]
            raise AssertionError('k {} {}: rows {} differ'.format(k, label, bad))
        if label.startswith('own best'):
            assert not same_topk(got, plain), (k, label)   # every excluded entry survives the threshold: the answer changes
    # (d) by hand: of the duplicates only the first row's two best are inside
    got = dense_topk_excluding(matrix[:1], k, ignored[None, :], base=base)
    wider = topk_by_the_contract(matrix[:1], k + 2, base=base)
    assert same_topk(got, (np.ascontiguousarray(wider[0][:, 2:]), np.ascontiguousarray(wider[1][:, 2:])))


def test_more_excluded_than_left(native):
    # (e) 70 columns, 64 of them excluded, k = 10: six entries and four empty slots
    matrix = np.stack([row for _, row in rows_of_every_kind(70, seed=3)])
    lists = np.broadcast_to(np.arange(3, 67, dtype=np.int64)[::-1], (matrix.shape[0], 64))
    got = dense_topk_excluding(matrix, 10, lists)
    assert same_topk(got, topk_excluding_by_the_contract(matrix, 10, lists))
    assert (got[1][:, 6:] == -1).all() and np.isneginf(got[0][:, 6:]).all() and (got[1][:, :6] >= 0).all()
    assert (np.sort(got[1][:, :6], axis=1) == np.array([0, 1, 2, 67, 68, 69])).all()
    everything = np.broadcast_to(np.arange(64, dtype=np.int64), (matrix.shape[0], 64))
    none = dense_topk_excluding(matrix[:, :64], 10, everything)
    assert (none[1] == -1).all() and np.isneginf(none[0]).all()


def test_excluded_among_ties_and_nans(native, kinds):
    # (f) the excluded entries sit among tied values and among NaNs; the rest keeps its stable order
    names, matrix = kinds
    n = matrix.shape[1]
    constant, nans = matrix[names.index('constant')], matrix[names.index('nan')]
    nan_columns = np.nonzero(np.isnan(nans))[0]
    rows = np.stack([constant, nans])
    lists = np.stack([np.array([0, 2, 3, 64, 1024], dtype=np.int64), nan_columns[[0, 2, 3, 5, 6]].astype(np.int64)])
    got = dense_topk_excluding(rows, 10, lists)
    assert same_topk(got, topk_excluding_by_the_contract(rows, 10, lists))
    assert got[1][0].tolist() == [1, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert got[1][1].tolist() == [int(c) for c in nan_columns if c not in set(lists[1].tolist())][:10]
    assert n // 2 in nan_columns   # (the NaN with a payload of its own is among them)


@pytest.mark.parametrize('k', (1, 10, 64))
def test_slices_merge_to_the_same_bits_in_any_order(native, kinds, k):
    # (g) slices fed with merge in both orders and base != 0, the list naming positions of both slices
    _, matrix = kinds
    count, n = matrix.shape
    base = 500
    best = topk_by_the_contract(matrix, 64, base=base)[1]
    lists = np.concatenate([best[:, :5], np.broadcast_to(base + np.array([0, n // 2 - 1, n // 2, n - 1]), (count, 4))], axis=1)
    want = topk_excluding_by_the_contract(matrix, k, lists, base=base)
    one = dense_topk_excluding(matrix, k, lists, base=base)
    assert same_topk(one, want), k
    assert ((lists >= base) & (lists < base + n // 2)).any() and (lists >= base + n // 2).any()
    slices = [(0, n // 2), (n // 2, n)]
    for order in (slices, slices[::-1]):
        held = None
        for start, stop in order:
            held = dense_topk_excluding(matrix[:, start:stop], k, lists, ld=stop - start + 1, base=base + start, held=held)
        assert same_topk(held, one), (k, order)


# ---- 2. the fused call ----

def topk_excluding_with_workspace(reader, vectors, on_device, k, lists, minimal, spare=2):
    """the raw call with a workspace of exactly the minimal or the recommended size, outputs between sentinels"""
    import torch
    count, n = vectors.shape[0], on_device.numel()
    needed = reader._impl.query_topk_workspace_bytes(count, n, k, minimal)
    workspace = torch.full((needed // 4 + 2,), 0x7FC00001, dtype=torch.int32, device='cuda')
    values = torch.full((count + 1, k + spare), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((count + 1, k + spare), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    keep, pointer, ld_excluded = lists_to_device(lists)
    assert reader._impl.query_topk_excluding_to_device(
        vectors.data_ptr(), count, vectors.stride(0) if count > 1 else reader.dim, on_device.data_ptr(), n, k, pointer,
        lists.shape[1], ld_excluded, values.data_ptr(), positions.data_ptr(), k + spare, workspace.data_ptr(), needed,
        torch.cuda.current_stream().cuda_stream)
    got_values, got_positions = values.cpu().numpy(), positions.cpu().numpy()
    assert (got_values[:count, k:] == np.float32(SENTINEL)).all() and (got_values[count] == np.float32(SENTINEL)).all()
    assert (got_positions[:count, k:] == SENTINEL_POSITION).all() and (got_positions[count] == SENTINEL_POSITION).all()
    assert (workspace[needed // 4:].cpu().numpy() == 0x7FC00001).all()
    return np.ascontiguousarray(got_values[:count, :k]), np.ascontiguousarray(got_positions[:count, :k])


def check_fused(reader, n_rows, context):
    block = memb().QUERY_MATRIX_BLOCK
    counts = (1, block, block + 1)
    n = two_segments()   # two segments under the recommended workspace, eighteen slices under the minimal
    rows = tied_candidates(n, n_rows, 41)
    queries = np.random.default_rng(42).standard_normal((max(counts), reader.dim)).astype(np.float32)
    on_device, vectors = to_device(rows), queries_to_device(queries)
    matrix = reader.similarity_matrix_device(vectors, on_device).cpu().numpy()
    assert (matrix != 0).any()
    # each query's list: three of its best (tied candidates: in different slices of 64), a column of the first and of the
    # last slice, padding; one query's list is all padding
    best = topk_by_the_contract(matrix, 64)[1]
    lists = np.concatenate([best[:, [0, 2, 5]], np.broadcast_to(np.array([3, n - 1, -1]), (max(counts), 3))], axis=1).astype(np.int64)
    lists[max(counts) - 2] = -1
    lists[0, :3] = best[0, [0, 1, 40]]
    assert len({int(p) // 64 for p in lists[0] if p >= 0}) >= 3   # (candidates of different slices)
    for count in counts:
        for k in (10, 58, 64) if count == counts[-1] else (10,):
            want = topk_excluding_by_the_contract(matrix[:count], k, lists[:count])
            least = topk_excluding_with_workspace(reader, vectors[:count], on_device, k, lists[:count], minimal=True)
            recommended = topk_excluding_with_workspace(reader, vectors[:count], on_device, k, lists[:count], minimal=False)
            assert same_topk(least, recommended), (context, count, k, 'minimal against recommended workspace')
            assert same_topk(least, want), (context, count, k)
            if k + lists.shape[1] <= 64:   # the parent path: k + E, then the stable-sort drop
                wider = reader.similarity_topk_device(vectors[:count], on_device, k + lists.shape[1])
                assert reader.last_query_topk_kernel == PLAIN, context
                dropped = drop_by_stable_sort(wider[0].cpu().numpy(), wider[1].cpu().numpy(), lists[:count], k)
                assert same_topk(least, dropped), (context, count, k, 'the parent path')
    # through Python: a strided list, fewer candidates than k, and no list at all
    import torch
    strided = torch.from_numpy(np.ascontiguousarray(lists[:2])).cuda()
    assert strided.stride() == (lists.shape[1], 1)
    got = reader.similarity_topk_device(vectors[:2], on_device[:7], 10, exclude=strided[:, :4])
    assert reader.last_query_topk_kernel == FUSED, context
    assert same_topk((got[0].cpu().numpy(), got[1].cpu().numpy()), topk_excluding_by_the_contract(matrix[:2, :7], 10, lists[:2, :4])), context
    plain = reader.similarity_topk_device(vectors[:2], on_device, 10)
    assert reader.last_query_topk_kernel == PLAIN, context
    empty = reader.similarity_topk_device(vectors[:2], on_device, 10, exclude=strided[:, :0])
    assert reader.last_query_topk_kernel == FUSED and same_topk([part.cpu().numpy() for part in empty], [part.cpu().numpy() for part in plain])


FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.query_topk_excluding_kernel_name() == FUSED, context
        FORMS_REACHED.add(kernel_form(reader))
        check_fused(reader, KEY_FORM_ROWS, context)

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


def test_seven_words_per_wavefront(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7
    check_fused(reader, N_ROWS, 'seven words per wavefront')


# ---- 3. weighted sums ----

def check_sums(reader, context):
    import torch
    from memb_amd import _memb
    dim = reader.dim
    rows = ids_with_misses(80, N_ROWS, 21)
    rows[1] = 0xFFFFFFFF
    offsets = np.array([0, 0, 1, 4, 74, 74, 80], dtype=np.int64)   # bags of 0, 1, 3, 70, 0 and 6 entries
    weights = np.random.default_rng(22).choice(np.array([1, -1, 0.5, -0.0], dtype=np.float32), size=80)
    on_device = to_device(rows)
    unit = reader.unit_rows_embedding_device(on_device).cpu().numpy()
    assert not unit[1].any() and unit.any()
    device_offsets = torch.from_numpy(offsets.astype(np.int32)).cuda()
    for given in (weights, None):
        want = weighted_rows_sum_reference(unit, given, offsets)
        got = reader.compose_queries_device(on_device, device_offsets, None if given is None else torch.from_numpy(given).cuda())
        assert tuple(got.shape) == (6, dim) and same_bits(got, want), (context, given is None)
        assert same_bits(reader.compose_queries(rows, offsets, given), want), (context, given is None)
    assert not want[[0, 4]].view(np.uint32).any()
    # the raw call: an `out` with a row stride above dim between sentinels, a matrix with a row stride of its own
    wide = torch.full((80, dim + 3), float('nan'), dtype=torch.float32, device='cuda')
    wide[:, :dim] = torch.from_numpy(unit).cuda()
    out = torch.full((7, dim + 5), float(SENTINEL), dtype=torch.float32, device='cuda')
    _memb.weighted_rows_sum_to_device(
        0, wide.data_ptr(), dim + 3, torch.from_numpy(weights).cuda().data_ptr(), device_offsets.data_ptr(), 6, dim, out.data_ptr(),
        dim + 5, torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    assert same_bits(np.ascontiguousarray(got[:6, :dim]), weighted_rows_sum_reference(unit, weights, offsets)), context
    assert (got[:6, dim:] == np.float32(SENTINEL)).all() and (got[6] == np.float32(SENTINEL)).all()
    # offsets beyond the entries are clamped by compose_queries_device, and no entry at all is answered with zeros
    beyond = reader.compose_queries_device(on_device, torch.tensor([0, 3, 90], dtype=torch.int32, device='cuda'))
    assert same_bits(beyond, weighted_rows_sum_reference(unit, None, [0, 3, 80]))
    nothing = reader.compose_queries_device(on_device[:0], torch.zeros(3, dtype=torch.int32, device='cuda'))
    assert tuple(nothing.shape) == (2, dim) and not nothing.cpu().numpy().view(np.uint32).any()


def test_weighted_sums(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    check_sums(native.Reader(path), 'trained 4-bit, dim 300')
    path, _ = make_model(N_ROWS, 50, 'uniform', 8)
    reader = native.Reader(path)
    assert reader.dim % 4 != 0
    check_sums(reader, 'uniform, dim 50')


# ---- 4. words ----

def test_analogies(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader, host = native.Reader(path), native.Reader(path, device='cpu')
    a, b, c, d = words[5], words[17], words[40], words[99]
    positive = [[b, c], [(b, 0.5), c, (d, 2.0)], [a], [b, 'no such word é'], [], [c, c]]
    negative = [[a], [(a, -0.25), d], [], [a], [], []]
    flat = [[b, c, a], [b, c, d, a, d], [a], None, None, [c, c]]
    weights = [[1, 1, -1], [0.5, 1, 2.0, -0.25, -1], [1], None, None, [1, 1]]
    for k in (7, 64):
        values, rows = reader.analogies_device(positive, negative, k)
        assert reader.last_query_topk_kernel == FUSED
        assert values.dtype == torch.float32 and rows.dtype == torch.int64 and tuple(values.shape) == tuple(rows.shape) == (6, k)
        values, rows = values.cpu().numpy(), rows.cpu().numpy()
        for q, entries in enumerate(flat):
            if entries is None:   # an unknown word, no word: empty slots
                assert (rows[q] == -1).all() and np.isneginf(values[q]).all(), q
                continue
            own = reader.resolve_rows_device(entries)
            offsets = torch.tensor([0, len(entries)], dtype=torch.int32, device='cuda')
            query = reader.compose_queries_device(own, offsets, torch.tensor(weights[q], dtype=torch.float32, device='cuda'))
            matrix = reader.similarity_matrix_device(query, reader._all_rows_device(torch, 0)).cpu().numpy()
            want = topk_excluding_by_the_contract(matrix, k, own.cpu().numpy().astype(np.int64)[None, :])
            assert same_topk((values[q:q + 1], rows[q:q + 1]), want), (k, q)
            assert (rows[q] >= 0).all() and not set(rows[q].tolist()) & set(own.cpu().numpy().tolist()), (k, q)   # k = 64 with three words
    pairs = reader.analogies(positive, negative, 7)
    assert pairs == host.analogies(positive, negative, 7)
    assert pairs[3] == pairs[4] == [] and [len(answer) for answer in pairs] == [7, 7, 7, 0, 0, 7]
    assert not {word for word, _ in pairs[0]} & {a, b, c}
    assert reader.analogy(a, b, c, k=7) == pairs[0] and reader.analogy(a, b, c) == pairs[0][:1] == host.analogy(a, b, c)
    assert tuple(reader.analogies_device([], None, 3)[0].shape) == (0, 3) and reader.analogies([], None, 3) == []
    with pytest.raises(ValueError, match='64'):
        reader.analogies_device([[a] * 65])
    assert tuple(reader.analogies_device([[a] * 40], [[b] * 24], 3)[1].shape) == (1, 3)
    with pytest.raises(ValueError, match='63'):
        reader.most_similar_device([a], k=64)   # (as it was)


# ---- 5. without a fused kernel ----

def test_a_uniform_model_through_the_fallback(native, make_model, monkeypatch):
    import memb_amd.reader
    import torch
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 128)   # 200 candidates: two slices
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    assert reader._impl.query_topk_excluding_kernel_name() == ''
    rows = tied_candidates(200, N_ROWS, 9)
    queries = np.random.default_rng(10).standard_normal((3, 300)).astype(np.float32)
    on_device, vectors = to_device(rows), queries_to_device(queries, ld=303, shift=1)
    matrix = reader.similarity_matrix_device(vectors, on_device).cpu().numpy()
    best = topk_by_the_contract(matrix, 64)[1]
    lists = np.ascontiguousarray(np.concatenate([best[:, [0, 1, 3]], np.broadcast_to(np.array([127, 128, 199, -1]), (3, 4))], axis=1), dtype=np.int64)
    lists[1] = -1
    for k in (1, 10, 64):
        got = reader.similarity_topk_device(vectors, on_device, k, exclude=torch.from_numpy(lists).cuda())
        assert reader.last_query_topk_kernel == DENSE
        assert same_topk((got[0].cpu().numpy(), got[1].cpu().numpy()), topk_excluding_by_the_contract(matrix, k, lists)), k
    none = reader.similarity_topk_device(vectors, on_device[:0], 4, exclude=torch.from_numpy(lists).cuda())
    assert (none[1].cpu().numpy() == -1).all() and np.isneginf(none[0].cpu().numpy()).all()
    assert reader.last_query_topk_kernel == 'topk_merge'
    host = reader.similarity_topk(queries, rows, 10, exclude=lists)
    assert same_topk(host, topk_excluding_by_the_contract(matrix, 10, lists))


# ---- 6. refusals ----

def test_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    on_device = to_device(ids_with_misses(40, N_ROWS, 3))
    vectors = queries_to_device(np.ones((3, 300), dtype=np.float32))
    good = torch.full((3, 4), -1, dtype=torch.int64, device='cuda')
    with pytest.raises(TypeError, match='int64'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=good.to(torch.int32))
    with pytest.raises(TypeError, match='int64'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=[[1, 2]] * 3)
    with pytest.raises(TypeError, match='on the GPU'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=good.cpu())
    with pytest.raises(ValueError, match='64'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=torch.full((3, 65), -1, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=good[:2])
    with pytest.raises(ValueError, match='shape'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=good[0])
    with pytest.raises(ValueError, match='contiguous'):
        reader.similarity_topk_device(vectors, on_device, 5, exclude=good.t().contiguous().t())
    with pytest.raises(TypeError, match='weights'):
        reader.compose_queries_device(on_device, torch.tensor([0, 40], dtype=torch.int32, device='cuda'), torch.ones(39, device='cuda'))
    with pytest.raises(TypeError, match='offsets'):
        reader.compose_queries_device(on_device, torch.tensor([0, 40], dtype=torch.int64, device='cuda'))
    # the C entry points: every new refusal, the sentinels left in place -- nothing was launched
    values = torch.full((3, 5), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((3, 5), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    matrix = torch.zeros((3, 40), dtype=torch.float32, device='cuda')
    lists = torch.zeros((3, 70), dtype=torch.int64, device='cuda')
    needed = memb().dense_topk_workspace_bytes(3, 40, 5)
    workspace = torch.full((needed // 4,), 0x7FC00001, dtype=torch.int32, device='cuda')
    fused_bytes = reader._impl.query_topk_workspace_bytes(3, 40, 5)
    fused_workspace = torch.full((fused_bytes // 4,), 0x7FC00001, dtype=torch.int32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    for word, pointer, width, ld_excluded in (('at most 64', lists.data_ptr(), 65, 70), ('ld_excluded', lists.data_ptr(), 4, 3),
                                              ('null', 0, 4, 4), ('aligned', lists.data_ptr() + 4, 4, 4)):
        with pytest.raises(RuntimeError, match=word):
            memb().dense_topk_excluding_to_device(
                0, matrix.data_ptr(), 3, 40, 40, 0, 5, False, pointer, width, ld_excluded, values.data_ptr(), positions.data_ptr(), 5,
                workspace.data_ptr(), needed, stream)
        with pytest.raises(RuntimeError, match=word):
            reader._impl.query_topk_excluding_to_device(
                vectors.data_ptr(), 3, 300, on_device.data_ptr(), 40, 5, pointer, width, ld_excluded, values.data_ptr(),
                positions.data_ptr(), 5, fused_workspace.data_ptr(), fused_bytes, stream)
    torch.cuda.synchronize()
    assert (values.cpu().numpy() == np.float32(SENTINEL)).all() and (positions.cpu().numpy() == SENTINEL_POSITION).all()
    assert (workspace.cpu().numpy() == 0x7FC00001).all() and (fused_workspace.cpu().numpy() == 0x7FC00001).all()


# ---- 7. a captured graph ----

def test_captured_into_a_graph(native, make_model):
    """similarity_topk_device with exclusion lists and a caller's workspace, captured, then replayed once over other queries
    AND other lists, both written in place; the answer is the host reader's for those"""
    import torch
    from test_gpu_query_topk import capture, graph_case, slices_of_256
    reader, host, rows, on_device, others = graph_case(native, make_model, 73)
    count, k = 5, 10
    queries = torch.from_numpy(np.random.default_rng(74).standard_normal((count, 300)).astype(np.float32)).cuda()
    lists = torch.from_numpy(np.random.default_rng(75).integers(0, rows.size, size=(count, 6)).astype(np.int64)).cuda()
    workspace = slices_of_256(reader._impl.query_topk_workspace_bytes(count, rows.size, k, True), count)
    graph, (values, positions) = capture(lambda: reader.similarity_topk_device(queries, on_device, k, exclude=lists, workspace=workspace))
    assert reader.last_query_topk_kernel == FUSED
    # the other lists: three of each other query's tied best, a column of the first and of the last slice, padding
    best = host.similarity_topk(others, rows, 64)[1]
    other_lists = np.concatenate([best[:, [0, 2, 5]], np.broadcast_to(np.array([3, rows.size - 1, -1]), (count, 3))], axis=1).astype(np.int64)
    queries.copy_(torch.from_numpy(others))
    lists.copy_(torch.from_numpy(other_lists))
    values.fill_(SENTINEL)
    positions.fill_(SENTINEL_POSITION)
    graph.replay()
    torch.cuda.synchronize()
    want = host.similarity_topk(others, rows, k, exclude=other_lists)
    assert not same_topk(want, host.similarity_topk(others, rows, k))   # (the lists name entries that would have been kept)
    assert same_topk((values.cpu().numpy(), positions.cpu().numpy()), want)
