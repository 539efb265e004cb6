"""Cosine similarity of query vectors against groups of candidate rows on the GPU (memb_hip_queries.hip: query_trained;
hip_queries_launch.h).

The oracle everywhere: the contract of include/memb_hip_queries.h in numpy (tests/queries_reference.py) over the reader's
own fp32 rows from reader.rows_embedding; the second oracle the two-step path on the same reader, rows_embedding_device and
the dense pair kernel over (query, row) side by side. Compared bit for bit: the tolerance is zero, whichever kernel ran."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, to_device
from pooled_reference import ids_with_misses, offsets_of, signed_zero_model
from queries_reference import groups_of_entries, queries_by_the_contract, query_batch

pytestmark = pytest.mark.gpu

N_ROWS = 3000
KEY_FORM_ROWS = 20000   # the models of tests/test_gpu_pooled.py (built once per session)
SENTINEL = np.float32(-1234.5)
FUSED = 'query_trained'
DENSE = 'pairs_dense'
TILES_PER_WAVE = 4      # memb_pooled::POOLED_TILES_PER_WAVE: the longest run of tiles a wavefront owns by default


def words_per_wave(reader):
    lanes = reader.info()['lanes_per_word']
    return 64 // lanes if lanes else 4


def planned_entries_per_wave(n, words):
    """hip_queries_launch.h's planQueryGrid at the reader's default options: a wavefront owns TILES_PER_WAVE tiles of `words`
    entries, fewer while the grid would not fill the CUs with 28 wavefronts each (four SIMDs of seven), at least one. Below
    28 * CUs entries that is ONE entry per wavefront: only a large batch walks a wavefront over several words and tiles."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, min(TILES_PER_WAVE * words, n // (cus * 28), 1 << 16))


def entry_values(reader, rows):
    rows = np.asarray(rows, dtype=np.uint32)
    return reader.rows_embedding(rows) if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)


def queries_to_device(queries, ld=None, shift=0):
    """the (G, dim) float32 queries on the device: rows ld floats apart (dim unless given), the matrix `shift` floats behind a
    16-byte boundary"""
    import torch
    groups, dim = queries.shape
    ld = ld or dim
    buffer = torch.zeros((groups * ld + 8,), dtype=torch.float32, device='cuda')
    assert buffer.data_ptr() % 16 == 0
    view = buffer[shift:shift + groups * ld].view(groups, ld)[:, :dim]
    view.copy_(torch.from_numpy(np.ascontiguousarray(queries)))
    assert view.data_ptr() % 16 == 4 * (shift % 4)
    return view


def check_queries(reader, queries, rows, offsets, context, kernel, ld=None, shift=0, want=None):
    """query_similarity_device in every output combination against the contract; the row norms against row_norms_device; the
    whole result against rows_embedding_device + the dense pair kernel on the same reader; dots alone and norms alone through
    the raw binding between sentinels; `out` between two sentinels, where the entries that lie in no group keep the
    sentinel; last_query_kernel is `kernel`. Returns the contract's (cosines, dots, norms, inside)."""
    import torch
    from memb_amd import _memb
    rows = np.asarray(rows, dtype=np.uint32)
    offsets = np.asarray(offsets)
    groups, n, dim = len(queries), len(rows), reader.dim
    if want is None:
        want = queries_by_the_contract(queries, entry_values(reader, rows), offsets)
    inside = want[3]
    on_device, cut, vectors = to_device(rows), to_device(offsets), queries_to_device(queries, ld, shift)

    cosines = reader.query_similarity_device(vectors, on_device, cut)
    assert cosines.dtype == torch.float32 and tuple(cosines.shape) == (n,) and cosines.is_cuda, context
    assert reader.last_query_kernel == kernel, (context, reader.last_query_kernel)
    if not same_bits(cosines, want[0]):
        bad = np.nonzero(cosines.cpu().numpy().view(np.uint32) != want[0].view(np.uint32))[0]
        raise AssertionError('{}: {} of {} cosines differ, first {}'.format(context, len(bad), n, bad[:8]))
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.query_similarity_device(vectors, on_device, cut, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and same_bits(got[0], want[0]), (context, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms), (context, dots, norms)
        if dots:
            assert tuple(got[1].shape) == (n,) and same_bits(got[1], want[1]), (context, dots, norms, 'dots')
        if norms:
            query_norms, row_norms = got[2]
            assert tuple(row_norms.shape) == (n,) and same_bits(row_norms, want[2]), (context, dots, norms, 'norms')
            if n:
                assert bits_equal(row_norms.cpu().numpy()[inside], reader.row_norms_device(on_device).cpu().numpy()[inside]), (context, 'row_norms_device')
            from norms_reference import norms_by_the_contract
            assert tuple(query_norms.shape) == (groups,) and same_bits(query_norms, norms_by_the_contract(queries) if groups else np.zeros(0, dtype=np.float32)), (context, 'query norms')
    # the second oracle: query and decoded row side by side through the dense pair kernel
    stream = torch.cuda.current_stream().cuda_stream
    if n and groups:
        group, _ = groups_of_entries(offsets, n)
        decoded = reader.rows_embedding_device(on_device)
        side_by_side = torch.stack((vectors[torch.from_numpy(np.clip(group, 0, groups - 1)).cuda()], decoded), dim=1).contiguous()
        second = torch.empty((4 * n,), dtype=torch.float32, device='cuda')
        _memb.dense_pair_similarity_to_device(
            0, side_by_side.data_ptr(), n, dim, dim, second[:n].data_ptr(), second[n:2 * n].data_ptr(), second[2 * n:].data_ptr(), stream)
        host = second.cpu().numpy()
        assert bits_equal(host[:n][inside], want[0][inside]) and bits_equal(host[n:2 * n][inside], want[1][inside]), (context, 'two steps')
        assert bits_equal(host[2 * n:].reshape(n, 2)[inside, 1], want[2][inside]), (context, 'two steps, norms')
    # dots alone, norms alone: the C entry point with the other pointers null
    framed = lambda values: np.where(inside, values, SENTINEL).astype(np.float32)
    if kernel == FUSED and n and groups:
        alone = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
        arguments = (vectors.data_ptr(), groups, vectors.stride(0) if groups > 1 else dim, on_device.data_ptr(), n, cut.data_ptr())
        assert reader._impl.query_similarity_to_device(*arguments, 0, alone[1:n + 1].data_ptr(), 0, stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:n + 1], framed(want[1])) and host[0] == SENTINEL and host[-1] == SENTINEL, (context, 'dots alone')
        alone.fill_(float(SENTINEL))
        assert reader._impl.query_similarity_to_device(*arguments, 0, 0, alone[1:n + 1].data_ptr(), stream)
        host = alone.cpu().numpy()
        assert bits_equal(host[1:n + 1], framed(want[2])) and host[0] == SENTINEL and host[-1] == SENTINEL, (context, 'norms alone')
    # into a caller's tensor between two sentinels
    buffer = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
    returned = reader.query_similarity_device(vectors, on_device, cut, out=buffer[1:n + 1])
    assert returned.data_ptr() == buffer[1:n + 1].data_ptr(), context
    host = buffer.cpu().numpy()
    assert host[0] == SENTINEL and host[-1] == SENTINEL and bits_equal(host[1:n + 1], framed(want[0])), (context, 'out')
    return want


def check_group_counts(reader, context, kernel, n_rows=N_ROWS, counts=(0, 1, 2, 3, 40)):
    """batches of 0, 1, 2, 3 and 40 groups of 0, 1, W - 1, W, W + 1 and 3 W + 1 entries -- an empty first group, an empty
    last one, three empty ones in a row --, and the batch of 40 again with entries in front of offsets[0] and behind
    offsets[G]; a row of the model against itself; an all-zero query"""
    words = words_per_wave(reader)
    for groups in counts:
        for head, tail in ((0, 0), (words + 1, 5)) if groups == 40 else ((0, 0),):
            queries, rows, offsets = query_batch(words, groups, reader.dim, n_rows, 7 + groups, head=head, tail=tail)
            if groups > 2:
                at = int(offsets[2])   # (group 2 holds 3 W + 1 entries)
                rows[at] %= np.uint32(n_rows)
                queries[2] = reader.rows_embedding(rows[at:at + 1])[0]
                queries[1] = 0
            want = check_queries(reader, queries, rows, offsets, (context, groups, head), kernel)
            assert want[3].sum() == len(rows) - head - tail
            if groups > 2:
                assert abs(float(want[0][at]) - 1) <= 2.0 ** -22, (context, groups)
                assert not want[0][int(offsets[1]):int(offsets[2])].any()   # the zero query
            if groups > 1:
                assert (want[0] != 0).any(), (context, groups)


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.query_kernel_name() == FUSED, context   # one word per wavefront (MEMB_HIP_LANES=64) included
        FORMS_REACHED.add(kernel_form(reader))
        queries, rows, offsets = query_batch(words_per_wave(reader), 40, 300, KEY_FORM_ROWS, context[0], head=3, tail=2)
        want = check_queries(reader, queries, rows, offsets, context, FUSED)
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
    assert reader._impl.query_kernel_name() == FUSED
    check_group_counts(reader, (dim, bits), FUSED)


def test_one_word_per_wavefront_runs_fused(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=64)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 1 and reader._impl.pairs_kernel_name() == '' and reader._impl.query_kernel_name() == FUSED
    check_group_counts(reader, 'one word per wavefront', FUSED, counts=(1, 3, 40))


def test_an_odd_number_of_words_per_wavefront(native, make_model, monkeypatch):
    # asked for nine lanes per word, dims 324 .. 360 get 40-symbol segments and nine lanes: seven words per wavefront
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7, reader.info()['lanes_per_word']
    check_group_counts(reader, 'seven words per wavefront', FUSED, counts=(1, 2, 40))


def test_one_group_spans_wavefronts_and_blocks(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    n = 5000
    # at this size the plan gives every wavefront ONE entry (planned_entries_per_wave), a block waves_per_block wavefronts:
    # 5 000 entries of ONE group take several blocks of several wavefronts, each of which finds the group by itself
    waves = reader.info(n)['waves_per_block']
    assert planned_entries_per_wave(n, words_per_wave(reader)) == 1 and waves > 1 and n > 2 * waves
    rows = np.random.default_rng(3).integers(0, N_ROWS, size=n).astype(np.uint32)   # with repeats: 5 000 draws of 3 000 rows
    assert len(np.unique(rows)) < n
    query = np.random.default_rng(4).standard_normal((1, 300)).astype(np.float32)
    want = check_queries(reader, query, rows, [0, n], 'one group of 5 000', FUSED)
    assert want[3].all() and (want[0] != 0).all()
    # offsets=None and a (dim,) query say the same
    vector = torch.from_numpy(query[0]).cuda()
    assert same_bits(reader.query_similarity_device(vector, to_device(rows)), want[0]) and reader.last_query_kernel == FUSED
    got = reader.query_similarity_device(vector.unsqueeze(0), to_device(rows), return_dots=True, return_norms=True)
    assert same_bits(got[1], want[1]) and same_bits(got[2][1], want[2]) and tuple(got[2][0].shape) == (1,)
    # the k best are torch.topk of the result
    assert same_bits(torch.topk(got[0], 5).values, np.sort(want[0])[::-1][:5].copy())


# (environment, rows of the model, dim, key form or None): nibble keys and byte keys on the session's 20 000-row 4-bit model
# (its codes are at most 8 bits long: nibble keys unless MEMB_HIP_NO_FAST), and seven words per wavefront (nine lanes per word)
LONG_RUN_CASES = [({}, KEY_FORM_ROWS, 300, (False, True)), ({'MEMB_HIP_NO_FAST': 1}, KEY_FORM_ROWS, 300, (False, False)),
                  ({'MEMB_HIP_LANES': 9}, N_ROWS, 340, None)]


@pytest.mark.parametrize('environment,n_rows,dim,form', LONG_RUN_CASES)
def test_a_wavefront_walks_several_tiles_and_groups(native, make_model, monkeypatch, environment, n_rows, dim, form):
    # The batches above give every wavefront one entry. This one is large enough that the plan gives a wavefront a run of
    # two tiles and one word more (one tile and three words more for W > 8): tiles of several words, a partial last tile,
    # group ends inside tiles and inside runs, a query reloaded in the middle of a tile, three empty groups in a row, the
    # long group across runs, and entries in front of offsets[0] and behind offsets[G] that share a tile with scored ones.
    import torch
    path, _ = make_model(n_rows, dim, 'trained', 4, distribution='normal')
    set_environment(monkeypatch, **environment)
    reader = native.Reader(path)
    assert reader._impl.query_kernel_name() == FUSED
    assert form is None or kernel_form(reader) == form, kernel_form(reader)
    words = words_per_wave(reader)
    assert words == (7 if 'MEMB_HIP_LANES' in environment else words) and words > 1
    run = 2 * words + 1 if words <= 8 else words + 3
    target = run * torch.cuda.get_device_properties(0).multi_processor_count * 28
    groups = target * 6 // (6 * words + 3) + 700   # (group_lengths draws a mean of W + 1 / 2 entries per group)
    queries, rows, offsets = query_batch(words, groups, dim, n_rows, 23, head=words + 1, tail=5)
    n = len(rows)
    owned = planned_entries_per_wave(n, words)
    assert words < owned < TILES_PER_WAVE * words and owned % words != 0, (n, owned, words)
    lengths = np.diff(offsets)
    assert any((lengths[k:k + 3] == 0).all() for k in range(1, 40)) and (offsets[1:-1] % words != 0).any()
    assert (offsets[1:-1] % owned != 0).any()   # group ends inside runs
    at = int(offsets[2])   # (group 2 holds 3 W + 1 entries): a row against itself, and an all-zero query
    rows[at] %= np.uint32(n_rows)
    queries[2] = reader.rows_embedding(rows[at:at + 1])[0]
    queries[1] = 0
    want = check_queries(reader, queries, rows, offsets, ('long runs', environment, n, owned), FUSED)
    assert want[3].sum() == n - (words + 1) - 5 and abs(float(want[0][at]) - 1) <= 2.0 ** -22
    # a strided query matrix one float behind a 16-byte boundary, through the same walk
    got = reader.query_similarity_device(queries_to_device(queries, ld=dim + 3, shift=1), to_device(rows), to_device(offsets))
    assert same_bits(got, want[0])


def test_strided_and_unaligned_queries(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, offsets = query_batch(words_per_wave(reader), 40, 300, N_ROWS, 19)
    want = queries_by_the_contract(queries, entry_values(reader, rows), offsets)
    # ld_queries = dim + 3: every row at another alignment; a matrix one float behind a 16-byte boundary; both
    for ld, shift in ((303, 0), (300, 1), (303, 1), (304, 0)):
        check_queries(reader, queries, rows, offsets, ('ld', ld, 'shift', shift), FUSED, ld=ld, shift=shift, want=want)


# ---- 3. the fallback path: a plain decode beside the queries and the dense kernel ----

@pytest.mark.parametrize('storage,bits,dim', [('uniform', 8, 300), ('full', 8, 300), ('trained', 4, 7), ('trained', 4, 302),
                                              ('trained', 6, 516)])
def test_fallback_models(native, make_model, storage, bits, dim):
    import torch
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    assert reader._impl.query_kernel_name() == ''
    # the C entry point says MEMB_HIP_UNSUPPORTED (the binding: False) and launches nothing
    guard = torch.full((8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    rows, offsets = to_device(np.arange(8)), to_device(np.array([0, 8]))
    query = torch.ones((1, dim), dtype=torch.float32, device='cuda')
    assert reader._impl.query_similarity_to_device(query.data_ptr(), 1, dim, rows.data_ptr(), 8, offsets.data_ptr(), guard.data_ptr(), 0, 0, 0) is False
    # no entries or no groups: a no-op for every model
    assert reader._impl.query_similarity_to_device(query.data_ptr(), 1, dim, 0, 0, offsets.data_ptr(), guard.data_ptr(), 0, 0, 0) is True
    assert reader._impl.query_similarity_to_device(0, 0, dim, rows.data_ptr(), 8, 0, guard.data_ptr(), 0, 0, 0) is True
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    check_group_counts(reader, (storage, bits, dim), DENSE)


def test_without_a_fused_kernel_candidates_are_decoded_in_slices(native, make_model, monkeypatch):
    import memb_amd.reader
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 64)
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    queries, rows, offsets = query_batch(4, 40, 300, N_ROWS, 8, head=70, tail=9)
    assert len(rows) > 3 * 64
    check_queries(reader, queries, rows, offsets, 'slices', DENSE, ld=303, shift=1)


# ---- 4. special rows, offsets that do not ascend, words, host arrays, the byte count ----

def test_signed_zero_rows_and_a_query_of_minus_zero(native, tmp_path):
    path, count = signed_zero_model(native, tmp_path)
    reader = native.Reader(path)
    # row 0 is all -0.0; rows 1 and 2 are subnormal, -0.0 in their first columns
    rows = np.array([0, 1, 2, 0xFFFFFFFF, 0, 1, 2, 0xFFFFFFFF, 1], dtype=np.uint32)
    queries = np.zeros((3, 300), dtype=np.float32)
    queries[0] = -0.0
    queries[2] = reader.rows_embedding(np.array([1], dtype=np.uint32))[0]
    cosines, dots, norms, _ = check_queries(reader, queries, rows, [0, 4, 8, 9], 'signed zeros', DENSE)
    minus_zero = np.float32(-0.0).tobytes()
    # (-0.0) * (-0.0) = +0.0; (-0.0) * (+0.0 of a missing row) = -0.0 in every piece: the sign survives the reduction
    assert dots[0].tobytes() == np.float32(0.0).tobytes() and dots[3].tobytes() == minus_zero and cosines[3].tobytes() == minus_zero
    assert dots[4].tobytes() == minus_zero   # +0.0 query against the row of -0.0
    assert not norms[[0, 3, 4, 7]].any()


def test_signed_zeros_through_the_fused_kernel(native, make_model):
    # a trained model decodes no -0.0, the query brings it: -0.0 against a missing row's +0.0, dims with one and two pieces per lane
    for dim in (4, 256, 300):
        path, _ = make_model(N_ROWS, dim, 'trained', 4)
        reader = native.Reader(path)
        rows = np.array([0xFFFFFFFF, 5, N_ROWS, 6], dtype=np.uint32)
        queries = np.full((1, dim), -0.0, dtype=np.float32)
        cosines, dots, norms, _ = check_queries(reader, queries, rows, [0, 4], ('minus zero', dim), FUSED)
        # every lane holds a piece of -0.0 from 64 pieces on; below that the lanes without a piece add their +0.0
        zero = np.float32(-0.0 if dim >= 256 else 0.0).tobytes()
        assert dots[0].tobytes() == zero and dots[2].tobytes() == zero and cosines[0].tobytes() == zero
        assert norms[1] > 0 and norms[0] == 0


def test_offsets_that_do_not_ascend_stay_within_bounds(native, make_model):
    # the results are unspecified; what is specified: the call returns, nothing outside rows[0 .. n), offsets[0 .. groups] and
    # the queries is read (they sit inside larger tensors; a read beyond changes nothing that could be seen, a write would)
    # and nothing outside [0, n) of the outputs is written
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rng = np.random.default_rng(2024)
    n, groups, margin = 700, 23, 64
    for draw in range(6):
        drawn = rng.integers(0, n + 50, size=groups + 1).astype(np.int64)
        if draw == 1:
            drawn[rng.integers(0, groups + 1, size=4)] = 0xFFFFFFFF
        if draw == 2:
            drawn = np.sort(drawn)[::-1].copy()
        ids = torch.full((n + 2 * margin,), 7, dtype=torch.int32, device='cuda')
        ids[margin:margin + n] = to_device(ids_with_misses(n, N_ROWS, draw))
        cut = torch.full((groups + 1 + 2 * margin,), 3, dtype=torch.int32, device='cuda')
        cut[margin:margin + groups + 1] = to_device(drawn)
        vectors = torch.full((groups + 2, 300), float(SENTINEL), dtype=torch.float32, device='cuda')
        vectors[1:groups + 1] = torch.from_numpy(rng.standard_normal((groups, 300)).astype(np.float32)).cuda()
        outputs = torch.full((3, n + 2 * margin), float(SENTINEL), dtype=torch.float32, device='cuda')
        before = (ids.clone(), cut.clone(), vectors.clone())
        assert reader._impl.query_similarity_to_device(
            vectors[1:].data_ptr(), groups, 300, ids[margin:].data_ptr(), n, cut[margin:].data_ptr(),
            outputs[0, margin:].data_ptr(), outputs[1, margin:].data_ptr(), outputs[2, margin:].data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()   # the call returns
        host = outputs.cpu().numpy()
        assert (host[:, :margin] == SENTINEL).all() and (host[:, margin + n:] == SENTINEL).all(), draw
        assert all(torch.equal(one, other) for one, other in zip(before, (ids, cut, vectors))), draw
        written = host[:, margin:margin + n] != SENTINEL
        assert (written[0] == written[1]).all() and (written[0] == written[2]).all() and not np.isnan(host[:, margin:margin + n]).any()
        # an entry that was written was scored against one of the queries: its norm is its row's
        row_norms = reader.row_norms_device(ids[margin:margin + n].contiguous()).cpu().numpy()
        assert bits_equal(host[2, margin:margin + n][written[2]], row_norms[written[2]]), draw
    # Python: through the method the same offsets return as well
    got = reader.query_similarity_device(vectors[1:groups + 1], ids[margin:margin + n].contiguous(), cut[margin:margin + groups + 1].contiguous())
    assert tuple(got.shape) == (n,) and not torch.isnan(got).any()


def test_candidate_words_and_host_arrays(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    query_words = [words[5], 'no such word é', words[9]]
    lists = [[words[6], 'nor this one', words[5], words[7]], [words[1], words[2]], list(words[100:140])]
    cosines, offsets = reader.candidates_similarity_device(query_words, lists)
    assert offsets.cpu().numpy().tolist() == [0, 4, 6, 46] and tuple(cosines.shape) == (46,)
    rows = reader.resolve_rows([word for candidates in lists for word in candidates])
    queries = reader.rows_embedding(reader.resolve_rows(query_words))
    want = queries_by_the_contract(queries, reader.rows_embedding(rows), [0, 4, 6, 46])
    assert same_bits(cosines, want[0]) and reader.last_query_kernel == FUSED
    got = cosines.cpu().numpy()
    assert got[1] == 0 and abs(float(got[2]) - 1) <= 2.0 ** -22 and not got[4:6].any() and (got[6:] != 0).all()
    empty, none = reader.candidates_similarity_device([], [])
    assert tuple(empty.shape) == (0,) and none.cpu().numpy().tolist() == [0]
    # numpy to numpy on the GPU reader and on a device='cpu' reader: the same bits
    host = native.Reader(path, device='cpu')
    batch = query_batch(4, 40, 300, N_ROWS, 5, head=2, tail=3)
    on_gpu = reader.query_similarity(*batch, return_dots=True, return_norms=True)
    on_cpu = host.query_similarity(*batch, return_dots=True, return_norms=True)
    want = queries_by_the_contract(batch[0], reader.rows_embedding(batch[1]), batch[2])
    for one, other, reference in zip((on_gpu[0], on_gpu[1], on_gpu[2][1]), (on_cpu[0], on_cpu[1], on_cpu[2][1]), want):
        assert isinstance(one, np.ndarray) and bits_equal(one, other) and bits_equal(one, reference)
    assert bits_equal(on_gpu[2][0], on_cpu[2][0])
    assert bits_equal(reader.query_similarity(batch[0][0], batch[1]), host.query_similarity(batch[0][0], batch[1]))


def test_query_algorithmic_bytes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, offsets = query_batch(4, 12, 300, N_ROWS, 3, head=2, tail=5)
    cut = offsets.astype(np.uint32)
    lengths = np.diff(offsets)
    entries, non_empty = int(lengths.sum()), int((lengths > 0).sum())
    assert entries == len(rows) - 7 and non_empty < 12
    # what the header says: the pooled count of the groups as bags without the 4 * dim stored per bag, the queries of the
    # groups that are not empty, 4 bytes per output and entry that lies in a group
    pooled = int(reader._impl.pooled_algorithmic_bytes(rows, cut))
    read = pooled - 12 * 4 * 300 + non_empty * 4 * 300
    count = reader._impl.query_algorithmic_bytes
    # by hand where no compressed byte is read: three missing candidates in the first of two groups -- 8 bytes of offsets per
    # group, one query, three ids, three cosines
    missing = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
    assert count(missing, np.array([0, 3, 3], dtype=np.uint32)) == 2 * 8 + 4 * 300 + 3 * 4 + 3 * 4
    assert count(rows, cut) == read + entries * 4
    assert count(rows, cut, True, True, True) == read + entries * 12
    assert count(rows, cut, False, True, False) == read + entries * 4
    assert count(rows, cut, cosines=False, dots=False, norms=True) == read + entries * 4
    assert count(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32)) == 0
    with pytest.raises(ValueError, match='groups \\+ 1'):
        count(rows, cut[:0])


# ---- 5. another stream ----

def test_another_stream_and_no_allocation(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, offsets = query_batch(4, 40, 300, N_ROWS, 31)
    want = queries_by_the_contract(queries, reader.rows_embedding(rows), offsets)
    on_device, cut, vectors = to_device(rows), to_device(offsets), queries_to_device(queries)
    out = torch.empty((len(rows),), dtype=torch.float32, device='cuda')
    reader.query_similarity_device(vectors, on_device, cut, out=out)   # (warm: the model is staged, the kernel loaded)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out.fill_(float(SENTINEL))
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        returned = reader.query_similarity_device(vectors, on_device, cut, out=out)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before   # everything on the device: nothing allocated
        stream.synchronize()
    assert returned.data_ptr() == out.data_ptr() and same_bits(out, want[0]) and reader.last_query_kernel == FUSED
    # offsets=None, the headline case: the two offsets of "one group of all rows" are kept on the device after the first
    # call with this many rows, so the second allocates and copies nothing
    single = vectors[:1]
    whole = queries_by_the_contract(queries[:1], reader.rows_embedding(rows), [0, len(rows)])
    reader.query_similarity_device(single, on_device, out=out)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        reader.query_similarity_device(single, on_device, out=out)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
        stream.synchronize()
    assert same_bits(out, whole[0])


# ---- 6. what Python and the C entry point refuse ----

def test_python_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = to_device(np.arange(10, dtype=np.uint32))
    offsets = to_device(np.array([0, 4, 10]))
    queries = torch.ones((2, 300), dtype=torch.float32, device='cuda')
    call = reader.query_similarity_device
    with pytest.raises(TypeError, match='rows must be'):
        call(queries, rows.cpu(), offsets)                                      # wrong device
    with pytest.raises(TypeError, match='rows must be'):
        call(queries, rows.to(torch.int64), offsets)                            # wrong dtype
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.to(torch.float64), rows, offsets)
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.cpu(), rows, offsets)
    with pytest.raises(TypeError, match='queries must be'):
        call(queries.cpu().numpy(), rows, offsets)
    with pytest.raises(ValueError, match='shape'):
        call(queries[:, :296], rows, offsets)                                   # wrong dim
    with pytest.raises(ValueError, match='shape'):
        call(queries.unsqueeze(0), rows, offsets)
    with pytest.raises(ValueError, match='contiguous last dimension'):
        call(torch.ones((2, 600), dtype=torch.float32, device='cuda')[:, ::2], rows, offsets)
    with pytest.raises(ValueError, match='row stride'):
        call(torch.ones((1, 300), dtype=torch.float32, device='cuda').expand(2, 300), rows, offsets)
    with pytest.raises(TypeError, match='offsets must be'):
        call(queries, rows, offsets.cpu())
    with pytest.raises(TypeError, match='offsets must be'):
        call(queries, rows, offsets.to(torch.int64))
    with pytest.raises(ValueError, match='G \\+ 1'):
        call(queries, rows, offsets[:2].contiguous())
    with pytest.raises(ValueError, match='one query'):
        call(queries, rows)                                                     # offsets=None needs G == 1
    with pytest.raises(TypeError, match='float32'):
        call(queries, rows, offsets, out=torch.empty((10,), dtype=torch.float16, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        call(queries, rows, offsets, out=torch.empty((9,), dtype=torch.float32, device='cuda'))   # wrong size
    with pytest.raises(ValueError, match='must be on cuda'):
        call(queries, rows, offsets, out=torch.empty((10,), dtype=torch.float32))
    with pytest.raises(ValueError, match='one list of candidates per word'):
        reader.candidates_similarity_device(['a'], [])
    # the C entry point's own refusals, with a staged model: nothing is launched (the sentinels stay)
    guard = torch.full((12,), float(SENTINEL), dtype=torch.float32, device='cuda')
    raw = reader._impl.query_similarity_to_device
    q, r, o, g = queries.data_ptr(), rows.data_ptr(), offsets.data_ptr(), guard.data_ptr()
    for arguments, word in (((0, 2, 300, r, 10, o, g, 0, 0, 0), 'null argument'),
                            ((q, 2, 300, r, 10, 0, g, 0, 0, 0), 'null argument'),
                            ((q, 2, 300, 0, 10, o, g, 0, 0, 0), 'null argument'),
                            ((q, 2, 300, r, 10, o, 0, 0, 0, 0), 'at least one'),
                            ((q, 2, 299, r, 10, o, g, 0, 0, 0), 'ld_queries'),
                            ((q, 2, 300, r, 10, o, g + 2, 0, 0, 0), 'aligned'),
                            ((q + 1, 2, 300, r, 10, o, g, 0, 0, 0), 'aligned'),
                            ((q, 2, 300, r, 10, o, 0, 0, g + 1, 0), 'aligned'),
                            ((q, 2, 300, r, 2 ** 36 + 1, o, g, 0, 0, 0), 'too large'),
                            ((q, 2 ** 32 - 1, 300, r, 10, o, g, 0, 0, 0), 'too large')):
        with pytest.raises(RuntimeError, match=word):
            raw(*arguments)
    assert raw(q, 2, 300, 0, 0, o, g, 0, 0, 0) is True    # n == 0: a no-op
    assert raw(0, 0, 300, r, 10, 0, g, 0, 0, 0) is True   # groups == 0: a no-op
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == SENTINEL).all()
    # nothing was launched by a refused call; the reader still answers
    itself = reader.rows_embedding_device(rows[:1])
    assert abs(float(reader.query_similarity_device(itself, rows)[0]) - 1) <= 2.0 ** -22
