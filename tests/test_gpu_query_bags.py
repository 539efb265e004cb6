"""Every query against every pooled bag of rows on the GPU (include/memb_hip_query_bags.h): bag_similarity_matrix_device,
bag_similarity_topk_device and nearest_sentences_device bit for bit against the numpy contract of
tests/query_bags_reference.py, against "bags_embedding_device, then the dense pair kernel" on the same reader, and against
the sibling kernels where their contracts meet this one. Zero tolerance everywhere: the contract is a composition of two
contracts that are pinned bit for bit already."""
import numpy as np
import pytest

from bag_pairs_reference import entry_values
from conftest import bits_equal
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, to_device
from pooled_reference import ids_with_misses, offsets_of, signed_zero_model
from query_bags_reference import bags_batch, queries_batch, query_bags_by_the_contract
from query_topk_reference import same_topk, topk_by_the_contract

pytestmark = pytest.mark.gpu

N_ROWS = 3000
KEY_FORM_ROWS = 20000   # the models of tests/test_gpu_pooled.py (built once per session)
SENTINEL = np.float32(-1234.5)
FUSED = 'query_bags_trained'
DENSE = 'pairs_dense'
MODES = ('sum', 'mean')
POOL_CODE = {'sum': 0, 'mean': 1}   # MEMB_HIP_POOL_SUM, MEMB_HIP_POOL_MEAN
BAG_COUNTS = (1, 2, 3, 13)


def words_per_wave(reader):
    lanes = reader.info()['lanes_per_word']
    return 64 // lanes if lanes else 4


def query_counts():
    from memb_amd import _memb
    block = _memb.QUERY_MATRIX_BLOCK
    return sorted({1, 2, max(block - 1, 1), block, block + 1, 2 * block + 1})


def two_steps(reader, queries, pooled):
    """the second oracle: (cosines, dots, norms) of every query beside every pooled row through the dense pair kernel"""
    import torch
    from memb_amd import _memb
    count, bags, dim = queries.shape[0], pooled.shape[0], reader.dim
    stream = torch.cuda.current_stream().cuda_stream
    cosines = torch.zeros((count, bags), dtype=torch.float32, device='cuda')
    dots = torch.zeros((count, bags), dtype=torch.float32, device='cuda')
    norms = torch.zeros((bags, 2), dtype=torch.float32, device='cuda')
    side = torch.empty((bags, 2, dim), dtype=torch.float32, device='cuda')
    side[:, 1] = pooled
    for q in range(count):
        side[:, 0] = queries[q]
        _memb.dense_pair_similarity_to_device(
            0, side.data_ptr(), bags, dim, dim, cosines[q].data_ptr(), dots[q].data_ptr(), norms.data_ptr(), stream)
    return cosines, dots, norms[:, 1].contiguous()


def check_query_bags(reader, queries, rows, offsets, mode, context, kernel, want=None):
    """bag_similarity_matrix_device in every output combination against the contract and against the two-step oracle; each
    output alone through the raw binding between sentinels; `out` with a row stride of bags + 3 between sentinels and above
    a guard row; last_query_bags_kernel is `kernel`. Returns the contract's (cosines, dots, norms)."""
    import torch
    rows = np.asarray(rows, dtype=np.uint32)
    offsets = np.asarray(offsets)
    count, bags = queries.shape[0], len(offsets) - 1
    if want is None:
        want = query_bags_by_the_contract(queries, entry_values(reader, rows), offsets, mode)
    on_device, cut, asked = to_device(rows), to_device(offsets), torch.from_numpy(queries).cuda()

    cosines = reader.bag_similarity_matrix_device(asked, on_device, cut, mode)
    assert cosines.dtype == torch.float32 and tuple(cosines.shape) == (count, bags) and cosines.is_cuda, context
    assert reader.last_query_bags_kernel == kernel, (context, reader.last_query_bags_kernel)
    if not same_bits(cosines, want[0]):
        bad = np.argwhere(cosines.cpu().numpy().view(np.uint32) != want[0].view(np.uint32))
        raise AssertionError('{}: {} of {} cosines differ, first {}'.format(context, len(bad), count * bags, bad[:8].tolist()))
    for dots, norms in ((True, False), (False, True), (True, True)):
        got = reader.bag_similarity_matrix_device(asked, on_device, cut, mode=mode, return_dots=dots, return_norms=norms)
        assert len(got) == 3 and same_bits(got[0], want[0]), (context, dots, norms)
        assert (got[1] is None) == (not dots) and (got[2] is None) == (not norms), (context, dots, norms)
        if dots:
            assert tuple(got[1].shape) == (count, bags) and same_bits(got[1], want[1]), (context, dots, norms, 'dots')
        if norms:
            assert tuple(got[2][1].shape) == (bags,) and same_bits(got[2][1], want[2]), (context, dots, norms, 'norms')
            assert tuple(got[2][0].shape) == (count,), context
    # the second oracle: the pooled rows of this reader through the dense pair kernel
    if bags and count:
        pooled = reader.bags_embedding_device(on_device, cut, mode=mode)
        second = two_steps(reader, asked, pooled)
        for name, got, wanted in zip(('cosines', 'dots', 'norms'), second, want):
            assert same_bits(got, wanted), (context, 'two steps', name)
    stream = torch.cuda.current_stream().cuda_stream
    if kernel == FUSED and bags and count:
        arguments = (asked.data_ptr(), count, reader.dim, on_device.data_ptr(), len(rows), cut.data_ptr(), bags, POOL_CODE[mode])
        for which in range(3):   # cosines alone, dots alone, norms alone
            size = bags if which == 2 else count * bags
            alone = torch.full((size + 2,), float(SENTINEL), dtype=torch.float32, device='cuda')
            pointers = [0, 0, 0]
            pointers[which] = alone[1:].data_ptr()
            assert reader._impl.query_bags_to_device(*arguments, pointers[0], pointers[1], bags, pointers[2], stream)
            host = alone.cpu().numpy()
            assert host[0] == SENTINEL and host[-1] == SENTINEL and bits_equal(host[1:-1], want[which].reshape(-1)), (context, 'alone', which)
    # into a caller's tensor: rows bags + 3 floats apart, a guard row below
    frame = torch.full((count + 1, bags + 3), float(SENTINEL), dtype=torch.float32, device='cuda')
    view = frame[:count, 1:bags + 1]
    returned = reader.bag_similarity_matrix_device(asked, on_device, cut, mode, out=view)
    assert returned.data_ptr() == view.data_ptr(), context
    host = frame.cpu().numpy()
    assert bits_equal(host[:count, 1:bags + 1], want[0]), (context, 'out')
    host[:count, 1:bags + 1] = SENTINEL
    assert (host == SENTINEL).all(), (context, 'out: written outside')
    return want


def sweep(reader, context, kernel, n_rows=N_ROWS, bag_counts=BAG_COUNTS, counts=None, modes=MODES):
    words = words_per_wave(reader)
    for bags in bag_counts:
        rows, offsets = bags_batch(words, bags, n_rows, 11 + bags)
        values = entry_values(reader, rows)
        for count in counts or query_counts():
            queries = queries_batch(count, reader.dim, count, values)
            for mode in modes:
                want = check_query_bags(reader, queries, rows, offsets, mode, (context, bags, count, mode), kernel,
                                        want=query_bags_by_the_contract(queries, values, offsets, mode))
                assert (want[0] != 0).any(), (context, bags, count, mode)


# ---- 1. the three key forms, row layouts, lanes per word and block sizes ----

FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    def check(reader, context):
        assert reader._impl.query_bags_kernel_name() == FUSED, context   # one word per wavefront (MEMB_HIP_LANES=64) included
        FORMS_REACHED.add(kernel_form(reader))
        # 25 bags: every length of the draw, the bag of 300 entries, several wavefronts; the query counts around a block
        sweep(reader, context, FUSED, n_rows=KEY_FORM_ROWS, bag_counts=(25,), counts=(1, 5), modes=('mean',))
        sweep(reader, context, FUSED, n_rows=KEY_FORM_ROWS, bag_counts=(3,), counts=(2,), modes=('sum',))

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


# ---- 2. the fused path: query counts around a block, bag counts around a group, dims with one and two pieces per lane ----

@pytest.mark.parametrize('dim,bits', [(4, 4), (300, 4), (300, 6), (260, 6), (512, 4)])
def test_sweep_of_queries_and_bags(native, make_model, dim, bits):
    path, _ = make_model(N_ROWS, dim, 'trained', bits)
    reader = native.Reader(path)
    assert reader._impl.query_bags_kernel_name() == FUSED
    sweep(reader, (dim, bits), FUSED)


def test_many_bags_and_queries_over_several_stores(native, make_model):
    # 140 bags (many wavefronts and groups, the long bag) against 67 queries: more than the 64 / G queries of one store
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    sweep(reader, 'many', FUSED, bag_counts=(140,), counts=(67,), modes=('mean',))


def test_one_word_per_wavefront_and_an_odd_number(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=64)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 1 and reader._impl.query_bags_kernel_name() == FUSED
    sweep(reader, 'one word per wavefront', FUSED, bag_counts=(3, 13), counts=(1, 3))
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7, reader.info()['lanes_per_word']
    sweep(reader, 'seven words per wavefront', FUSED, bag_counts=(13,), counts=(3,))


def test_launch_options_never_change_a_bit(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bags_batch(words_per_wave(reader), 40, N_ROWS, 5)
    queries = queries_batch(5, 300, 5, entry_values(reader, rows))
    want = query_bags_by_the_contract(queries, entry_values(reader, rows), offsets, 'mean')
    arguments = (torch.from_numpy(queries).cuda(), to_device(rows), to_device(offsets), 'mean')
    for waves in (1, 2, 7):
        for tiles in (1, 2, 64):
            reader.set_option('waves_per_block', waves)
            reader.set_option('tiles_per_wave', tiles)
            got = reader.bag_similarity_matrix_device(*arguments, return_dots=True, return_norms=True)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2][1], want[2]), (waves, tiles)


# ---- 3. the third oracle: the sibling kernels where the contracts meet ----

def test_bags_of_one_entry_are_the_query_matrix(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 6)
    reader = native.Reader(path)
    rows = ids_with_misses(37, N_ROWS, 3)
    queries = torch.from_numpy(queries_batch(5, 300, 3, entry_values(reader, rows))).cuda()
    on_device = to_device(rows)
    matrix = reader.similarity_matrix_device(queries, on_device, return_dots=True, return_norms=True)
    assert reader.last_query_matrix_kernel == 'query_matrix_trained'
    got = reader.bag_similarity_matrix_device(queries, on_device, to_device(np.arange(38)), 'sum', return_dots=True, return_norms=True)
    assert reader.last_query_bags_kernel == FUSED
    assert same_bits(got[0], matrix[0]) and same_bits(got[1], matrix[1])
    assert same_bits(got[2][0], matrix[2][0]) and same_bits(got[2][1], matrix[2][1])


def test_a_pooled_bag_as_the_query_is_the_bag_pair(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bags_batch(words_per_wave(reader), 12, N_ROWS, 9)
    on_device, cut = to_device(rows), to_device(offsets)
    for mode in MODES:
        pooled = reader.bags_embedding_device(on_device, cut, mode=mode)
        matrix = reader.bag_similarity_matrix_device(pooled, on_device, cut, mode).cpu().numpy()
        # pair j of the bag-pair call: the bags 2j and 2j + 1
        pairs = reader.bag_pair_similarity_device(on_device, cut, mode).cpu().numpy()
        assert reader.last_bag_pairs_kernel == 'bag_pairs_trained'
        assert bits_equal(pairs, np.array([matrix[2 * j, 2 * j + 1] for j in range(6)], dtype=np.float32)), mode


# ---- 4. queries with a stride and at an unaligned start; offsets that overrun or descend ----

def test_strided_and_unaligned_queries(native, make_model):
    import torch
    for dim in (300, 512):
        path, _ = make_model(N_ROWS, dim, 'trained', 4)
        reader = native.Reader(path)
        rows, offsets = bags_batch(words_per_wave(reader), 13, N_ROWS, 2)
        queries = queries_batch(5, dim, 2, entry_values(reader, rows))
        want = query_bags_by_the_contract(queries, entry_values(reader, rows), offsets, 'mean')
        for stride, shift in ((dim + 8, 0), (dim + 3, 1), (dim, 3)):
            flat = torch.zeros((5 * stride + shift + 4,), dtype=torch.float32, device='cuda')
            view = torch.as_strided(flat, (5, dim), (stride, 1), shift)
            view.copy_(torch.from_numpy(queries))
            got = reader.bag_similarity_matrix_device(view, to_device(rows), to_device(offsets), 'mean')
            assert same_bits(got, want[0]), (dim, stride, shift)


def test_offsets_that_overrun_or_descend(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(50, N_ROWS, 4)
    rows[:10] %= N_ROWS
    queries = queries_batch(3, 300, 4, entry_values(reader, rows))
    for offsets in ([0, 10, 30, 70, 90, 0xFFFFFFFF], [0, 20, 12, 40, 40, 50], [5, 3, 60, 2, 50]):
        for mode in MODES:
            check_query_bags(reader, queries, rows, np.array(offsets, dtype=np.int64), mode, (offsets, mode), FUSED)


def test_no_entry_no_bag_no_query(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    queries = torch.from_numpy(queries_batch(3, 300, 1)).cuda()
    empty = torch.empty((0,), dtype=torch.int32, device='cuda')
    got = reader.bag_similarity_matrix_device(queries, empty, to_device(np.zeros(5)), return_dots=True, return_norms=True)
    assert tuple(got[0].shape) == (3, 4) and not got[0].cpu().numpy().view(np.uint32).any()   # empty bags: +0.0
    assert not got[1].cpu().numpy().view(np.uint32).any() and not got[2][1].cpu().numpy().view(np.uint32).any()
    assert tuple(reader.bag_similarity_matrix_device(queries, empty, to_device(np.zeros(1))).shape) == (3, 0)
    rows, offsets = bags_batch(4, 5, N_ROWS, 1)
    none = reader.bag_similarity_matrix_device(queries[:0], to_device(rows), to_device(offsets), return_norms=True)
    want = query_bags_by_the_contract(np.zeros((0, 300), dtype=np.float32), entry_values(reader, rows), offsets, 'mean')
    assert tuple(none[0].shape) == (0, 5) and same_bits(none[2][1], want[2])


# ---- 5. models without the fused kernel: pooled in slices, the dense pair kernel, the same bits ----

@pytest.mark.parametrize('storage,bits,dim', [('uniform', 8, 300), ('full', 8, 300), ('trained', 4, 7), ('trained', 4, 302)])
def test_fallback_models(native, make_model, monkeypatch, storage, bits, dim):
    import memb_amd.reader
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    assert reader._impl.query_bags_kernel_name() == '' and reader._impl.query_bags_topk_kernel_name() == ''
    sweep(reader, (storage, dim), DENSE, bag_counts=(3, 13), counts=(1, 3))
    monkeypatch.setattr(memb_amd.reader, 'QUERY_BAGS_DEVICE_SLICE', 4)   # 13 bags: four slices, rebased offsets
    sweep(reader, (storage, dim, 'slices'), DENSE, bag_counts=(13,), counts=(3,))
    rows, offsets = bags_batch(4, 13, N_ROWS, 6)
    queries = queries_batch(3, dim, 6, entry_values(reader, rows))
    import torch
    want = topk_by_the_contract(query_bags_by_the_contract(queries, entry_values(reader, rows), offsets, 'mean')[0], 10)
    got = reader.bag_similarity_topk_device(torch.from_numpy(queries).cuda(), to_device(rows), to_device(offsets), 10)
    assert same_topk(tuple(part.cpu().numpy() for part in got), want)
    assert reader.last_query_bags_topk_kernel == 'pairs_dense+topk_select+topk_merge'


def test_signed_zero_bags(native, tmp_path):
    # rows of -0.0 and of subnormals with mixed signs: -0.0 products reach the lane partials, sums of zeros keep their sign
    path, count = signed_zero_model(native, tmp_path)
    reader = native.Reader(path)
    rows = np.array([0, 0, 1, 2, 0, 1, 0xFFFFFFFF, 0, 2, 2, 1, 0], dtype=np.uint32)
    offsets = np.array([0, 2, 3, 4, 6, 8, 8, 12])
    queries = np.concatenate([reader.rows_embedding(np.array([0, 1, 2], dtype=np.uint32)), -reader.rows_embedding(np.array([1], dtype=np.uint32))])
    for mode in MODES:
        check_query_bags(reader, queries, rows, offsets, mode, ('signed zeros', mode), DENSE)


# ---- 6. top-k ----

def corpus_with_ties(reader, bags, seed):
    """`bags` bags of 1 .. 5 entries; every third bag repeats the bag before it, so equal cosines meet in every query's order"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 6, size=bags)
    for b in range(2, bags, 3):
        lengths[b] = lengths[b - 1]
    offsets = offsets_of(lengths)
    rows = rng.integers(0, len(reader), size=int(offsets[-1])).astype(np.uint32)
    for b in range(2, bags, 3):
        rows[offsets[b]:offsets[b + 1]] = rows[offsets[b - 1]:offsets[b]]
    return rows, offsets


@pytest.fixture(scope='module')
def topk_reader(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    return native.Reader(path)


@pytest.mark.parametrize('k', (1, 10, 64))
def test_topk_is_the_stable_sort_of_the_matrix(topk_reader, k):
    import torch
    reader = topk_reader
    queries = torch.from_numpy(queries_batch(5, 300, k)).cuda()
    for bags in sorted({0, 1, max(k - 1, 0), k, k + 1, 1100}):
        rows, offsets = corpus_with_ties(reader, bags, bags + k) if bags else (np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.int64))
        on_device, cut = to_device(rows), to_device(offsets)
        values, positions = reader.bag_similarity_topk_device(queries, on_device, cut, k)
        assert reader.last_query_bags_topk_kernel == 'query_bags_trained+topk_select+topk_merge'
        assert tuple(values.shape) == (5, k) and positions.dtype == torch.int64
        matrix = reader.bag_similarity_matrix_device(queries, on_device, cut)
        found = min(k, bags)
        ordered = torch.sort(matrix, dim=1, descending=True, stable=True)
        assert torch.equal(positions[:, :found], ordered.indices[:, :found]), (k, bags)
        assert same_bits(values[:, :found].contiguous(), ordered.values[:, :found].contiguous()), (k, bags)
        assert (positions[:, found:] == -1).all() and torch.isneginf(values[:, found:]).all(), (k, bags)
        assert same_topk((values.cpu().numpy(), positions.cpu().numpy()), topk_by_the_contract(matrix.cpu().numpy(), k)), (k, bags)
        if bags > 3:   # bag 2 repeats bag 1: wherever both are kept, the lower index comes first
            host = positions.cpu().numpy()
            for q in range(5):
                both = [int(np.nonzero(host[q] == b)[0][0]) for b in (1, 2) if (host[q] == b).any()]
                assert len(both) < 2 or both[0] + 1 == both[1], (k, bags, q)
        if bags == 1100:
            # the minimal workspace: slices of 64 bags, eighteen of them, the same bits; an output wider than k keeps its padding
            from memb_amd import _memb
            needed = reader._impl.query_bags_topk_workspace_bytes(5, bags, k, minimal=True)
            assert needed < reader._impl.query_bags_topk_workspace_bytes(5, bags, k) and _memb.QUERY_TOPK_MIN_SLICE == 64
            small = torch.empty((needed,), dtype=torch.uint8, device='cuda')
            again = reader.bag_similarity_topk_device(queries, on_device, cut, k, workspace=small)
            assert torch.equal(again[1], positions) and same_bits(again[0], values), k
            wide_values = torch.full((5, k + 3), float(SENTINEL), dtype=torch.float32, device='cuda')
            wide_positions = torch.full((5, k + 3), -77, dtype=torch.int64, device='cuda')
            assert reader._impl.query_bags_topk_to_device(
                queries.data_ptr(), 5, 300, on_device.data_ptr(), len(rows), cut.data_ptr(), bags, POOL_CODE['mean'], k,
                wide_values.data_ptr(), wide_positions.data_ptr(), k + 3, small.data_ptr(), needed, torch.cuda.current_stream().cuda_stream)
            assert torch.equal(wide_positions[:, :k], positions) and same_bits(wide_values[:, :k].contiguous(), values)
            assert (wide_positions[:, k:] == -77).all() and (wide_values[:, k:] == float(SENTINEL)).all()


def test_topk_of_an_all_empty_corpus_and_the_sum(topk_reader):
    import torch
    reader = topk_reader
    queries = torch.from_numpy(queries_batch(3, 300, 8)).cuda()
    empty = torch.empty((0,), dtype=torch.int32, device='cuda')
    values, positions = reader.bag_similarity_topk_device(queries, empty, to_device(np.zeros(8)), 10)
    assert positions[:, :7].cpu().tolist() == [list(range(7))] * 3 and (positions[:, 7:] == -1).all()   # ties of +0.0: index order
    assert not values[:, :7].contiguous().cpu().numpy().view(np.uint32).any() and torch.isneginf(values[:, 7:]).all()
    rows, offsets = corpus_with_ties(reader, 200, 1)
    want = topk_by_the_contract(query_bags_by_the_contract(queries.cpu().numpy(), entry_values(reader, rows), offsets, 'sum')[0], 10)
    got = reader.bag_similarity_topk_device(queries, to_device(rows), to_device(offsets), 10, mode='sum')
    assert same_topk(tuple(part.cpu().numpy() for part in got), want)
    none = reader.bag_similarity_topk_device(queries[:0], to_device(rows), to_device(offsets), 10)
    assert tuple(none[0].shape) == (0, 10) and reader.last_query_bags_topk_kernel == ''


# ---- 7. sentences, host arrays ----

def test_nearest_sentences_is_the_composition_of_its_parts(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rng = np.random.default_rng(3)
    corpus = [[words[int(i)] for i in rng.integers(0, N_ROWS, size=int(length))] for length in rng.integers(0, 9, size=12)]
    corpus[3] = corpus[3] + ['no such word é']
    corpus[5] = []
    corpus[7] = list(corpus[2])
    asked = [corpus[2], [words[1], 'no such word é', words[2]], []]
    for mode in MODES:
        values, positions = reader.nearest_sentences_device(asked, corpus, k=5, mode=mode)
        from memb_amd.reader import flatten_sentences
        flat, offsets = flatten_sentences(corpus)
        queries = reader.sentences_embedding_device(asked, mode=mode)
        want = reader.bag_similarity_topk_device(queries, reader.resolve_rows_device(flat), to_device(offsets), 5, mode=mode)
        assert torch.equal(positions, want[1]) and same_bits(values, want[0]), mode
        assert positions[0, :2].cpu().tolist() == [2, 7], mode   # the sentence itself and its copy, lower index first
        host = reader.bag_similarity_topk(queries.cpu().numpy(), reader.resolve_rows(flat), offsets, 5, mode=mode)
        assert same_topk(host, (values.cpu().numpy(), positions.cpu().numpy())), mode
    matrix = reader.bag_similarity_matrix(queries.cpu().numpy(), reader.resolve_rows(flat), offsets, mode='sum', return_dots=True, return_norms=True)
    on_device = reader.bag_similarity_matrix_device(queries, reader.resolve_rows_device(flat), to_device(offsets), 'sum', return_dots=True, return_norms=True)
    assert same_bits(on_device[0], matrix[0]) and same_bits(on_device[1], matrix[1])
    assert same_bits(on_device[2][0], matrix[2][0]) and same_bits(on_device[2][1], matrix[2][1])


def test_algorithmic_bytes(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = bags_batch(4, 13, N_ROWS, 1)
    from memb_amd import _memb
    pooled = reader._impl.pooled_algorithmic_bytes(rows, offsets.astype(np.uint32), _memb.OUT_F32)
    without = pooled - 13 * 4 * 300
    assert reader._impl.query_bags_algorithmic_bytes(rows, offsets.astype(np.uint32), 5) == without + 5 * 1200 + 5 * 13 * 4
    assert reader._impl.query_bags_algorithmic_bytes(rows, offsets.astype(np.uint32), 5, True, True, True) == without + 5 * 1200 + 5 * 13 * 8 + 13 * 4


def test_python_refusals_on_the_device(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = to_device(np.arange(9)), to_device(np.array([0, 4, 9]))
    queries = torch.zeros((3, 300), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='mode'):
        reader.bag_similarity_matrix_device(queries, rows, offsets, 'max')
    with pytest.raises(TypeError, match='float32'):
        reader.bag_similarity_matrix_device(queries.double(), rows, offsets)
    with pytest.raises(ValueError, match='shape'):
        reader.bag_similarity_matrix_device(queries[:, :296], rows, offsets)
    with pytest.raises(TypeError, match='offsets'):
        reader.bag_similarity_matrix_device(queries, rows, offsets.cpu())
    with pytest.raises(TypeError, match='offsets'):
        reader.bag_similarity_matrix_device(queries, rows, offsets.to(torch.int64))
    with pytest.raises(ValueError, match='bags \\+ 1'):
        reader.bag_similarity_matrix_device(queries, rows, offsets[:0])
    with pytest.raises(TypeError, match='out'):
        reader.bag_similarity_matrix_device(queries, rows, offsets, out=torch.zeros((3, 3), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError, match='stride'):
        reader.bag_similarity_matrix_device(queries, rows, offsets, out=torch.zeros((2, 3), dtype=torch.float32, device='cuda').t())
    with pytest.raises(TypeError, match='rows'):
        reader.bag_similarity_matrix_device(queries, rows.cpu(), offsets)
    for k in (0, 65):
        with pytest.raises(ValueError, match='64'):
            reader.bag_similarity_topk_device(queries, rows, offsets, k)
    with pytest.raises(ValueError, match='64'):
        reader.nearest_sentences_device([['a']], [['b']], k=65)
    with pytest.raises(TypeError, match='workspace'):
        reader.bag_similarity_topk_device(queries, rows, offsets, 3, workspace=torch.zeros((64,), dtype=torch.float32, device='cuda'))
    with pytest.raises(RuntimeError, match='workspace too small'):
        reader.bag_similarity_topk_device(queries, rows, offsets, 3, workspace=torch.zeros((8,), dtype=torch.uint8, device='cuda'))


# ---- 8. a captured graph ----

def test_topk_captured_into_a_graph(native, make_model, topk_reader):
    """bag_similarity_topk_device with a caller's workspace allocates nothing but its results: captured on one stream (a
    single chain of launches, five slices of 256 bags), then replayed once over other queries written in place -- rows of
    the model that are bags of one entry themselves, each repeated by the bag behind it; the answer is a host reader's"""
    import torch
    reader = topk_reader
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    host = native.Reader(path, device='cpu')
    bags, count, k = 1100, 5, 10
    rows, offsets = corpus_with_ties(reader, bags, 91)
    singles = [b for b in range(1, bags, 3) if offsets[b + 1] - offsets[b] == 1][:count]   # (bag b + 1 repeats bag b)
    assert len(singles) == count
    others = host.rows_embedding(rows[offsets[singles]])
    on_device, cut = to_device(rows), to_device(offsets)
    queries = torch.from_numpy(queries_batch(count, 300, 92)).cuda()
    least = reader._impl.query_bags_topk_workspace_bytes(count, bags, k, minimal=True)
    workspace = torch.empty((least + 4 * count * 192,), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        reader.bag_similarity_topk_device(queries, on_device, cut, k, workspace=workspace)   # (warm-up)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        values, positions = reader.bag_similarity_topk_device(queries, on_device, cut, k, workspace=workspace)
    queries.copy_(torch.from_numpy(others))
    values.fill_(float(SENTINEL))
    positions.fill_(-77)
    graph.replay()
    torch.cuda.synchronize()
    want = host.bag_similarity_topk(others, rows, offsets, k)
    for q, b in enumerate(singles):
        assert want[1][q, :2].tolist() == [b, b + 1] and want[0][q, 0].view(np.uint32) == want[0][q, 1].view(np.uint32)
    assert same_topk((values.cpu().numpy(), positions.cpu().numpy()), want)
