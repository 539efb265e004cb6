"""3CosMul on the GPU: cosmul_scores alone over a dense matrix of cosines (between sentinels), the fused call in every key
form and geometry against the restatement of tests/cosmul_reference.py over similarity_matrix_device's matrix, under the
recommended, the minimal and a dirty workspace, with and without exclusion lists, a uniform model through the fallback, the
word-level calls against their pieces and against a device='cpu' reader, and the refusals. Every comparison is bit for bit."""
import numpy as np
import pytest

from analogies_reference import topk_excluding_by_the_contract
from cosmul_reference import EPSILON, cosmul_scores_by_the_contract, questions_of
from pooled_device import ALL_KEY_FORMS, KEY_FORM_MODELS, for_every_key_form, kernel_form, same_bits, set_environment, to_device
from pooled_reference import ids_with_misses
from query_topk_reference import same_topk, topk_by_the_contract
from test_gpu_analogies import lists_to_device, two_segments
from test_gpu_queries import KEY_FORM_ROWS, N_ROWS, queries_to_device, words_per_wave
from test_gpu_query_topk import SENTINEL, SENTINEL_POSITION, tied_candidates

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained+cosmul_scores+topk_select_excluding+topk_merge'
DENSE = 'pairs_dense+cosmul_scores+topk_select_excluding+topk_merge'
# (positive, negative) terms of the questions of one launch; one without any term first, in the middle and last
PAIRS = ((0, 0), (1, 0), (0, 1), (0, 0), (2, 1), (1, 2), (3, 61), (64, 0), (0, 0))
COLUMNS = (1, 63, 64, 65, 1100)
EMPTY_SCORE = np.float32(1) / np.float32(np.float32(1) + EPSILON)


def cosmul():
    from memb_amd import _memb_cosmul
    return _memb_cosmul


def questions_to_device(offsets, negatives_from):
    import torch
    return torch.from_numpy(np.asarray(offsets, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(negatives_from, dtype=np.int32)).cuda()


# ---- 1. the kernel alone ----

@pytest.fixture(scope='module')
def cosines_and_scores():
    """(cosines float32 (T, 1100), offsets, negatives_from, the reference scores (9, 1100)): random cosines with -1, +1,
    values just outside, NaN and both zeros in the first columns and scattered; worked out once"""
    offsets, negatives_from, terms = questions_of(PAIRS)
    rng = np.random.default_rng(51)
    cosines = rng.uniform(-1, 1, size=(terms, max(COLUMNS))).astype(np.float32)
    special = np.array([0.25, -1.0, 1.0, np.float32(1) + np.float32(2.0 ** -23), np.nan, 0.0, -0.0, np.float32(-1) - np.float32(2.0 ** -23)],
                       dtype=np.float32)
    cosines[:, 1:8] = special[1:]
    cosines[rng.integers(0, terms, 40), rng.integers(8, max(COLUMNS), 40)] = rng.choice(special, 40)
    cosines[5, 8:12] = special[[4, 1, 5, 6]]   # (among the terms of (2, 1) and (1, 2): one special value, the others ordinary)
    with np.errstate(invalid='ignore'):
        scores = cosmul_scores_by_the_contract(cosines, offsets, negatives_from)
    assert np.isnan(scores).any() and (scores == 0).any() and (scores > 1e5).any()
    return cosines, offsets, negatives_from, scores


def cosmul_scores(cosines, offsets, negatives_from, spare=3, spare_scores=5):
    """_memb_cosmul.cosmul_scores_to_device on a host matrix: rows n + spare floats apart on the device with NaN behind them, the
    scores n + spare_scores apart between sentinels and above a guard row, which must all survive"""
    import torch
    terms, n = cosines.shape
    count = len(negatives_from)
    on_device = torch.full((terms + 1, n + spare), float('nan'), dtype=torch.float32, device='cuda')
    on_device[:terms, :n] = torch.from_numpy(np.ascontiguousarray(cosines)).cuda()
    scores = torch.full((count + 1, n + spare_scores), SENTINEL, dtype=torch.float32, device='cuda')
    device_offsets, device_negatives = questions_to_device(offsets, negatives_from)
    cosmul().cosmul_scores_to_device(
        0, on_device.data_ptr(), n + spare, device_offsets.data_ptr(), device_negatives.data_ptr(), count, n, scores.data_ptr(),
        n + spare_scores, torch.cuda.current_stream().cuda_stream)
    got = scores.cpu().numpy()
    assert (got[:count, n:] == np.float32(SENTINEL)).all() and (got[count] == np.float32(SENTINEL)).all()
    return np.ascontiguousarray(got[:count, :n])


@pytest.mark.parametrize('n', COLUMNS)
def test_the_kernel_alone(native, cosines_and_scores, n):
    cosines, offsets, negatives_from, want = cosines_and_scores
    # every question in one launch
    got = cosmul_scores(cosines[:, :n], offsets, negatives_from)
    for q, pair in enumerate(PAIRS):
        assert same_bits(got[q], want[q, :n]), (n, q, pair)
    assert (got[[0, 3, 8]] == EMPTY_SCORE).all()
    # five questions of the same matrix, the first not at term 0, and tight rows (ld == n)
    five = cosmul_scores(cosines[:, :n], offsets[1:7], negatives_from[1:6], spare=0, spare_scores=0)
    assert same_bits(five, want[1:6, :n]), n
    # one question: without any term, with 64 terms in the one order and in the other
    for q in (3, 6, 7):
        one = cosmul_scores(cosines[:, :n], offsets[q:q + 2], negatives_from[q:q + 1])
        assert same_bits(one, want[q:q + 1, :n]), (n, q)


@pytest.mark.parametrize('n', COLUMNS)
def test_one_positive_term_alone(native, cosines_and_scores, n):
    # (64 terms in one launch of their own are above: questions 6 and 7; the question of a single positive term is not)
    cosines, offsets, negatives_from, want = cosines_and_scores
    assert PAIRS[1] == (1, 0) and offsets[2] - offsets[1] == 1 and negatives_from[1] == offsets[2]
    one = cosmul_scores(cosines[:, :n], offsets[1:3], negatives_from[1:2])
    assert same_bits(one, want[1:2, :n]), n
    # score = ((1 + c) * 0.5) / (1 + 1e-6): one rounded operation each
    c = cosines[offsets[1], :n]
    with np.errstate(invalid='ignore'):
        by_hand = ((np.float32(1) + c) * np.float32(0.5)) / (np.float32(1) + EPSILON)
    assert same_bits(one[0], by_hand.astype(np.float32)), n


def test_nothing_to_score_is_a_no_op(native):
    import torch
    scores = torch.full((3, 9), SENTINEL, dtype=torch.float32, device='cuda')
    device_offsets, device_negatives = questions_to_device([0, 0, 0], [0, 0])
    stream = torch.cuda.current_stream().cuda_stream
    cosmul().cosmul_scores_to_device(0, scores.data_ptr(), 9, device_offsets.data_ptr(), device_negatives.data_ptr(), 0, 9, scores.data_ptr(), 9, stream)
    cosmul().cosmul_scores_to_device(0, 0, 0, device_offsets.data_ptr(), device_negatives.data_ptr(), 2, 0, scores.data_ptr(), 9, stream)
    assert (scores.cpu().numpy() == np.float32(SENTINEL)).all()


# ---- 2. the fused call ----

QUESTIONS = ((2, 1), (0, 0), (1, 0), (0, 2), (3, 2))   # an analogy, no term, one positive, negatives only, five terms


def nearest_with_workspace(reader, terms, questions, on_device, k, lists, minimal, spare=2, fill=0x7FC00001):
    """the raw call with a dirty workspace of exactly the minimal or the recommended size, outputs between sentinels"""
    import torch
    offsets, negatives_from = questions
    count, n_terms, n = len(negatives_from), terms.shape[0], on_device.numel()
    needed = cosmul().query_cosmul_workspace_bytes(reader._impl.context_handle(), n_terms, count, n, k, minimal)
    workspace = torch.full((needed // 4 + 2,), fill, dtype=torch.int32, device='cuda')
    values = torch.full((count + 1, k + spare), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((count + 1, k + spare), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    keep, pointer, ld_excluded = lists_to_device(lists) if lists is not None else (None, 0, 0)
    device_offsets, device_negatives = questions_to_device(offsets, negatives_from)
    assert cosmul().query_cosmul_nearest_to_device(
        reader._impl.context_handle(), terms.data_ptr() if n_terms else 0, n_terms, terms.stride(0) if n_terms > 1 else reader.dim, device_offsets.data_ptr(),
        device_negatives.data_ptr(), count, on_device.data_ptr() if n else 0, n, k, pointer, 0 if lists is None else lists.shape[1],
        ld_excluded, values.data_ptr(), positions.data_ptr(), k + spare, workspace.data_ptr() if needed else 0, needed,
        torch.cuda.current_stream().cuda_stream)
    got_values, got_positions = values.cpu().numpy(), positions.cpu().numpy()
    assert (got_values[:count, k:] == np.float32(SENTINEL)).all() and (got_values[count] == np.float32(SENTINEL)).all()
    assert (got_positions[:count, k:] == SENTINEL_POSITION).all() and (got_positions[count] == SENTINEL_POSITION).all()
    assert (workspace[needed // 4:].cpu().numpy() == fill).all()
    return np.ascontiguousarray(got_values[:count, :k]), np.ascontiguousarray(got_positions[:count, :k])


def check_fused(reader, n_rows, context, ranks=(10,)):
    import torch
    offsets, negatives_from, n_terms = questions_of(QUESTIONS)
    n = two_segments()   # two segments under the recommended workspace, eighteen slices under the minimal
    rows = tied_candidates(n, n_rows, 61)
    term_rows = ids_with_misses(n_terms, n_rows, 62)
    term_rows[:3] = rows[[5, 70, 200]] % np.uint32(n_rows)   # the analogy's words are candidates themselves
    on_device = to_device(rows)
    terms = queries_to_device(reader.unit_rows_embedding_device(to_device(term_rows)).cpu().numpy(), ld=reader.dim + 3, shift=1)
    matrix = reader.similarity_matrix_device(terms, on_device).cpu().numpy()
    assert (matrix != 0).any()
    scores = cosmul_scores_by_the_contract(matrix, offsets, negatives_from)
    # each question's list: three of its best (tied candidates: in different slices of 64), a column of the first and of
    # the last slice, padding; one question's list is all padding
    best = topk_by_the_contract(scores, 64)[1]
    lists = np.concatenate([best[:, [0, 2, 5]], np.broadcast_to(np.array([3, n - 1, -1]), (len(QUESTIONS), 3))], axis=1).astype(np.int64)
    lists[3] = -1
    lists[0, :3] = best[0, [0, 10, 40]]
    assert len({int(p) // 64 for p in lists[0] if p >= 0}) >= 3   # (candidates of different slices)
    questions = (offsets, negatives_from)
    for k in ranks:
        for given in (None, lists):
            want = topk_excluding_by_the_contract(scores, k, given)
            least = nearest_with_workspace(reader, terms, questions, on_device, k, given, minimal=True)
            recommended = nearest_with_workspace(reader, terms, questions, on_device, k, given, minimal=False)
            assert same_topk(least, recommended), (context, k, 'minimal against recommended workspace')
            assert same_topk(least, want), (context, k, given is None)
        # a workspace dirty in another way (finite values, columns out of range): the same bits
        other = nearest_with_workspace(reader, terms, questions, on_device, k, lists, minimal=True, fill=0x4F000000)
        assert same_topk(other, want), (context, k, 'another dirt')
    # one question alone, and the questions beyond the first over the same terms
    alone = nearest_with_workspace(reader, terms[:3], (offsets[:2], negatives_from[:1]), on_device, 10, lists[:1], minimal=False)
    assert same_topk(alone, topk_excluding_by_the_contract(scores[:1], 10, lists[:1])), context
    rest = nearest_with_workspace(reader, terms, (offsets[1:], negatives_from[1:]), on_device, 10, lists[1:], minimal=True)
    assert same_topk(rest, topk_excluding_by_the_contract(scores[1:], 10, lists[1:])), context
    # through Python: a strided list, fewer candidates than k, no list at all, a workspace of the caller's
    strided = torch.from_numpy(np.ascontiguousarray(lists)).cuda()
    got = reader.cosmul_topk_device(terms, offsets, negatives_from, on_device[:7], 10, exclude=strided[:, :4])
    assert reader.last_cosmul_kernel == FUSED, context
    assert same_topk([part.cpu().numpy() for part in got], topk_excluding_by_the_contract(scores[:, :7], 10, lists[:, :4])), context
    own = torch.empty((cosmul().query_cosmul_workspace_bytes(reader._impl.context_handle(), n_terms, len(QUESTIONS), n, 10, True) + 4096,), dtype=torch.uint8, device='cuda')
    got = reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 10, workspace=own)
    assert same_topk([part.cpu().numpy() for part in got], topk_excluding_by_the_contract(scores, 10, None)), context
    # no candidate and no question
    none = nearest_with_workspace(reader, terms, questions, on_device[:0], 4, lists, minimal=False)
    assert (none[1] == -1).all() and np.isneginf(none[0]).all()
    nothing = reader.cosmul_topk_device(terms, [0], [], on_device, 4)
    assert tuple(nothing[0].shape) == tuple(nothing[1].shape) == (0, 4) and reader.last_cosmul_kernel == ''


FORMS_REACHED = set()


@pytest.mark.parametrize('bits,distribution', KEY_FORM_MODELS)
def test_every_key_form(native, make_model, monkeypatch, bits, distribution):
    seen = []

    def check(reader, context):
        assert cosmul().query_cosmul_kernel_name(reader._impl.context_handle()) == FUSED, context
        FORMS_REACHED.add(kernel_form(reader))
        check_fused(reader, KEY_FORM_ROWS, context, ranks=(10,) if seen else (1, 10, 64))
        seen.append(context)

    for_every_key_form(native, make_model, monkeypatch, KEY_FORM_ROWS, check, models=[(bits, distribution)], all_forms=False)


def test_the_three_key_forms_ran():
    assert FORMS_REACHED == ALL_KEY_FORMS, FORMS_REACHED


def test_seven_words_per_wavefront(native, make_model, monkeypatch):
    path, _ = make_model(N_ROWS, 340, 'trained', 4)
    set_environment(monkeypatch, MEMB_HIP_LANES=9)
    reader = native.Reader(path)
    assert words_per_wave(reader) == 7
    check_fused(reader, N_ROWS, 'seven words per wavefront', ranks=(1, 64))


def test_candidate_ids_with_misses(native, make_model):
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = ids_with_misses(333, N_ROWS, 63)
    assert (rows >= N_ROWS).any()
    offsets, negatives_from, n_terms = questions_of(((2, 1), (1, 1)))
    on_device = to_device(rows)
    terms = reader.unit_rows_embedding_device(to_device(ids_with_misses(n_terms, N_ROWS, 64)))
    matrix = reader.similarity_matrix_device(terms, on_device).cpu().numpy()
    assert (matrix[:, rows >= N_ROWS] == 0).all()
    scores = cosmul_scores_by_the_contract(matrix, offsets, negatives_from)
    for k in (1, 10, 64):
        got = reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, k)
        assert same_topk([part.cpu().numpy() for part in got], topk_excluding_by_the_contract(scores, k, None)), k
    host = reader.cosmul_topk(terms.cpu().numpy(), offsets, negatives_from, rows, 10)
    assert same_topk(host, topk_excluding_by_the_contract(scores, 10, None))


# ---- 3. without a fused kernel ----

def test_a_uniform_model_through_the_fallback(native, make_model, monkeypatch):
    import memb_amd.reader
    import torch
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 128)   # 200 candidates: two slices
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    reader = native.Reader(path)
    assert cosmul().query_cosmul_kernel_name(reader._impl.context_handle()) == ''
    rows = tied_candidates(200, N_ROWS, 9)
    offsets, negatives_from, n_terms = questions_of(QUESTIONS)
    on_device = to_device(rows)
    terms = queries_to_device(reader.unit_rows_embedding_device(to_device(ids_with_misses(n_terms, N_ROWS, 65))).cpu().numpy(), ld=303, shift=1)
    matrix = reader.similarity_matrix_device(terms, on_device).cpu().numpy()
    scores = cosmul_scores_by_the_contract(matrix, offsets, negatives_from)
    best = topk_by_the_contract(scores, 64)[1]
    lists = np.ascontiguousarray(np.concatenate([best[:, [0, 1, 3]], np.broadcast_to(np.array([127, 128, 199, -1]), (len(QUESTIONS), 4))], axis=1), dtype=np.int64)
    lists[1] = -1
    for k in (1, 10, 64):
        for given in (None, lists):
            got = reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, k, exclude=None if given is None else torch.from_numpy(given).cuda())
            assert reader.last_cosmul_kernel == DENSE
            assert same_topk([part.cpu().numpy() for part in got], topk_excluding_by_the_contract(scores, k, given)), (k, given is None)
    none = reader.cosmul_topk_device(terms, offsets, negatives_from, on_device[:0], 4)
    assert (none[1].cpu().numpy() == -1).all() and np.isneginf(none[0].cpu().numpy()).all()
    assert reader.last_cosmul_kernel == 'topk_merge'
    # questions without any term at all: no matrix is asked for
    bare = reader.cosmul_topk_device(terms[:0], [0, 0, 0], [0, 0], on_device, 3)
    assert (bare[1].cpu().numpy() == [0, 1, 2]).all() and (bare[0].cpu().numpy() == EMPTY_SCORE).all()
    assert reader.last_cosmul_kernel == 'cosmul_scores+topk_select_excluding+topk_merge'
    host = reader.cosmul_topk(terms.cpu().numpy(), offsets, negatives_from, rows, 10, exclude=lists)
    assert same_topk(host, topk_excluding_by_the_contract(scores, 10, lists))


# ---- 4. words ----

def test_cosmul_analogies(native, make_model):
    import torch
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader, host = native.Reader(path), native.Reader(path, device='cpu')
    a, b, c, d = words[5], words[17], words[40], words[99]
    positive = [[b, c], [b, c, d], [a], [b, 'no such word é'], [], [c, c], []]
    negative = [[a], [a, d], [], [a], [], [], [a]]
    flat = [([b, c], [a]), ([b, c, d], [a, d]), ([a], []), None, None, ([c, c], []), ([], [a])]
    everything = reader._all_rows_device(torch, 0)
    for k in (7, 64):
        values, rows = reader.analogies_cosmul_device(positive, negative, k)
        assert reader.last_cosmul_kernel == FUSED
        assert values.dtype == torch.float32 and rows.dtype == torch.int64 and tuple(values.shape) == tuple(rows.shape) == (7, k)
        values, rows = values.cpu().numpy(), rows.cpu().numpy()
        for q, entries in enumerate(flat):
            if entries is None:   # an unknown word, no word: empty slots
                assert (rows[q] == -1).all() and np.isneginf(values[q]).all(), q
                continue
            own = reader.resolve_rows_device(entries[0] + entries[1])
            matrix = reader.similarity_matrix_device(reader.unit_rows_embedding_device(own), everything).cpu().numpy()
            scores = cosmul_scores_by_the_contract(matrix, [0, len(entries[0]) + len(entries[1])], [len(entries[0])])
            want = topk_excluding_by_the_contract(scores, k, own.cpu().numpy().astype(np.int64)[None, :])
            assert same_topk((values[q:q + 1], rows[q:q + 1]), want), (k, q)
            assert (rows[q] >= 0).all() and not set(rows[q].tolist()) & set(own.cpu().numpy().tolist()), (k, q)
    pairs = reader.analogies_cosmul(positive, negative, 7)
    assert pairs == host.analogies_cosmul(positive, negative, 7)
    assert pairs[3] == pairs[4] == [] and [len(answer) for answer in pairs] == [7, 7, 7, 0, 0, 7, 7]
    assert not {word for word, _ in pairs[0]} & {a, b, c}
    assert reader.analogy_cosmul(a, b, c, k=7) == pairs[0] and reader.analogy_cosmul(a, b, c) == pairs[0][:1] == host.analogy_cosmul(a, b, c)
    assert tuple(reader.analogies_cosmul_device([], None, 3)[0].shape) == (0, 3) and reader.analogies_cosmul([], None, 3) == []
    # one positive word and nothing else: the score rises with the cosine, so the positions are analogies_device's, down to
    # the first neighbours whose cosines tie -- or whose rounded scores do, which can happen where the cosines differ
    # (1 + c is rounded), never the reverse
    for word in (a, d):
        cosines, by_cosine = (part.cpu().numpy()[0] for part in reader.analogies_device([[word]], None, 64))
        scores, by_score = (part.cpu().numpy()[0] for part in reader.analogies_cosmul_device([[word]], None, 64))
        ties = np.nonzero((cosines[1:] == cosines[:-1]) | (scores[1:] == scores[:-1]))[0]
        until = int(ties[0]) if ties.size else 64
        assert until >= 10 and by_score[:until].tolist() == by_cosine[:until].tolist(), word
    with pytest.raises(TypeError, match='no weights'):
        reader.analogies_cosmul_device([[(b, 0.5), c]], [[a]])
    with pytest.raises(ValueError, match='64'):
        reader.analogies_cosmul_device([[a] * 65])
    assert tuple(reader.analogies_cosmul_device([[a] * 40], [[b] * 24], 3)[1].shape) == (1, 3)


# ---- 5. refusals ----

def test_refusals(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    on_device = to_device(ids_with_misses(40, N_ROWS, 3))
    terms = queries_to_device(np.ones((3, 300), dtype=np.float32))
    offsets, negatives_from = [0, 3], [2]
    with pytest.raises(TypeError, match='float32'):
        reader.cosmul_topk_device(terms.to(torch.float64), offsets, negatives_from, on_device, 5)
    with pytest.raises(TypeError, match='on the GPU'):
        reader.cosmul_topk_device(terms.cpu(), offsets, negatives_from, on_device, 5)
    with pytest.raises(ValueError, match='shape'):
        reader.cosmul_topk_device(terms[0], offsets, negatives_from, on_device, 5)
    with pytest.raises(ValueError, match='ascend'):
        reader.cosmul_topk_device(terms, [0, 4], [2], on_device, 5)
    with pytest.raises(ValueError, match='ascend'):
        reader.cosmul_topk_device(terms, [2, 1], [2], on_device, 5)
    with pytest.raises(ValueError, match='negatives_from'):
        reader.cosmul_topk_device(terms, [0, 2], [3], on_device, 5)
    with pytest.raises(ValueError, match='Q \\+ 1'):
        reader.cosmul_topk_device(terms, [0, 2], [1, 2], on_device, 5)
    with pytest.raises(ValueError, match='64'):
        reader.cosmul_topk_device(queries_to_device(np.ones((65, 300), dtype=np.float32)), [0, 65], [65], on_device, 5)
    with pytest.raises(ValueError, match='k must'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 65)
    with pytest.raises(TypeError, match='int64'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 5, exclude=torch.zeros((1, 2), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='shape'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 5, exclude=torch.zeros((2, 2), dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError, match='workspace'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 5, workspace=torch.zeros(64, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='workspace too small'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, 5, workspace=torch.zeros(64, dtype=torch.uint8, device='cuda'))
    # the C entry points: every refusal, the sentinels left in place -- nothing was launched
    values = torch.full((1, 5), SENTINEL, dtype=torch.float32, device='cuda')
    positions = torch.full((1, 5), SENTINEL_POSITION, dtype=torch.int64, device='cuda')
    cosines = torch.zeros((3, 40), dtype=torch.float32, device='cuda')
    scores = torch.full((1, 40), SENTINEL, dtype=torch.float32, device='cuda')
    lists = torch.zeros((1, 70), dtype=torch.int64, device='cuda')
    device_offsets, device_negatives = questions_to_device(offsets, negatives_from)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(device=0, cosines_ptr=cosines.data_ptr(), ld=40, offsets_ptr=device_offsets.data_ptr(),
                negatives_from_ptr=device_negatives.data_ptr(), n_questions=1, n=40, scores_ptr=scores.data_ptr(), ld_scores=40, stream=stream)
    for word, change in (('device', dict(device=-1)), ('null', dict(offsets_ptr=0)), ('null', dict(negatives_from_ptr=0)),
                         ('null', dict(scores_ptr=0)), ('cosines', dict(cosines_ptr=0)), ('at least n', dict(ld=39)),
                         ('at least n', dict(ld_scores=39)), ('aligned', dict(cosines_ptr=cosines.data_ptr() + 2)),
                         ('aligned', dict(scores_ptr=scores.data_ptr() + 1)), ('aligned', dict(offsets_ptr=device_offsets.data_ptr() + 2)),
                         ('too large', dict(n_questions=2 ** 16 + 1)), ('too large', dict(n=2 ** 31 + 1, ld=2 ** 32, ld_scores=2 ** 32))):
        with pytest.raises(RuntimeError, match=word):
            cosmul().cosmul_scores_to_device(**dict(good, **change))
    needed = cosmul().query_cosmul_workspace_bytes(reader._impl.context_handle(), 3, 1, 40, 5)
    workspace = torch.full((needed // 4,), 0x7FC00001, dtype=torch.int32, device='cuda')
    fine = dict(terms_ptr=terms.data_ptr(), n_terms=3, ld_terms=300, offsets_ptr=device_offsets.data_ptr(),
                negatives_from_ptr=device_negatives.data_ptr(), n_questions=1, rows_ptr=on_device.data_ptr(), n=40, k=5,
                excluded_ptr=lists.data_ptr(), width=4, ld_excluded=70, values_ptr=values.data_ptr(), positions_ptr=positions.data_ptr(),
                ld_out=5, workspace_ptr=workspace.data_ptr(), workspace_bytes=needed, stream=stream)
    for word, change in (('k must', dict(k=0)), ('k must', dict(k=65)), ('null', dict(values_ptr=0)), ('null', dict(positions_ptr=0)),
                         ('ld_out', dict(ld_out=4)), ('2\\^16 terms', dict(n_terms=2 ** 16 + 1)), ('2\\^16 questions', dict(n_questions=2 ** 16 + 1)),
                         ('offsets', dict(offsets_ptr=0)), ('negatives_from', dict(negatives_from_ptr=0)),
                         ('aligned', dict(offsets_ptr=device_offsets.data_ptr() + 1)), ('queries', dict(terms_ptr=0)), ('rows', dict(rows_ptr=0)),
                         ('ld_queries', dict(ld_terms=299)), ('too large', dict(n=2 ** 36 + 1)), ('at most 64', dict(width=65)),
                         ('ld_excluded', dict(ld_excluded=3)), ('null', dict(excluded_ptr=0)), ('aligned', dict(excluded_ptr=lists.data_ptr() + 4)),
                         ('aligned', dict(workspace_ptr=workspace.data_ptr() + 4)), ('aligned', dict(positions_ptr=positions.data_ptr() + 4)),
                         ('workspace too small', dict(workspace_bytes=cosmul().query_cosmul_workspace_bytes(reader._impl.context_handle(), 3, 1, 40, 5, True) - 1)),
                         ('workspace too small', dict(workspace_ptr=0))):
        with pytest.raises(RuntimeError, match=word):
            cosmul().query_cosmul_nearest_to_device(reader._impl.context_handle(), **dict(fine, **change))
    torch.cuda.synchronize()
    assert (values.cpu().numpy() == np.float32(SENTINEL)).all() and (positions.cpu().numpy() == SENTINEL_POSITION).all()
    assert (scores.cpu().numpy() == np.float32(SENTINEL)).all() and (workspace.cpu().numpy() == 0x7FC00001).all()
    # a model without the fused matrix kernel: refused as unsupported (False), nothing launched
    path, _ = make_model(N_ROWS, 300, 'uniform', 8)
    uniform = native.Reader(path)
    assert cosmul().query_cosmul_nearest_to_device(uniform._impl.context_handle(), **fine) is False
    torch.cuda.synchronize()
    assert (values.cpu().numpy() == np.float32(SENTINEL)).all() and (workspace.cpu().numpy() == 0x7FC00001).all()


# ---- 6. a captured graph ----

def test_captured_into_a_graph(native, make_model):
    """cosmul_topk_device with a caller's workspace and its questions uploaded beforehand (questions=: the upload is the one
    step of the call no capture admits), captured, then replayed once over other terms and other lists, both written in
    place; the answer is the host reader's for those"""
    import torch
    from test_gpu_query_topk import capture, graph_case, slices_of_256
    reader, host, rows, on_device, _ = graph_case(native, make_model, 76)
    offsets, negatives_from, n_terms = questions_of(QUESTIONS)
    count, k = len(QUESTIONS), 10
    rng = np.random.default_rng(77)
    terms = torch.from_numpy(rng.standard_normal((n_terms, 300)).astype(np.float32)).cuda()
    lists = torch.from_numpy(rng.integers(0, rows.size, size=(count, 6)).astype(np.int64)).cuda()
    questions = torch.from_numpy(np.concatenate([offsets, negatives_from]).astype(np.int32)).cuda()
    context = reader._impl.context_handle()
    workspace = slices_of_256(cosmul().query_cosmul_workspace_bytes(context, n_terms, count, rows.size, k, True), n_terms + count)
    graph, (values, positions) = capture(lambda: reader.cosmul_topk_device(
        terms, offsets, negatives_from, on_device, k, exclude=lists, workspace=workspace, questions=questions))
    assert reader.last_cosmul_kernel == FUSED
    # the other terms: unit rows of the model that are candidates themselves, so scores repeat bit for bit
    valid = np.unique(rows[rows < N_ROWS])
    other_terms = host.unit_rows_embedding(valid[np.arange(n_terms) % 5])
    best = host.cosmul_topk(other_terms, offsets, negatives_from, rows, 64)[1]
    other_lists = np.concatenate([best[:, [0, 2, 5]], np.broadcast_to(np.array([3, rows.size - 1, -1]), (count, 3))], axis=1).astype(np.int64)
    terms.copy_(torch.from_numpy(other_terms))
    lists.copy_(torch.from_numpy(other_lists))
    values.fill_(SENTINEL)
    positions.fill_(SENTINEL_POSITION)
    graph.replay()
    torch.cuda.synchronize()
    want = host.cosmul_topk(other_terms, offsets, negatives_from, rows, k, exclude=other_lists)
    assert not same_topk(want, host.cosmul_topk(other_terms, offsets, negatives_from, rows, k))
    assert same_topk((values.cpu().numpy(), positions.cpu().numpy()), want)
    with pytest.raises(TypeError, match='questions'):
        reader.cosmul_topk_device(terms, offsets, negatives_from, on_device, k, questions=questions[:-1])
