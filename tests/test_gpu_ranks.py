"""The rank counts on the GPU: the dense call over hostile matrices at every column count at which rank_count takes
another path (between sentinels, dirty workspaces, slices accumulated in shuffled order), the fused call on trained models
against the brute-force restatement of tests/ranks_reference.py over similarity_matrix_device's matrix under the
recommended and the minimal workspace, the slot similarity_topk_device gives the same candidate, a uniform model through
the fallback, the word-level calls against a device='cpu' reader, and a captured graph. Every comparison is exact."""
import numpy as np
import pytest

from ranks_reference import INT64_MAX, hostile_matrix, marks_over, ranks_by_the_contract

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained+rank_count+rank_fold'
DENSE = 'pairs_dense+rank_count+rank_fold'
BLOCK_RUN = 2048                                     # memb_ranks::BLOCK_RUN: the columns of one block of rank_count
COLUMNS = (1, 63, 255, 257, BLOCK_RUN - 1, BLOCK_RUN + 1, 5003)
ROWS = (1, 3, 17)
SENTINEL = -777
DIRTY = 0x7FC00001


def ranks():
    from memb_amd import _memb_ranks
    return _memb_ranks


def lists_over(count, n, seed, base=0):
    """int64 (count, 9): positions all over the columns (so that they fall into different slices and blocks), a repeat,
    -1 padding, one entry beyond each end"""
    rng = np.random.default_rng(seed)
    lists = base + rng.integers(0, n, size=(count, 9)).astype(np.int64)
    lists[:, 3] = lists[:, 0]
    lists[:, 4] = -1
    lists[:, 5] = base + n + rng.integers(0, 5, size=count)
    lists[:, 6] = base - 1 - rng.integers(0, 5, size=count)
    return lists


@pytest.fixture(scope='module')
def dense_cases():
    """{n: (matrix (17, n), thresholds, marks, lists, counts without the lists, counts with them)}, worked out once"""
    whole = hostile_matrix(max(ROWS), max(COLUMNS), seed=61)
    cases = {}
    for n in COLUMNS:
        matrix = np.ascontiguousarray(whole[:, :n])
        thresholds, marks = marks_over(matrix, seed=n)
        lists = lists_over(max(ROWS), n, seed=n + 1)
        lists[:, 7] = np.clip(marks, -1, n)           # the mark itself among the non-candidates
        cases[n] = (matrix, thresholds, marks, lists, ranks_by_the_contract(matrix, thresholds, marks),
                    ranks_by_the_contract(matrix, thresholds, marks, 0, lists))
    return cases


def dense_ranks(matrix, thresholds, marks, base=0, lists=None, accumulate=False, held=None, spare=3):
    """_memb_ranks.dense_ranks_to_device on a host matrix: rows n + spare floats apart with NaN behind them (NaN precedes
    every mark but a NaN one: a read beyond a row shows), a dirty workspace of exactly the size asked for, the counts above
    a sentinel, which must survive. held: the counts to add to under accumulate."""
    import torch
    count, n = matrix.shape
    on_device = torch.full((count + 1, n + spare), float('nan'), dtype=torch.float32, device='cuda')
    if n:
        on_device[:count, :n] = torch.from_numpy(np.ascontiguousarray(matrix)).cuda()
    device_thresholds = torch.from_numpy(np.ascontiguousarray(thresholds)).cuda()
    device_marks = torch.from_numpy(np.ascontiguousarray(marks, dtype=np.int64)).cuda()
    device_lists = None if lists is None else torch.from_numpy(np.ascontiguousarray(lists)).cuda()
    counts = torch.full((count + 1,), SENTINEL, dtype=torch.int64, device='cuda')
    if held is not None:
        counts[:count] = torch.from_numpy(held).cuda()
    needed = ranks().dense_ranks_workspace_bytes(count, n)
    assert needed == (count * -(-n // BLOCK_RUN) * 4 + 7) // 8 * 8
    workspace = torch.full((needed // 4 + 2,), DIRTY, dtype=torch.int32, device='cuda')
    ranks().dense_ranks_to_device(
        0, on_device.data_ptr() if n else 0, count, n, n + spare, base, device_thresholds.data_ptr(), device_marks.data_ptr(),
        0 if lists is None else device_lists.data_ptr(), 0 if lists is None else lists.shape[1], 0 if lists is None else lists.shape[1],
        accumulate, counts.data_ptr(), workspace.data_ptr() if needed else 0, needed, torch.cuda.current_stream().cuda_stream)
    got = counts.cpu().numpy()
    assert got[count] == SENTINEL and (workspace[needed // 4:].cpu().numpy() == DIRTY).all()
    return got[:count]


# ---- 1. the dense call ----

@pytest.mark.parametrize('n', COLUMNS)
def test_the_dense_call(native, dense_cases, n):
    matrix, thresholds, marks, lists, plain, without = dense_cases[n]
    for count in ROWS:
        assert dense_ranks(matrix[:count], thresholds[:count], marks[:count]).tolist() == plain[:count].tolist(), (n, count)
        assert dense_ranks(matrix[:count], thresholds[:count], marks[:count], lists=lists[:count]).tolist() == without[:count].tolist(), (n, count)
    # tight rows (ld == n), and a base: the positions of the marks and of the lists move with it
    moved = np.where((marks >= 0) & (marks < INT64_MAX), marks + 1000, marks)
    assert dense_ranks(matrix, thresholds, moved, base=1000, spare=0).tolist() == ranks_by_the_contract(matrix, thresholds, moved, 1000).tolist()
    shifted = np.where(lists >= 0, lists + 1000, lists)
    assert dense_ranks(matrix, thresholds, moved, base=1000, lists=shifted, spare=0).tolist() == \
        ranks_by_the_contract(matrix, thresholds, moved, 1000, shifted).tolist()


def test_slices_in_any_order_accumulate(native, dense_cases):
    matrix, thresholds, marks, lists, _, without = dense_cases[5003]
    cuts = [0, 1, 64, 2048, 2049, 4097, 5003]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    np.random.default_rng(62).shuffle(pieces)
    held = None
    for start, stop in pieces:
        held = dense_ranks(matrix[:, start:stop], thresholds, marks, base=start, lists=lists, accumulate=held is not None, held=held)
    assert held.tolist() == without.tolist()
    # no column: zeros, or what was there under accumulate
    assert dense_ranks(matrix[:3, :0], thresholds[:3], marks[:3], lists=lists[:3]).tolist() == [0, 0, 0]
    kept = np.array([5, 6, 7], dtype=np.int64)
    assert dense_ranks(matrix[:3, :0], thresholds[:3], marks[:3], accumulate=True, held=kept).tolist() == [5, 6, 7]


# ---- 2. the fused call ----

MODELS = ((3000, 300, 4), (3000, 300, 6), (2000, 12, 4))
N_CANDIDATES = 1100


@pytest.fixture(scope='module', params=MODELS, ids=lambda model: '{}x{}-{}bit'.format(*model))
def fused_case(request, native, make_model):
    """(reader, queries, rows, matrix, thresholds, marks, lists, counts without the lists, counts with them): 1100
    candidates with repeated rows -- bit-equal cosines at different positions --, five queries, two of them the unit rows
    of repeated candidates; the reference over similarity_matrix_device's matrix, worked out once"""
    import torch
    count, dim, bits = request.param
    path, _ = make_model(count, dim, 'trained', bits)
    reader = native.Reader(path)
    rng = np.random.default_rng(63 + bits + dim)
    host_rows = rng.integers(0, count, size=N_CANDIDATES).astype(np.uint32)
    host_rows[::7] = host_rows[3]                       # one row 158 times, in every slice of 64
    host_rows[5::50] = host_rows[9]
    host_rows[20] = 0xFFFFFFFF                          # not in the model: cosine 0
    rows = torch.from_numpy(host_rows.view(np.int32)).cuda()
    queries = torch.from_numpy(rng.normal(size=(5, dim)).astype(np.float32)).cuda()
    queries[0] = reader.unit_rows_embedding_device(rows[3:4])[0]
    queries[1] = reader.unit_rows_embedding_device(rows[9:10])[0]
    matrix = reader.similarity_matrix_device(queries, rows).cpu().numpy()
    assert reader.last_query_matrix_kernel == 'query_matrix_trained'
    # ranks of the repeated candidates (ties decided by the position), then the other kinds of mark
    columns = np.array([7 * 64, 5 + 50 * 11, 14, 700, 21])
    thresholds = matrix[np.arange(5), columns].copy()
    marks = np.array([columns[0], columns[1], columns[2], -1, INT64_MAX], dtype=np.int64)
    lists = lists_over(5, N_CANDIDATES, seed=64)
    lists[0, :3] = (0, 7, 7 * 100)                      # among the tied best of query 0, in different slices
    # query 0 is the unit row of a candidate that stands at many positions: the ones before the mark are all that precede it
    tied = np.nonzero(host_rows[:columns[0]] == host_rows[3])[0]
    assert tied.size >= 60 and {0, 7} <= set(tied.tolist())
    plain = ranks_by_the_contract(matrix, thresholds, marks)
    assert plain[0] == tied.size and ranks_by_the_contract(matrix, thresholds, marks, 0, lists)[0] == tied.size - len(set(tied.tolist()) & set(lists[0].tolist()))
    return (reader, queries, rows, matrix, thresholds, marks, lists, ranks_by_the_contract(matrix, thresholds, marks),
            ranks_by_the_contract(matrix, thresholds, marks, 0, lists))


def to_device(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def test_the_fused_call(fused_case):
    import torch
    reader, queries, rows, matrix, thresholds, marks, lists, plain, without = fused_case
    context = reader._impl.context_handle()
    assert plain[0] >= 60 and without[0] <= plain[0] - 2              # some sixty bit-equal cosines come first, two of them named
    for exclude, want in ((None, plain), (lists, without)):
        got = reader.similarity_ranks_device(queries, rows, to_device(thresholds), to_device(marks),
                                             exclude=None if exclude is None else to_device(exclude))
        assert reader.last_ranks_kernel == FUSED
        assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == want.tolist()
        # the minimal workspace: slices of 64 candidates, eighteen of them; a dirty one of exactly that size
        least = ranks().query_ranks_workspace_bytes(context, 5, N_CANDIDATES, minimal=True)
        assert least == 24 + 4 * 5 * 64 < ranks().query_ranks_workspace_bytes(context, 5, N_CANDIDATES) == 24 + 4 * 5 * N_CANDIDATES
        workspace = torch.full((least // 4 + 2,), DIRTY, dtype=torch.int32, device='cuda').view(torch.uint8)[:least]
        sliced = reader.similarity_ranks_device(queries, rows, to_device(thresholds), to_device(marks),
                                                exclude=None if exclude is None else to_device(exclude), workspace=workspace)
        assert sliced.cpu().numpy().tolist() == want.tolist()
        with pytest.raises(RuntimeError, match='workspace too small'):
            reader.similarity_ranks_device(queries, rows, to_device(thresholds), to_device(marks), workspace=workspace[:least - 8])
    # marks=None counts the strictly greater cosines
    got = reader.similarity_ranks_device(queries, rows, to_device(thresholds))
    assert got.cpu().numpy().tolist() == ranks_by_the_contract(matrix, thresholds, [-1] * 5).tolist()
    # the numpy form, and nothing to count
    assert reader.similarity_ranks(queries.cpu().numpy(), rows.cpu().numpy().view(np.uint32), thresholds, marks, exclude=lists).tolist() == without.tolist()
    assert reader.similarity_ranks_device(queries, rows[:0], to_device(thresholds), to_device(marks)).cpu().numpy().tolist() == [0] * 5
    assert reader.last_ranks_kernel == FUSED
    assert reader.similarity_ranks_device(queries[:0], rows, to_device(thresholds[:0])).shape == (0,) and reader.last_ranks_kernel == ''


def test_a_rank_is_the_slot_of_the_selection(fused_case):
    reader, queries, rows, matrix, thresholds, marks, lists, plain, without = fused_case
    # the first three marks are candidates with their own cosines: where the rank is below 64 the selection holds them there
    for exclude, counts in ((None, plain), (lists, without)):
        positions = reader.similarity_topk_device(queries, rows, 64, exclude=None if exclude is None else to_device(exclude))[1].cpu().numpy()
        checked = 0
        for q in range(3):
            named = exclude is not None and marks[q] in exclude[q]
            if counts[q] < 64 and not named:
                assert positions[q, counts[q]] == marks[q], (q, counts[q])
                checked += 1
        assert checked >= 1
    # and every slot of the selection is the rank of its candidate
    values, positions = (part.cpu().numpy() for part in reader.similarity_topk_device(queries[:2], rows, 64))
    for slot in (0, 1, 31, 63):
        got = reader.similarity_ranks_device(queries[:2], rows, to_device(values[:, slot]), to_device(positions[:, slot]))
        assert got.cpu().numpy().tolist() == [slot, slot]


def test_the_whole_model_and_the_threshold_of_a_word(fused_case):
    import torch
    reader, queries, rows, *_ = fused_case
    everything = torch.arange(len(reader), dtype=torch.int32, device='cuda')
    matrix = reader.similarity_matrix_device(queries, everything).cpu().numpy()
    expected = rows[[3, 9, 14, 700, 21]].contiguous()
    # one candidate per group: bit for bit the matrix's entry at the mark
    thresholds = reader.query_similarity_device(queries, expected, torch.arange(6, dtype=torch.int32, device='cuda'))
    host_expected = expected.cpu().numpy().astype(np.int64)
    assert np.array_equal(thresholds.cpu().numpy().view(np.uint32), matrix[np.arange(5), host_expected].view(np.uint32))
    got = reader.similarity_ranks_device(queries, None, thresholds, expected.to(torch.int64))
    assert got.cpu().numpy().tolist() == ranks_by_the_contract(matrix, thresholds.cpu().numpy(), host_expected).tolist()


def test_a_uniform_model_takes_the_fallback(native, make_model, monkeypatch):
    import memb_amd.reader
    import torch
    path, _ = make_model(1500, 300, 'uniform', 8)
    reader = native.Reader(path)
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 500)   # three slices, the last shorter: accumulate
    rng = np.random.default_rng(65)
    host_rows = rng.integers(0, 1500, size=1234).astype(np.uint32)
    host_rows[::9] = host_rows[4]
    rows = torch.from_numpy(host_rows.view(np.int32)).cuda()
    queries = torch.from_numpy(rng.normal(size=(3, 300)).astype(np.float32)).cuda()
    queries[0] = reader.unit_rows_embedding_device(rows[4:5])[0]
    matrix = reader.similarity_matrix_device(queries, rows).cpu().numpy()
    thresholds = matrix[np.arange(3), [9 * 100, 600, 50]].copy()
    marks = np.array([9 * 100, -1, INT64_MAX], dtype=np.int64)
    lists = lists_over(3, 1234, seed=66)
    got = reader.similarity_ranks_device(queries, rows, to_device(thresholds), to_device(marks), exclude=to_device(lists))
    assert reader.last_ranks_kernel == DENSE
    assert got.cpu().numpy().tolist() == ranks_by_the_contract(matrix, thresholds, marks, 0, lists).tolist()
    assert reader.similarity_ranks_device(queries, rows[:0], to_device(thresholds)).cpu().numpy().tolist() == [0, 0, 0]
    assert reader.last_ranks_kernel == 'rank_fold'


# ---- 3. words ----

def test_words_equal_a_host_reader(native, make_model):
    path, words = make_model(3000, 300, 'trained', 4)
    reader, host = native.Reader(path), native.Reader(path, device='cpu')
    rng = np.random.default_rng(67)
    first = [words[i] for i in rng.integers(0, 3000, size=12)] + ['no such word é', words[5]]
    second = [words[i] for i in rng.integers(0, 3000, size=12)] + [words[7], 'no such word é']
    ranks_of_pairs = reader.rank(first, second)
    assert ranks_of_pairs.tolist() == host.rank(first, second).tolist()
    assert ranks_of_pairs.tolist() == reader.rank_device(first, second).cpu().numpy().tolist()
    assert ranks_of_pairs[-2:].tolist() == [0, 0] and (ranks_of_pairs[:12] >= 1).all()
    assert reader.count_closer_than(first, second).tolist() == (ranks_of_pairs - 1).tolist()
    # the nearest words of a word have the ranks 1, 2, 3, ...
    nearest = [word for word, _ in reader.most_similar([words[40]], k=5)[0]]
    assert reader.rank([words[40]] * 5, nearest).tolist() == [1, 2, 3, 4, 5]
    positive = [[words[17], words[40]], [words[99], words[3], words[8]], [words[17], 'no such word é'], [words[1]], []]
    negative = [[words[5]], [words[17], words[99]], [words[5]], [], []]
    expected = [words[2000], words[41], words[41], 'no such word é', words[1]]
    got = reader.analogy_ranks(positive, negative, expected)
    assert got.tolist() == host.analogy_ranks(positive, negative, expected).tolist() and got[2:].tolist() == [0, 0, 0]
    assert got.tolist() == reader.analogy_ranks_device(positive, negative, expected).cpu().numpy().tolist()
    # the answers of analogies have the ranks 1, 2, 3
    answers = [word for word, _ in reader.analogies(positive[:1], negative[:1], k=3)[0]]
    assert reader.analogy_ranks(positive[:1] * 3, negative[:1] * 3, answers).tolist() == [1, 2, 3]
    questions = [(words[5], words[17], words[40], answers[0]), (words[5], words[17], words[40], answers[2]),
                 (words[5], words[17], 'no such word é', answers[0]), (words[9], words[10], words[11], words[12])]
    result = reader.evaluate_analogies(questions)
    assert result == host.evaluate_analogies(questions)
    assert result['questions'] == 4 and result['answered'] == 3 and 1 / 3 <= result['accuracy'] <= 2 / 3
    assert result['mean_reciprocal_rank'] >= (1 + 1 / 3) / 3


def test_argument_errors(fused_case):
    import torch
    reader, queries, rows, matrix, thresholds, marks, lists, *_ = fused_case
    good_thresholds, good_marks = to_device(thresholds), to_device(marks)
    with pytest.raises(TypeError, match='thresholds'):
        reader.similarity_ranks_device(queries, rows, good_thresholds.double())
    with pytest.raises(TypeError, match='thresholds'):
        reader.similarity_ranks_device(queries, rows, thresholds)
    with pytest.raises(TypeError, match='on the GPU'):
        reader.similarity_ranks_device(queries, rows, good_thresholds.cpu())
    with pytest.raises(ValueError, match='thresholds'):
        reader.similarity_ranks_device(queries, rows, good_thresholds[:4])
    with pytest.raises(TypeError, match='marks'):
        reader.similarity_ranks_device(queries, rows, good_thresholds, good_marks.int())
    with pytest.raises(ValueError, match='marks'):
        reader.similarity_ranks_device(queries, rows, good_thresholds, torch.zeros(10, dtype=torch.int64, device='cuda')[::2])
    with pytest.raises(ValueError, match='64'):
        reader.similarity_ranks_device(queries, rows, good_thresholds, good_marks, exclude=torch.zeros((5, 65), dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError, match='workspace'):
        reader.similarity_ranks_device(queries, rows, good_thresholds, good_marks, workspace=torch.zeros(4096, dtype=torch.float32, device='cuda'))
    with pytest.raises(TypeError, match='float32'):
        reader.similarity_ranks_device(queries.double(), rows, good_thresholds)


# ---- 4. a captured graph ----

def test_captured_into_a_graph(fused_case):
    import torch
    reader, queries, rows, matrix, thresholds, marks, lists, plain, without = fused_case
    context = reader._impl.context_handle()
    workspace = torch.empty((ranks().query_ranks_workspace_bytes(context, 5, N_CANDIDATES, minimal=True) + 4 * 5 * 192,), dtype=torch.uint8,
                            device='cuda')          # slices of 256 candidates: five of them
    device_thresholds, device_marks, device_lists = to_device(thresholds), to_device(marks), to_device(lists)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        reader.similarity_ranks_device(queries, rows, device_thresholds, device_marks, exclude=device_lists, workspace=workspace)   # (warm-up)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        counts = reader.similarity_ranks_device(queries, rows, device_thresholds, device_marks, exclude=device_lists, workspace=workspace)
    # replayed over other marks: the strictly greater cosines, without the lists' columns
    device_marks.fill_(-1)
    counts.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == ranks_by_the_contract(matrix, thresholds, [-1] * 5, 0, lists).tolist()
