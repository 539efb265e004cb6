"""The lists of the candidates before a mark on the GPU: the dense call at every column count at which a wavefront, a
block or a run ends (and at 65 blocks per row, where within_starts carries), between guard entries, with a dirty workspace
of exactly the size asked for; lists of non-candidates inside one run and across runs; slices accumulated in ascending and
in reverse order; offsets and a capacity that are too small; the fused call on a trained model and the fallback on a
uniform one against the dense call over similarity_matrix_device's matrix under three workspaces; the word-level calls
against a device='cpu' reader; and a captured graph. Every comparison is exact: integers and copied bits."""
import numpy as np
import pytest

from ranks_reference import INT64_MAX, hostile_matrix, marks_over
from within_reference import same_lists, within_by_the_contract

pytestmark = pytest.mark.gpu

FUSED = 'query_matrix_trained+within_count+within_starts+within_write'
DENSE = 'pairs_dense+within_count+within_starts+within_write'
BLOCK_RUN = 2048                                     # memb_ranks::BLOCK_RUN: the columns of one block
COLUMNS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 131073)
GUARD = 64
SENTINEL = -777
VALUE_SENTINEL = 0x7FC00777                          # a NaN no matrix here holds
DIRTY = 0x7FC00001


def within():
    from memb_amd import _memb_within
    return _memb_within


def to_device(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


class DenseLists:
    """positions and values of `room` entries between GUARD sentinel entries on each side, cursors above a sentinel, and
    _memb_within.dense_within_to_device into them: the matrix rows n + spare floats apart with NaN behind them (NaN precedes
    every mark but a NaN one: a read beyond a row shows), a dirty workspace of exactly the size asked for."""

    def __init__(self, offsets, room):
        import torch
        self.count, self.room = len(offsets) - 1, int(room)
        self.offsets = to_device(np.asarray(offsets, dtype=np.int64))
        self.positions = torch.full((self.room + 2 * GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
        self.values = torch.full((self.room + 2 * GUARD,), VALUE_SENTINEL, dtype=torch.int32, device='cuda')
        self.cursors = torch.full((self.count + 1,), SENTINEL, dtype=torch.int64, device='cuda')

    def feed(self, matrix, thresholds, marks, base=0, lists=None, accumulate=False, capacity=None, spare=3, values=True):
        import torch
        from memb_amd import _memb_ranks
        count, n = matrix.shape
        on_device = torch.full((count + 1, n + spare), float('nan'), dtype=torch.float32, device='cuda')
        if n:
            on_device[:count, :n] = to_device(matrix)
        device_thresholds, device_marks = to_device(thresholds), to_device(np.asarray(marks, dtype=np.int64))
        device_lists = None if lists is None else to_device(lists)
        list_arguments = (0, 0, 0) if lists is None else (device_lists.data_ptr(), lists.shape[1], lists.shape[1])
        needed = within().dense_within_workspace_bytes(count, n)
        assert needed == 8 * count * -(-n // BLOCK_RUN) + (4 * count * -(-n // BLOCK_RUN) + 7) // 8 * 8
        workspace = torch.full((needed // 4 + 2,), DIRTY, dtype=torch.int32, device='cuda')
        stream = torch.cuda.current_stream().cuda_stream
        within().dense_within_to_device(
            0, on_device.data_ptr() if n else 0, count, n, n + spare, base, device_thresholds.data_ptr(), device_marks.data_ptr(),
            *list_arguments, accumulate, self.offsets.data_ptr(), self.cursors.data_ptr(), self.positions[GUARD:].data_ptr(),
            self.values[GUARD:].data_ptr() if values else 0, self.room if capacity is None else capacity,
            workspace.data_ptr() if needed else 0, needed, stream)
        assert (workspace[needed // 4:].cpu().numpy() == DIRTY).all()
        # what the call found, against the count of the rank call over the same arguments
        counts = torch.empty((count,), dtype=torch.int64, device='cuda')
        partials = torch.empty((max(_memb_ranks.dense_ranks_workspace_bytes(count, n), 8),), dtype=torch.uint8, device='cuda')
        _memb_ranks.dense_ranks_to_device(
            0, on_device.data_ptr() if n else 0, count, n, n + spare, base, device_thresholds.data_ptr(), device_marks.data_ptr(),
            *list_arguments, False, counts.data_ptr(), partials.data_ptr(), partials.numel(), stream)
        return counts.cpu().numpy()

    def read(self):
        """(positions (room,), the values' bits (room,), cursors (Q,)), the guards and the cursors' sentinel checked"""
        positions, values, cursors = self.positions.cpu().numpy(), self.values.cpu().numpy().view(np.uint32), self.cursors.cpu().numpy()
        for guard in (slice(0, GUARD), slice(GUARD + self.room, None)):
            assert (positions[guard] == SENTINEL).all() and (values[guard] == VALUE_SENTINEL).all()
        assert cursors[self.count] == SENTINEL
        return positions[GUARD:GUARD + self.room], values[GUARD:GUARD + self.room], cursors[:self.count]


def dense_call(matrix, thresholds, marks, want, base=0, lists=None, spare=3):
    """one dense call with the offsets of the right answer `want`: the lists, the cursors and the rank call's counts must
    all be that answer"""
    run = DenseLists(want[0], want[0][-1])
    counts = run.feed(matrix, thresholds, marks, base=base, lists=lists, spare=spare)
    positions, values, cursors = run.read()
    assert cursors.tolist() == np.diff(want[0]).tolist() == counts.tolist()
    assert positions.tolist() == want[1].tolist()
    assert values.tolist() == want[2].view(np.uint32).tolist()


def every_column(matrix, upto=None, base=0):
    """the answer "columns 0 .. upto of every row", stated directly"""
    count, n = matrix.shape
    upto = n if upto is None else upto
    return (np.arange(count + 1, dtype=np.int64) * upto, np.tile(base + np.arange(upto, dtype=np.int64), count),
            np.ascontiguousarray(matrix[:, :upto]).reshape(-1))


# ---- 1. the dense call ----

@pytest.fixture(scope='module')
def dense_cases():
    """{n: (matrix (3, n), thresholds, marks, the restatement's answer)} over hostile values and marks of every kind,
    worked out once and never changed; the answer for one row is its prefix"""
    whole = hostile_matrix(3, max(COLUMNS), seed=71)
    cases = {}
    for n in COLUMNS:
        matrix = np.ascontiguousarray(whole[:, :n])
        thresholds, marks = marks_over(matrix, seed=n)
        cases[n] = (matrix, thresholds, marks, within_by_the_contract(matrix, thresholds, marks))
    return cases


@pytest.mark.parametrize('n', COLUMNS)
def test_the_dense_call(native, dense_cases, n):
    matrix, thresholds, marks, want = dense_cases[n]
    for count in (1, 3):
        rows = matrix[:count]
        cut = (want[0][:count + 1], want[1][:want[0][count]], want[2][:want[0][count]])
        dense_call(rows, thresholds[:count], marks[:count], cut)
        # all precede, none precede
        dense_call(rows, np.full(count, -np.inf, dtype=np.float32), np.full(count, INT64_MAX), every_column(rows))
        dense_call(rows, np.full(count, np.nan, dtype=np.float32), np.full(count, -1), every_column(rows, 0))
        # a mark in the middle of a row of bit-equal values: the columns before it, and with a base the positions move
        equal = np.full((count, n), 0.5, dtype=np.float32)
        half = np.full(count, 0.5, dtype=np.float32)
        dense_call(equal, half, np.full(count, n // 2), every_column(equal, n // 2))
        dense_call(equal, half, np.full(count, 1000 + n // 2), every_column(equal, n // 2, base=1000), base=1000, spare=0)


# ---- 2. lists of non-candidates ----

def test_lists_of_non_candidates(native, dense_cases):
    matrix, thresholds, marks, plain = dense_cases[4097]
    everything = (np.full(3, -np.inf, dtype=np.float32), np.full(3, INT64_MAX))
    # 64 entries inside one run (the second), at a run's first and last column too
    inside = np.empty((3, 64), dtype=np.int64)
    inside[0] = BLOCK_RUN + np.arange(64) * 32
    inside[1] = 2 * BLOCK_RUN - 1 - np.arange(64)
    inside[2] = np.arange(64) * 7
    # entries in different runs, repeats, -1 padding, negatives and entries beyond the columns
    spread = np.array([[0, 2047, 2048, 4095, 4096, 2048, 0, -1, -5, 4097, 9000, INT64_MAX],
                       [4096, 4096, 4096, 1, 255, 256, 257, -1, -1, -1, -1, -(2 ** 63)],
                       [100, 2100, 4090, 100, 2100, 4090, 63, 64, 65, 5000, -2, -1]], dtype=np.int64)
    for lists in (inside, spread):
        dense_call(matrix, *everything, within_by_the_contract(matrix, *everything, 0, lists), lists=lists)
        # marks of every kind: a named column that does not precede changes nothing, one that does is taken out
        want = within_by_the_contract(matrix, thresholds, marks, 0, lists)
        named = [(q, int(c)) for q in range(3) for c in set(lists[q].tolist()) if 0 <= c < 4097]
        preceding = {(q, int(c)) for q in range(3) for c in plain[1][plain[0][q]:plain[0][q + 1]]}
        assert [entry for entry in named if entry not in preceding] and [entry for entry in named if entry in preceding]
        assert want[0][-1] == plain[0][-1] - len([entry for entry in named if entry in preceding])
        dense_call(matrix, thresholds, marks, want, lists=lists)
        # with a base the entries are positions, not columns
        moved = np.where((lists >= 0) & (lists < INT64_MAX), lists + 500, lists)
        dense_call(matrix, *everything, within_by_the_contract(matrix, *everything, 500, moved), base=500, lists=moved)


# ---- 3. accumulate ----

def test_slices_accumulate(native, dense_cases):
    matrix, thresholds, marks, _ = dense_cases[4097]
    lists = np.array([[0, 63, 64, 163, 164, 2216, 2217, 4096], [5, 5, 5, -1, 4000, 2300, 70, 9999], [-1] * 8], dtype=np.int64)
    want = within_by_the_contract(matrix, thresholds, marks, 0, lists)
    cuts = [0, 64, 164, 2217, 2281, 2381, 4097]         # slices of 64, 100 and 2053 columns, twice, the last one cut
    pieces = list(zip(cuts[:-1], cuts[1:]))
    run = DenseLists(want[0], want[0][-1])
    for start, stop in pieces:
        run.feed(matrix[:, start:stop], thresholds, marks, base=start, lists=lists, accumulate=start > 0)
    positions, values, cursors = run.read()
    assert cursors.tolist() == np.diff(want[0]).tolist()
    assert positions.tolist() == want[1].tolist() and values.tolist() == want[2].view(np.uint32).tolist()
    # in reverse order: the same set in each row, slice after slice as they were fed
    run = DenseLists(want[0], want[0][-1])
    for start, stop in reversed(pieces):
        run.feed(matrix[:, start:stop], thresholds, marks, base=start, lists=lists, accumulate=stop < 4097)
    positions, values, cursors = run.read()
    assert cursors.tolist() == np.diff(want[0]).tolist()
    for q in range(3):
        row = positions[want[0][q]:want[0][q + 1]]
        right = want[1][want[0][q]:want[0][q + 1]]
        assert sorted(row.tolist()) == right.tolist()
        fed = [c for start, stop in reversed(pieces) for c in right.tolist() if start <= c < stop]
        assert row.tolist() == fed
        lookup = dict(zip(right.tolist(), want[2].view(np.uint32)[want[0][q]:want[0][q + 1]].tolist()))
        assert values[want[0][q]:want[0][q + 1]].tolist() == [lookup[c] for c in fed]
    # no column: zero cursors, or what was there under accumulate
    run = DenseLists(want[0], want[0][-1])
    run.feed(matrix[:, :0], thresholds, marks, lists=lists)
    assert run.read()[2].tolist() == [0, 0, 0]
    run.cursors[:3] = to_device(np.array([5, 6, 7], dtype=np.int64))
    run.feed(matrix[:, :0], thresholds, marks, accumulate=True)
    assert run.read()[2].tolist() == [5, 6, 7] and (run.read()[0] == SENTINEL).all()


# ---- 4. offsets and a capacity that are too small ----

def test_writes_stay_inside_the_segments(native, dense_cases):
    matrix, thresholds, marks, want = dense_cases[4097]
    sizes = np.diff(want[0])
    assert (sizes[1:] >= 16).all()
    # row 1 gets half of its entries, and the capacity ends 5 entries before row 2's segment does. The buffers hold the
    # FULL answer between their guards, so that a destination the clamps let through wrongly still lies in allocated memory
    short = np.concatenate([[0], np.cumsum([sizes[0], sizes[1] // 2, sizes[2]])]).astype(np.int64)
    capacity = int(short[-1]) - 5
    for with_values in (True, False):
        run = DenseLists(short, want[0][-1])
        run.feed(matrix, thresholds, marks, capacity=capacity, values=with_values)
        positions, values, cursors = run.read()
        assert cursors.tolist() == sizes.tolist()                    # what each row FOUND: row 1 reports its shortfall
        assert cursors[1] > short[2] - short[1]
        for q in range(3):
            end = min(int(short[q + 1]), capacity)
            kept = end - int(short[q])
            assert positions[short[q]:end].tolist() == want[1][want[0][q]:want[0][q] + kept].tolist()
            if with_values:
                assert values[short[q]:end].tolist() == want[2].view(np.uint32)[want[0][q]:want[0][q] + kept].tolist()
        assert (positions[capacity:] == SENTINEL).all() and (values[capacity:] == VALUE_SENTINEL).all()
        if not with_values:
            assert (values == VALUE_SENTINEL).all()
    # segments that do not start at 0 and leave gaps: nothing lands in a gap
    gapped = np.array([10, 10 + sizes[0] + 7, 10 + sizes[0] + 7 + sizes[1] + 3, 0], dtype=np.int64)
    gapped[3] = gapped[2] + sizes[2]
    run = DenseLists(gapped, gapped[3] + 9)
    run.feed(matrix, thresholds, marks)
    positions, values, cursors = run.read()
    assert cursors.tolist() == sizes.tolist()
    written = np.zeros(run.room, dtype=bool)
    for q in range(3):
        held = min(int(sizes[q]), int(gapped[q + 1] - gapped[q]))
        written[gapped[q]:gapped[q] + held] = True
        assert positions[gapped[q]:gapped[q] + held].tolist() == want[1][want[0][q]:want[0][q] + held].tolist()
    assert (positions[~written] == SENTINEL).all() and (values[~written] == VALUE_SENTINEL).all()


# ---- 5. the fused call and the fallback ----

N_CANDIDATES = 1100


def fused_case_of(reader, count, dim, seed):
    """(queries, rows, matrix, thresholds, marks, lists): 1100 candidates with repeated rows -- bit-equal cosines at
    different positions, in every slice of 64 --, five queries, two of them the unit rows of repeated candidates"""
    import torch
    rng = np.random.default_rng(seed)
    host_rows = rng.integers(0, count, size=N_CANDIDATES).astype(np.uint32)
    host_rows[::7] = host_rows[3]
    host_rows[5::50] = host_rows[9]
    host_rows[20] = 0xFFFFFFFF                          # not in the model: cosine 0
    rows = torch.from_numpy(host_rows.view(np.int32)).cuda()
    queries = torch.from_numpy(rng.normal(size=(5, dim)).astype(np.float32)).cuda()
    queries[0] = reader.unit_rows_embedding_device(rows[3:4])[0]
    queries[1] = reader.unit_rows_embedding_device(rows[9:10])[0]
    matrix = reader.similarity_matrix_device(queries, rows).cpu().numpy()
    columns = np.array([7 * 64, 5 + 50 * 11, 14, 700, 21])
    thresholds = matrix[np.arange(5), columns].copy()
    marks = np.array([columns[0], columns[1], columns[2], -1, INT64_MAX], dtype=np.int64)
    lists = np.random.default_rng(seed + 1).integers(-2, N_CANDIDATES + 3, size=(5, 9)).astype(np.int64)
    lists[0, :3] = (0, 7, 7 * 100)                      # among the tied best of query 0, in different slices
    lists[:, 4] = lists[:, 5]
    return queries, rows, matrix, thresholds, marks, lists


def device_lists(result):
    return tuple(part.cpu().numpy() for part in result[:3])


def test_the_fused_call(native, make_model):
    import torch
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, matrix, thresholds, marks, lists = fused_case_of(reader, 3000, 300, seed=72)
    assert reader.last_query_matrix_kernel == 'query_matrix_trained'
    context = reader._impl.context_handle()
    least = within().query_within_workspace_bytes(context, 5, N_CANDIDATES, minimal=True)
    assert least == 40 + 24 + 4 * 5 * 64 < within().query_within_workspace_bytes(context, 5, N_CANDIDATES) == 40 + 24 + 4 * 5 * N_CANDIDATES
    for exclude in (None, lists):
        want = within_by_the_contract(matrix, thresholds, marks, 0, exclude)
        assert want[0][1] >= 50                                        # some sixty bit-equal cosines come first for query 0
        dense_call(matrix, thresholds, marks, want, lists=exclude)      # the dense call over the same matrix is that answer
        arguments = (queries, rows, to_device(thresholds), to_device(marks))
        device_exclude = None if exclude is None else to_device(exclude)
        got = reader.similarity_within_device(*arguments, exclude=device_exclude)
        assert reader.last_within_kernel == FUSED
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float32
        assert same_lists(device_lists(got), want)
        assert np.diff(want[0]).tolist() == reader.similarity_ranks_device(*arguments, exclude=device_exclude).cpu().numpy().tolist()
        # the minimal workspace (eighteen slices of 64) and one in between (slices of 256), dirty, of exactly that size
        for size in (least, least + 4 * 5 * 192):
            workspace = torch.full((size // 4 + 2,), DIRTY, dtype=torch.int32, device='cuda').view(torch.uint8)[:size]
            assert same_lists(device_lists(reader.similarity_within_device(*arguments, exclude=device_exclude, workspace=workspace)), want)
        with pytest.raises(RuntimeError, match='workspace too small'):
            reader.similarity_within_device(*arguments, workspace=workspace[:least - 8])
        without = reader.similarity_within_device(*arguments, exclude=device_exclude, return_values=False)
        assert without[2] is None and without[1].cpu().numpy().tolist() == want[1].tolist()
    # marks=None lists the strictly greater cosines; the numpy form; nothing to list
    assert same_lists(device_lists(reader.similarity_within_device(queries, rows, to_device(thresholds))),
                      within_by_the_contract(matrix, thresholds, [-1] * 5))
    assert same_lists(reader.similarity_within(queries.cpu().numpy(), rows.cpu().numpy().view(np.uint32), thresholds, marks, exclude=lists),
                      within_by_the_contract(matrix, thresholds, marks, 0, lists))
    empty = reader.similarity_within_device(queries, rows[:0], to_device(thresholds), to_device(marks))
    assert empty[0].cpu().numpy().tolist() == [0] * 6 and empty[1].shape == (0,) and reader.last_within_kernel == FUSED
    assert reader.similarity_within_device(queries[:0], rows, to_device(thresholds[:0]))[0].cpu().numpy().tolist() == [0]
    assert reader.last_within_kernel == ''
    # rows=None: every row of the model, positions are row ids
    everything = reader.similarity_matrix_device(queries, torch.arange(3000, dtype=torch.int32, device='cuda')).cpu().numpy()
    radius = np.sort(everything, axis=1)[:, -40].copy()
    want = within_by_the_contract(everything, radius, [INT64_MAX] * 5)
    assert np.diff(want[0]).min() >= 40
    assert same_lists(device_lists(reader.similarity_within_device(queries, None, to_device(radius), to_device(np.full(5, INT64_MAX)))), want)
    # offsets given: the fill alone, and what each query found; a segment too short keeps the head of its list
    want = within_by_the_contract(matrix, thresholds, marks, 0, lists)
    short = want[0].copy()
    short[1:] -= 10                                                     # query 0 loses its last ten entries
    offsets, positions, values, found = reader.similarity_within_device(
        queries, rows, to_device(thresholds), to_device(marks), exclude=to_device(lists), offsets=to_device(short), capacity=int(want[0][-1]))
    assert found.cpu().numpy().tolist() == np.diff(want[0]).tolist() and offsets.cpu().numpy().tolist() == short.tolist()
    positions = positions.cpu().numpy()
    assert positions[:short[1]].tolist() == want[1][:short[1]].tolist()
    assert positions[short[1]:short[5]].tolist() == want[1][want[0][1]:].tolist()


def test_a_uniform_model_takes_the_fallback(native, make_model, monkeypatch):
    import memb_amd.reader
    path, _ = make_model(1500, 300, 'uniform', 8)
    reader = native.Reader(path)
    monkeypatch.setattr(memb_amd.reader, 'QUERY_DEVICE_SLICE', 500)   # three slices, the last shorter: accumulate
    queries, rows, matrix, thresholds, marks, lists = fused_case_of(reader, 1500, 300, seed=73)
    want = within_by_the_contract(matrix, thresholds, marks, 0, lists)
    dense_call(matrix, thresholds, marks, want, lists=lists)
    got = reader.similarity_within_device(queries, rows, to_device(thresholds), to_device(marks), exclude=to_device(lists))
    assert reader.last_within_kernel == DENSE
    assert same_lists(device_lists(got), want)
    assert np.diff(want[0]).tolist() == reader.similarity_ranks_device(
        queries, rows, to_device(thresholds), to_device(marks), exclude=to_device(lists)).cpu().numpy().tolist()
    empty = reader.similarity_within_device(queries, rows[:0], to_device(thresholds))
    assert empty[0].cpu().numpy().tolist() == [0] * 6 and reader.last_within_kernel == 'within_starts'


# ---- 6. words ----

def test_words_equal_a_host_reader(native, make_model):
    path, words = make_model(3000, 300, 'trained', 4)
    reader, host = native.Reader(path), native.Reader(path, device='cpu')
    rng = np.random.default_rng(74)
    first = [words[i] for i in rng.integers(0, 3000, size=6)] + ['no such word é', words[5]]
    second = [words[i] for i in rng.integers(0, 3000, size=6)] + [words[7], 'no such word é']
    offsets, found = (part.cpu().numpy() for part in reader.closer_than_device(first, second))
    counts = reader.count_closer_than(first, second)
    assert np.diff(offsets).tolist() == np.maximum(counts, 0).tolist() and counts[-2:].tolist() == [-1, -1]
    vocabulary = reader.keys()
    for i in (0, 3, 6, 7):
        closer = reader.closer_than(first[i], second[i])
        assert closer == host.closer_than(first[i], second[i]) == [vocabulary[row] for row in found[offsets[i]:offsets[i + 1]]]
    assert reader.closer_than_device([], [])[0].cpu().numpy().tolist() == [0]
    with pytest.raises(ValueError, match='one word per pair'):
        reader.closer_than_device(first, second[:2])
    # the nearest words of a word are the ones closer than the last of them
    nearest = [word for word, _ in reader.most_similar([words[40]], k=5)[0]]
    assert sorted(reader.closer_than(words[40], nearest[4])) == sorted(nearest[:4])
    asked = [words[40], 'no such word é', words[17], words[40]]
    got = reader.words_within(asked, 0.15)
    assert got == host.words_within(asked, 0.15)
    assert got[1] == [] and got[0] == got[3] and len(got[0]) >= 1 and all(cosine >= np.float32(0.15) for _, cosine in got[0])
    assert words[40] not in [word for word, _ in got[0]]
    offsets, found, values = (part.cpu().numpy() for part in reader.words_within_device(asked, 0.15))
    assert [vocabulary[row] for row in found[offsets[2]:offsets[3]]] == [word for word, _ in got[2]]
    assert values[offsets[2]:offsets[3]].tolist() == [np.float32(cosine) for _, cosine in got[2]]
    assert reader.words_within([], 0.5) == [] and reader.words_within_device([], 0.5)[0].cpu().numpy().tolist() == [0]


def test_argument_errors(native, make_model):
    import torch
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, matrix, thresholds, marks, lists = fused_case_of(reader, 3000, 300, seed=72)
    good = (queries, rows, to_device(thresholds), to_device(marks))
    offsets = torch.zeros(6, dtype=torch.int64, device='cuda')
    with pytest.raises(TypeError, match='thresholds'):
        reader.similarity_within_device(queries, rows, thresholds)
    with pytest.raises(ValueError, match='marks'):
        reader.similarity_within_device(queries, rows, good[2], good[3][:4])
    with pytest.raises(ValueError, match='64'):
        reader.similarity_within_device(*good, exclude=torch.zeros((5, 65), dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError, match='workspace'):
        reader.similarity_within_device(*good, workspace=torch.zeros(4096, dtype=torch.float32, device='cuda'))
    with pytest.raises(TypeError, match='offsets'):
        reader.similarity_within_device(*good, offsets=offsets.int())
    with pytest.raises(TypeError, match='offsets'):
        reader.similarity_within_device(*good, offsets=np.zeros(6, dtype=np.int64))
    with pytest.raises(ValueError, match='offsets'):
        reader.similarity_within_device(*good, offsets=offsets[:5])
    with pytest.raises(ValueError, match='offsets'):
        reader.similarity_within_device(*good, offsets=offsets.cpu())
    with pytest.raises(ValueError, match='capacity'):
        reader.similarity_within_device(*good, offsets=offsets, capacity=-1)
    with pytest.raises(ValueError, match='capacity'):
        reader.similarity_within_device(*good, capacity=10)
    with pytest.raises(TypeError, match='min_cosine'):
        reader.words_within_device(['a'], None)


# ---- 7. a captured graph ----

def test_captured_into_a_graph(native, make_model):
    import torch
    path, _ = make_model(3000, 300, 'trained', 4)
    reader = native.Reader(path)
    queries, rows, matrix, thresholds, marks, lists = fused_case_of(reader, 3000, 300, seed=72)
    context = reader._impl.context_handle()
    workspace = torch.empty((within().query_within_workspace_bytes(context, 5, N_CANDIDATES, minimal=True) + 4 * 5 * 192,), dtype=torch.uint8,
                            device='cuda')          # slices of 256 candidates: five of them
    want = within_by_the_contract(matrix, thresholds, marks, 0, lists)
    arguments = (queries, rows, to_device(thresholds), to_device(marks))
    given = dict(exclude=to_device(lists), offsets=to_device(want[0]), capacity=int(want[0][-1]), workspace=workspace)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eager = reader.similarity_within_device(*arguments, **given)   # (also the warm-up)
    stream.synchronize()
    assert same_lists(device_lists(eager), want) and eager[3].cpu().numpy().tolist() == np.diff(want[0]).tolist()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        _, positions, values, found = reader.similarity_within_device(*arguments, **given)
    for _ in range(2):
        positions.fill_(SENTINEL)
        values.fill_(0)
        found.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(positions, eager[1]) and torch.equal(values.view(torch.int32), eager[2].view(torch.int32))
        assert torch.equal(found, eager[3])
