"""Several threads at once on the sliced searches of one Reader: similarity_topk_device (plain and with exclude=),
cosmul_topk_device, similarity_ranks_device, bag_similarity_topk_device, analogies_device and analogy_ranks_device -- each a
host loop of three to five launches per slice through one context, one kernel table and one lazily staged model -- next to
one another, next to decodes and chunked pooling, next to the host-returning most_similar, as a fresh reader's first use,
and on two readers of one file. The reference is a Reader(path, device='cpu') of the same file (the host tests tie it to
tests/*_reference.py) and, for the decode, oracle.OracleReader: every expected answer is worked out serially on the host
BEFORE a thread starts; no GPU call ever serves as the reference of another. Values are compared as bits, positions, rows
and counts for equality."""
import numpy as np
import pytest

import oracle
from conftest import bits_equal
from query_topk_reference import same_topk
from ranks_reference import INT64_MAX
from test_gpu_concurrency import run_threads
from test_gpu_query_bags import corpus_with_ties
from test_gpu_ranks import lists_over

pytestmark = pytest.mark.gpu

N_ROWS = 3000
N_CANDIDATES = 1100      # eighteen slices of 64 under a minimal workspace
N_QUERIES = 3
DIRTY = 0x7FC00001
UNKNOWN = 'no such word é'


class Case:
    """A model file, its host reader and the candidates every searcher shares: 1100 ids with repeated rows -- bit-equal
    cosines in every slice of 64 --, a miss of each kind, and 1100 bags of which every third repeats the one before"""

    def __init__(self, native, path, words):
        self.path, self.words = path, words
        self.host = native.Reader(path, device='cpu')
        self.keys = self.host.keys()
        self.row_of = {word: row for row, word in enumerate(self.keys)}
        rng = np.random.default_rng(81)
        rows = rng.integers(0, N_ROWS, size=N_CANDIDATES).astype(np.uint32)
        rows[::7] = rows[3]
        rows[5::50] = rows[9]
        rows[20], rows[21] = 0xFFFFFFFF, N_ROWS
        self.rows = rows
        self.bag_rows, self.bag_offsets = corpus_with_ties(self.host, N_CANDIDATES, 82)
        self.calls = {}      # seed -> the calls of searcher_calls, worked out once
        self.uploaded = None


@pytest.fixture(scope='module')
def cases(native, make_model):
    kept = {}

    def case(bits):
        if bits not in kept:
            kept[bits] = Case(native, *make_model(N_ROWS, 300, 'trained', bits))
        return kept[bits]

    return case


def upload(array):
    import torch
    array = np.ascontiguousarray(array)
    return torch.from_numpy(array.view(np.int32) if array.dtype == np.uint32 else array).cuda()


class Call:
    """One device call with its inputs on the device already and the host reader's answer: run(reader, workspace) makes
    it, least(reader) is the size of its minimal workspace (None: it takes none)"""

    def __init__(self, name, want, run, least=None):
        self.name, self.want, self.run, self.least = name, want, run, least

    def same(self, got):
        if isinstance(self.want, tuple):
            return same_topk(tuple(part.cpu().numpy() for part in got), self.want)
        return got.cpu().numpy().dtype == np.int64 and got.cpu().numpy().tolist() == self.want.tolist()


def pairs_as_arrays(pairs, k, row_of):
    """the (word, value) lists of analogies as analogies_device's (values, rows): empty slots behind them"""
    values = np.full((len(pairs), k), -np.inf, dtype=np.float32)
    rows = np.full((len(pairs), k), -1, dtype=np.int64)
    for q, answer in enumerate(pairs):
        for slot, (word, value) in enumerate(answer):
            values[q, slot], rows[q, slot] = value, row_of[word]
    return values, rows


def searcher_calls(case, seed):
    """The calls of one searcher -- queries of its own from a seeded generator -- and what the host reader answers to each,
    worked out here, on the calling thread, before any other thread exists."""
    if seed in case.calls:
        return case.calls[seed]
    from memb_amd import _memb_cosmul, _memb_ranks
    host, rows, words = case.host, case.rows, case.words
    if case.uploaded is None:
        case.uploaded = (upload(rows), upload(case.bag_rows), upload(case.bag_offsets.astype(np.uint32)))
    device_rows, device_bag_rows, device_bag_offsets = case.uploaded
    rng = np.random.default_rng(1000 + seed)
    repeated = (3, 9)[seed % 2]
    tied = np.nonzero(rows == rows[repeated])[0]
    queries = rng.standard_normal((N_QUERIES, host.dim)).astype(np.float32)
    queries[0] = host.unit_rows_embedding(rows[repeated:repeated + 1])[0]   # the unit row of a candidate at many positions
    lists = lists_over(N_QUERIES, N_CANDIDATES, seed=2000 + seed)
    lists[0, :3] = tied[[0, 1, -1]]                                          # among query 0's tied best, in different slices
    device_queries, device_lists = upload(queries), upload(lists)
    calls = []

    # similarity_topk_device: k 1, 10 and 64, with and without a list (which of them alternates with the seed)
    for k, excluded in ((1, seed % 2 == 1), (10, seed % 2 == 0), (64, seed % 2 == 1)):
        want = host.similarity_topk(queries, rows, k, exclude=lists if excluded else None)
        calls.append(Call(
            'similarity_topk_device k {} {}'.format(k, 'with a list' if excluded else 'plain'), want,
            lambda reader, workspace, k=k, excluded=excluded: reader.similarity_topk_device(
                device_queries, device_rows, k, exclude=device_lists if excluded else None, workspace=workspace),
            lambda reader, k=k: reader._impl.query_topk_workspace_bytes(N_QUERIES, N_CANDIDATES, k, minimal=True)))
    assert len(np.unique(calls[1].want[0][0])) < 10   # (ties among the best of query 0)

    # cosmul_topk_device: an analogy whose words are candidates themselves, and a question of two terms
    term_rows = np.concatenate([rows[[repeated, 70, 200]], rng.integers(0, N_ROWS, size=2).astype(np.uint32)])
    terms = host.unit_rows_embedding(term_rows)
    offsets, negatives_from = [0, 3, 5], [2, 4]
    device_terms = upload(terms)
    want = host.cosmul_topk(terms, offsets, negatives_from, rows, 10, exclude=lists[:2])
    calls.append(Call(
        'cosmul_topk_device', want,
        lambda reader, workspace: reader.cosmul_topk_device(
            device_terms, offsets, negatives_from, device_rows, 10, exclude=device_lists[:2], workspace=workspace),
        lambda reader: _memb_cosmul.query_cosmul_workspace_bytes(reader._impl.context_handle(), 5, 2, N_CANDIDATES, 10, minimal=True)))

    # similarity_ranks_device: the rank of a tied candidate, the strictly greater and the greater-or-equal cosines
    matrix = host.similarity_matrix(queries, rows)
    columns = np.array([tied[tied.size // 2], rng.integers(0, N_CANDIDATES), rng.integers(0, N_CANDIDATES)])
    thresholds = matrix[np.arange(N_QUERIES), columns].copy()
    marks = np.array([columns[0], -1, INT64_MAX], dtype=np.int64)
    want = host.similarity_ranks(queries, rows, thresholds, marks, exclude=lists)
    assert want[0] >= tied.size // 2 - 3 >= 8         # (the tied candidates before the mark, but those the list names)
    device_thresholds, device_marks = upload(thresholds), upload(marks)
    calls.append(Call(
        'similarity_ranks_device', want,
        lambda reader, workspace: reader.similarity_ranks_device(
            device_queries, device_rows, device_thresholds, device_marks, exclude=device_lists, workspace=workspace),
        lambda reader: _memb_ranks.query_ranks_workspace_bytes(reader._impl.context_handle(), N_QUERIES, N_CANDIDATES, minimal=True)))

    # bag_similarity_topk_device
    want = host.bag_similarity_topk(queries, case.bag_rows, case.bag_offsets, 10)
    calls.append(Call(
        'bag_similarity_topk_device', want,
        lambda reader, workspace: reader.bag_similarity_topk_device(
            device_queries, device_bag_rows, device_bag_offsets, 10, workspace=workspace),
        lambda reader: reader._impl.query_bags_topk_workspace_bytes(N_QUERIES, N_CANDIDATES, 10, minimal=True)))

    # analogies_device and analogy_ranks_device over the whole model, an unknown word among the questions
    picked = [words[int(i)] for i in rng.integers(0, N_ROWS, size=9)]
    positive = [[picked[0], picked[1]], [picked[2], UNKNOWN], [picked[3]], [(picked[4], 0.5), picked[5]]]
    negative = [[picked[6]], [picked[7]], [], [picked[8]]]
    want = pairs_as_arrays(host.analogies(positive, negative, 5), 5, case.row_of)
    assert (want[1][1] == -1).all() and (want[1][[0, 2, 3]] >= 0).all()
    calls.append(Call('analogies_device', want, lambda reader, workspace: reader.analogies_device(positive, negative, 5)))
    expected = [case.keys[int(want[1][0, 2])], picked[0], UNKNOWN, case.keys[int(want[1][3, 0])]]
    want = host.analogy_ranks(positive, negative, expected)
    assert want.tolist() == [3, 0, 0, 1]
    calls.append(Call('analogy_ranks_device', want, lambda reader, workspace: reader.analogy_ranks_device(positive, negative, expected)))

    case.calls[seed] = calls
    return calls


def searcher(readers, calls, index, minimal):
    """Thread `index`: every call of `calls` in an order rotated by the index, call i on readers[i % len(readers)], on the
    default stream (thread 0) or a stream of its own; with `minimal` under a dirty workspace of exactly the minimal size
    with two guard words behind it. One synchronisation at the end, then every comparison."""
    def target(failures):
        import torch
        stream = torch.cuda.current_stream() if index == 0 else torch.cuda.Stream()
        order = calls[index % len(calls):] + calls[:index % len(calls)]
        results = []
        with torch.cuda.stream(stream):
            for i, call in enumerate(order):
                guard, needed = None, 0
                if minimal and call.least is not None:
                    needed = call.least(readers[i % len(readers)])
                    assert needed and needed % 8 == 0
                    guard = torch.full((needed // 4 + 2,), DIRTY, dtype=torch.int32, device='cuda')
                got = call.run(readers[i % len(readers)], None if guard is None else guard.view(torch.uint8)[:needed])
                results.append((call, got, guard, needed))
        torch.cuda.synchronize()
        for call, got, guard, needed in results:
            if not call.same(got):
                failures.append('thread {}{}: {} differs from the host reader'.format(index, ' (minimal workspace)' if minimal else '', call.name))
            if guard is not None and not (guard[needed // 4:].cpu().numpy() == DIRTY).all():
                failures.append('thread {}: {} wrote behind its workspace'.format(index, call.name))

    return target


def ready():
    """every upload of the calling thread has arrived: the threads' own streams may read them"""
    import torch
    torch.cuda.synchronize()


@pytest.mark.parametrize('bits', (4, 6))
def test_one_reader_many_searchers(native, cases, bits):
    case = cases(bits)
    reader = native.Reader(case.path)
    targets = [searcher([reader], searcher_calls(case, seed), seed, minimal=seed % 2 == 1) for seed in range(6)]
    ready()
    failures = run_threads(targets)
    assert not failures, failures[:5]
    assert reader.host_rows_decoded == 0


def test_searches_next_to_decodes_and_pooling(native, cases):
    """Four searchers, a thread that alternates decodes of 20 000 rows with chunked pooling -- launches of other block
    sizes and LDS amounts through the same kernel table --, and a thread in most_similar, which brings its answer to the
    host. Their references: the checker's rows, the host reader's bags_embedding and its most_similar."""
    import torch
    case = cases(4)
    reader = native.Reader(case.path)
    checker = oracle.OracleReader(case.path)
    rng = np.random.default_rng(83)
    lookups, pooled = [], []
    for step in range(2):
        rows = rng.integers(0, N_ROWS, size=20000).astype(np.uint32)
        rows[::97] = 0xFFFFFFFF
        lookups.append((upload(rows), checker.rows_embedding(rows)))
        # sixty bags of 1 .. 700 entries: up to eleven chunks of 64, an empty bag among them
        lengths = rng.integers(1, 700, size=60)
        lengths[7] = 0
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
        entries = rng.integers(0, N_ROWS, size=int(offsets[-1])).astype(np.uint32)
        entries[::89] = 0xFFFFFFFF
        mode = ('mean', 'sum')[step]
        pooled.append((upload(entries), upload(offsets), mode, case.host.bags_embedding(entries, offsets, mode=mode, reduction='chunked')))
    asked = [[case.words[int(i)] for i in rng.integers(0, N_ROWS, size=5)] + [UNKNOWN] for _ in range(3)]
    nearest = [case.host.most_similar(words, k=6) for words in asked]
    assert all(len(answer[0]) == 6 and answer[5] == [] for answer in nearest)

    def decoder(failures):
        results = []
        with torch.cuda.stream(torch.cuda.Stream()):
            for step in range(2):
                results.append(('rows_embedding_device', reader.rows_embedding_device(lookups[step][0]), lookups[step][1]))
                entries, offsets, mode, want = pooled[step]
                results.append(('bags_embedding_device chunked ' + mode, reader.bags_embedding_device(entries, offsets, mode=mode, reduction='chunked'), want))
        torch.cuda.synchronize()
        for name, got, want in results:
            if not bits_equal(got.cpu().numpy(), want):
                failures.append('{} differs from its reference'.format(name))

    def host_caller(failures):
        for words, want in zip(asked, nearest):
            got = reader.most_similar(words, k=6)
            same = len(got) == len(want) and all(
                [word for word, _ in a] == [word for word, _ in b]
                and bits_equal(np.array([value for _, value in a], dtype=np.float32), np.array([value for _, value in b], dtype=np.float32))
                for a, b in zip(got, want))
            if not same:
                failures.append('most_similar differs from the host reader')

    targets = [searcher([reader], searcher_calls(case, seed), seed, minimal=seed % 2 == 1) for seed in range(4)]
    ready()
    failures = run_threads(targets + [decoder, host_caller])
    assert not failures, failures[:5]


def test_first_fused_use_from_several_threads(native, cases):
    """A fresh Reader whose first use is four different fused calls from four threads at once: the model is staged once
    and every caller sees it finished."""
    case = cases(4)
    calls = searcher_calls(case, 0)
    first = [next(call for call in calls if call.name.startswith(name)) for name in
             ('similarity_topk_device k 10', 'cosmul_topk_device', 'similarity_ranks_device', 'bag_similarity_topk_device')]
    reader = native.Reader(case.path)
    ready()
    failures = run_threads([searcher([reader], [call], index, minimal=index % 2 == 1) for index, call in enumerate(first)])
    assert not failures, failures[:5]


def test_two_readers_of_one_file_alternating(native, cases):
    """Two Readers of one file, every thread alternating between them call by call: nothing may be kept per file or per
    process where it should be per reader."""
    case = cases(4)
    readers = [native.Reader(case.path), native.Reader(case.path)]
    targets = [searcher(readers, searcher_calls(case, seed), seed, minimal=seed % 2 == 1) for seed in range(4)]   # (call i on readers[i % 2])
    ready()
    failures = run_threads(targets)
    assert not failures, failures[:5]
