"""Several threads on one Reader or ReadersUnion at once. The reference's read methods are re-entrant (src/reader.h:19-27);
here every call of the device word API (resolve_rows_device, resolve_packed_device, batch_embedding_device,
ReadersUnion.batch_embedding_device) packs its words into a word batch that no other call in flight uses, next to the host
path (batch_embedding: the reader's leased C++ batch) and device row lookups that change the launch geometry of later ones.
Every result is compared bit for bit with the CPU checker (oracle.OracleReader: the reference's lower_bound + strcmp and
its decoder restated). Also the guard behind it all: a WordBatch handed to two calls at once makes the second a
RuntimeError, never a shared batch."""
import threading
import traceback

import numpy as np
import pytest

import oracle
from conftest import bits_equal

pytestmark = pytest.mark.gpu

MISSING = 0xFFFFFFFF
VOCAB = 30000
# the small batches of a serving loop, both sides of the pooled fill's threshold (8192 words), and a chunked fill
# (70 000: runs of jobs looked up while later ones are filled)
SIZES = [1, 63, 5000, 8191, 8192, 8193, 70000]
LARGE = 300000
KINDS = ['rows', 'bytes', 'numpy', 'device', 'embed']


@pytest.fixture(scope='module')
def model(make_model):
    """A trained 4-bit model of 30 000 words and a pool of queries with the checker's row for each: known words, misses,
    the empty word, non-ASCII words, and (at the end) three words long enough that a job of a small batch overflows its
    region, which makes the fill start again with larger regions."""
    path, words = make_model(VOCAB, 300, 'trained', 4)
    checker = oracle.OracleReader(path)
    extra = ['', 'naïve-日本語', 'fehlt-ä-ß', '没有', '\U0001f600'] + ['miss-{}'.format(i) for i in range(500)]
    extra += [words[i] + 'é' for i in range(200)] + [words[i] + 'z' for i in range(200, 400)]
    longs = ['y' * 5000, 'x' * 3001 + 'é', words[0] * 400]
    pool = list(words) + extra + longs
    return path, checker, pool, checker.resolve_rows(pool), len(pool) - len(longs)


def draw(model, rng, size):
    """`size` queries and their rows: fresh str objects for the non-ASCII words (no cached UTF-8 form: the fill prepares
    them through the C API and fills again), the long words somewhere in every batch of 63 words and more"""
    _, _, pool, rows, short = model
    index = rng.integers(0, short, size=size)
    if size >= 63:
        index[rng.choice(size, size=len(pool) - short, replace=False)] = np.arange(short, len(pool))
    words = [pool[i] if pool[i].isascii() else (pool[i] + '.')[:-1] for i in index]
    return words, rows[index]


def packed(words):
    encoded = [word.encode('utf-8') for word in words]
    offsets = np.zeros(len(words) + 1, dtype=np.uint32)
    np.cumsum([len(e) for e in encoded], out=offsets[1:])
    return b''.join(encoded), offsets


def run_threads(targets):
    """Start every target at once (behind a barrier) and join them all. Returns the failures -- mismatches and exceptions
    alike: no thread may die silently."""
    failures = []
    finished = []
    barrier = threading.Barrier(len(targets), timeout=120)

    def wrap(index, target):
        try:
            barrier.wait()
            target(failures)
            finished.append(index)
        except BaseException:   # (collected, asserted on the main thread)
            failures.append('thread {}: {}'.format(index, traceback.format_exc()))

    threads = [threading.Thread(target=wrap, args=(index, target)) for index, target in enumerate(targets)]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join(timeout=300)
    assert not any(thread.is_alive() for thread in threads), 'a thread did not finish'
    assert failures or sorted(finished) == list(range(len(targets)))
    return failures


def word_api_caller(readers, model, seed, plan, use_default_stream):
    """A thread's handful of device word calls -- call k on readers[k % len(readers)] -- on a stream of its own (or the
    default one). Every result is checked after torch.cuda.synchronize()."""
    import torch
    checker = model[1]

    def target(failures):
        rng = np.random.default_rng(seed)
        stream = torch.cuda.current_stream() if use_default_stream else torch.cuda.Stream()
        results = []
        with torch.cuda.stream(stream):
            for k, (kind, size) in enumerate(plan):
                reader = readers[k % len(readers)]
                words, expected = draw(model, rng, size)
                keep = None
                if kind == 'rows':
                    got = reader.resolve_rows_device(words)
                elif kind == 'bytes':
                    got = reader.resolve_packed_device(*packed(words))
                elif kind == 'numpy':
                    blob, offsets = packed(words)
                    got = reader.resolve_packed_device(np.frombuffer(blob, dtype=np.uint8), offsets.astype(np.int64))
                elif kind == 'device':
                    blob, offsets = packed(words)
                    keep = (torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda(),
                            torch.from_numpy(offsets.view(np.int32)).cuda())
                    got = reader.resolve_packed_device(*keep)
                else:
                    got = reader.batch_embedding_device(words)
                results.append((kind, size, got, expected, keep))
        torch.cuda.synchronize()
        for kind, size, got, expected, _ in results:
            if kind == 'embed':
                ok = bits_equal(got.cpu().numpy(), checker.rows_embedding(expected))
            else:
                ok = got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), expected)
            if not ok:
                failures.append('seed {}: {} of {} words differs from the checker'.format(seed, kind, size))

    return target


def plans(threads, large_in):
    """Per thread five calls of growing size (the pinned buffers grow while other calls are in flight), every kind once;
    every size of SIZES in several threads. Thread `large_in` ends with two batches of 300 000 words."""
    result = []
    for t in range(threads):
        sizes = sorted(SIZES[(t + k) % len(SIZES)] for k in (0, 3, 6, 9, 12))
        plan = [(KINDS[(t + k) % len(KINDS)], size) for k, size in enumerate(sizes)]
        if t == large_in:
            plan[-1] = ('bytes', LARGE)
            plan.append(('rows', LARGE + 1))
        result.append(plan)
    return result


def test_one_reader_many_callers(native, model):
    reader = native.Reader(model[0])
    targets = [word_api_caller([reader], model, 100 + t, plan, use_default_stream=t == 0)
               for t, plan in enumerate(plans(7, large_in=3))]
    failures = run_threads(targets)
    assert not failures, failures[:5]
    assert reader.host_rows_decoded == 0


def test_word_api_next_to_the_host_path_and_large_row_lookups(native, model):
    """The same mix with two more threads: batch_embedding of 4 096 words and more (the reader's own leased C++ batch,
    DEVICE_SEARCH_THRESHOLD), and rows_embedding_device of more than 524 000 rows -- random ones with order='random'
    alternating with key-order dumps. What the reader has seen of the order picks the block size of later large launches
    (orderSeen): a concurrent call may change the launch geometry of another, never a bit of its result."""
    import torch
    path, checker = model[0], model[1]
    reader = native.Reader(path)
    # the checker's rows of every key on the device, a zero row behind them for MISSING
    table = torch.from_numpy(np.concatenate([checker.rows_embedding(np.arange(VOCAB, dtype=np.uint32)),
                                             np.zeros((1, 300), dtype=np.float32)])).cuda()

    def host_caller(failures):
        rng = np.random.default_rng(7)
        for size in (4096, 6000, 9000, 20000):
            words, _ = draw(model, rng, size)
            if not bits_equal(reader.batch_embedding(words), checker.batch_embedding(words)):
                failures.append('batch_embedding of {} words differs from the checker'.format(size))

    def row_caller(failures):
        rng = np.random.default_rng(8)
        with torch.cuda.stream(torch.cuda.Stream()):
            for step in range(4):
                if step % 2 == 0:
                    rows = rng.integers(0, VOCAB, size=530000).astype(np.uint32)
                    rows[::97] = MISSING
                    got = reader.rows_embedding_device(torch.from_numpy(rows.view(np.int32)).cuda(), order='random')
                else:
                    rows = np.repeat(np.arange(VOCAB, dtype=np.uint32), 18)   # 540 000 rows in key order
                    got = reader.rows_embedding_device(torch.from_numpy(rows.view(np.int32)).cuda())
                expected = table[torch.from_numpy(np.where(rows == MISSING, VOCAB, rows).astype(np.int64)).cuda()]
                if not torch.equal(got.view(torch.int32), expected.view(torch.int32)):
                    failures.append('rows_embedding_device step {} differs from the checker'.format(step))

    targets = [word_api_caller([reader], model, 200 + t, plan, use_default_stream=t == 0)
               for t, plan in enumerate(plans(6, large_in=1))]
    failures = run_threads(targets + [host_caller, row_caller])
    assert not failures, failures[:5]


def test_first_use_from_several_threads(native, model):
    """A fresh Reader whose first calls come from four threads at once: the model, the keys and the hash table over them
    are staged once, and every caller sees them finished."""
    import torch
    path, checker = model[0], model[1]
    reader = native.Reader(path)
    rows = np.random.default_rng(9).integers(0, VOCAB, size=20000).astype(np.uint32)
    expected_rows = checker.rows_embedding(rows)

    def words_caller(seed, size, kind):
        def target(failures):
            words, expected = draw(model, np.random.default_rng(seed), size)
            got = reader.resolve_rows_device(words) if kind == 'rows' else reader.resolve_packed_device(*packed(words))
            torch.cuda.synchronize()
            if not np.array_equal(got.cpu().numpy().view(np.uint32), expected):
                failures.append('first use: {} of {} words differs from the checker'.format(kind, size))
        return target

    def rows_caller(failures):
        got = reader.rows_embedding_device(torch.from_numpy(rows.view(np.int32)).cuda())
        torch.cuda.synchronize()
        if not bits_equal(got.cpu().numpy(), expected_rows):
            failures.append('first use: rows_embedding_device differs from the checker')

    failures = run_threads([words_caller(1, 5000, 'rows'), words_caller(2, 70000, 'bytes'), rows_caller, rows_caller])
    assert not failures, failures[:5]


@pytest.mark.parametrize('mode', ['concatenate', 'average'])
def test_one_union_many_callers(native, make_model, mode):
    import torch
    path_a, words_a = make_model(6000, 300, 'trained', 4, seed=1)
    path_b, _ = make_model(5000, 300, 'trained', 4, seed=2)
    # (one word generator: b knows the first 5000 of a's 6000 words and misses the rest)
    union = native.ReadersUnion([native.Reader(path_a), native.Reader(path_b)], mode)
    checkers = [oracle.OracleReader(path_a), oracle.OracleReader(path_b)]
    pool = list(words_a) + ['miss-{}'.format(i) for i in range(300)] + ['', 'naïve-日本語', 'y' * 5000]

    def caller(seed):
        def target(failures):
            rng = np.random.default_rng(seed)
            results = []
            with torch.cuda.stream(torch.cuda.Stream()):
                for size in sorted(rng.choice([63, 5000, 8193, 20000], size=3, replace=False)):
                    words = [pool[i] for i in rng.integers(0, len(pool), size=size)]
                    results.append((words, union.batch_embedding_device(words)))
            torch.cuda.synchronize()
            for words, got in results:
                pieces = [checker.batch_embedding(words) for checker in checkers]
                expected = np.concatenate(pieces, axis=-1) if mode == 'concatenate' else np.mean(pieces, axis=0)
                if not bits_equal(got.cpu().numpy(), expected):
                    failures.append('union ({}) of {} words differs from the checker'.format(mode, len(words)))
        return target

    failures = run_threads([caller(seed) for seed in range(4)])
    assert not failures, failures[:5]


def test_several_readers_of_one_file(native, model):
    """Two Readers of one file, every thread alternating between them call by call: nothing may be kept per file
    instead of per reader object."""
    readers = [native.Reader(model[0]), native.Reader(model[0])]
    targets = []
    for t in range(4):
        plan = [(KINDS[(t + k) % len(KINDS)], size) for k, size in enumerate([63, 5000, 8193, 20000])]
        targets.append(word_api_caller(readers[t % 2:] + readers[:t % 2], model, 300 + t, plan, use_default_stream=t == 0))
    failures = run_threads(targets)
    assert not failures, failures[:5]


def test_a_word_batch_in_use_is_refused_not_shared(native, model):
    """Every binding that fills or looks up through a WordBatch holds it for its whole call. While one call holds a batch
    (here: stopped inside the iteration over its words), every other call on that batch -- through this reader, another
    reader, a union, or the batch itself -- raises at once instead of sharing it. Afterwards the held call's answer is
    the checker's and the batch serves again."""
    import torch
    from memb_amd import _memb
    path = model[0]
    reader, other = native.Reader(path), native.Reader(path)
    reader.stage_words()
    other.stage_words()
    batch = _memb.WordBatch(0)
    entered, leave = threading.Event(), threading.Event()
    words, expected = draw(model, np.random.default_rng(11), 500)

    class Stalling:
        """a sequence of str that is not a list: the fill iterates over it, and waits there until told to go on"""
        def __len__(self):
            return len(words)

        def __getitem__(self, index):
            return words[index]

        def __iter__(self):
            entered.set()
            leave.wait(60)
            return iter(words)

    held = torch.full((len(words),), 7, dtype=torch.int32, device='cuda')
    spare = torch.full((4,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    outcome = []

    def holder():
        try:
            outcome.append(reader._impl.words_to_rows_device(batch, Stalling(), held.data_ptr(), 0))
        except BaseException:
            outcome.append(traceback.format_exc())

    thread = threading.Thread(target=holder)
    thread.start()
    try:
        assert entered.wait(60)
        offsets = np.array([0, 2], dtype=np.uint32)
        attempts = [
            lambda: reader._impl.words_to_rows_device(batch, ['ab'], spare.data_ptr(), 0),
            lambda: other._impl.words_to_rows_device(batch, ['ab'], spare.data_ptr(), 0),
            lambda: reader._impl.packed_to_rows_device(batch, b'ab', offsets, spare.data_ptr(), 0),
            lambda: reader._impl.resolve_batch_to_device(batch, spare.data_ptr(), 0),
            lambda: _memb.union_words_to_rows_device(batch, ['ab'], [reader._impl, other._impl],
                                                     [spare.data_ptr(), spare[2:].data_ptr()], 0),
            lambda: batch.pack(['ab']),
            lambda: _memb._word_fill_seconds(batch, ['ab']),
            lambda: _memb._packed_fill_seconds(batch, b'ab', offsets),
        ]
        for attempt in attempts:
            with pytest.raises(RuntimeError, match='word batch is in use by another call'):
                attempt()
    finally:
        leave.set()
        thread.join(120)
    assert outcome == [len(words)], outcome
    torch.cuda.synchronize()
    assert np.array_equal(held.cpu().numpy().view(np.uint32), expected)
    assert spare.cpu().numpy().tolist() == [7, 7, 7, 7]   # no refused call wrote anything
    assert batch.pack(['ab', 'cd']) == 2 and batch.size() == 2


def test_a_single_caller_keeps_one_batch(native, model):
    """One thread's calls reuse one word batch (whose next begin waits for the lookups still reading it); only calls in
    flight at the same time get batches of their own."""
    reader = native.Reader(model[0])
    words, expected = draw(model, np.random.default_rng(12), 5000)
    blob, offsets = packed(words)
    first = reader.resolve_rows_device(words)
    batch = reader._word_batch
    second = reader.resolve_packed_device(blob, offsets)
    third = reader.batch_embedding_device(words)
    assert batch is not None and reader._word_batch is batch
    for got in (first, second):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), expected)
    assert bits_equal(third.cpu().numpy(), model[1].rows_embedding(expected))
