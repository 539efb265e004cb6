"""reduction='chunked' on the GPU over the plan sizes, batch edges, column blocks and launch geometries that
tests/test_gpu_pooled_chunked.py does not reach (memb_hip_pooled_chunked.hip, pool_rows_chunked_checked in hip_pooled_launch.h):

  A  the plan: bag counts on every edge of a thread's 8 bags and of a block's 2048, and more than 256 blocks -- the second
     round of chunk_scan_sums;
  B  pool_chunks: bags of exactly j chunks on both sides of every edge of its batches of 8, in both branches, and whole
     chunks without a known entry at every place of a batch;
  C  column blocks: dims around 64 and 128, one to three columns, rows of thousands of values, 2-byte stores at odd and even
     columns;
  D  the partial sums under every geometry the sequential kernels are walked through;
  E  a caller-owned workspace of exactly the promised size, full of zeros, of 0xFF and of random bytes, and used twice;
  F  the whole call captured into a graph and replayed over other batches: the plan is made on the device.

The reference is R1 of tests/test_gpu_pooled_chunked.py, the contract's float32 loop over the reader's own rows (for very
many bags chunked_side_by_side, which tests/test_pooled_chunked_host.py shows to have R1's bits), and R2, the sequential
'sum' over the derived offsets followed by the in-order loop, where it is cheap. Bit for bit: the tolerance is zero. A
bf16 / fp16 result is R1 .to(dtype) on the CPU; counts are compared exactly; every `out` lies between sentinel columns."""
import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import check_chunked, for_every_key_form, narrow_bits, pooled, sweep_options, to_device
from pooled_reference import (COLUMN_DIMS, COLUMN_ROWS, COLUMN_STORAGES, EDGE_CHUNK_COUNTS, PLAN_BAG_COUNTS, PLAN_BAGS_PER_BLOCK,
                              PLAN_THREADS, UNKNOWN, UNKNOWN_CHUNKS, WIDE_MODELS, check_negative_zeros_survive,
                              chunked_by_the_contract, chunked_side_by_side, column_batch, contract_batch, derived_offsets,
                              edge_batch, from_partial_sums, offsets_of, plan_batch, reversed_batch, second_round_batch,
                              sequential_by_the_contract, signed_zero_model, signed_zero_rows, sub_batch, wide_batch,
                              with_unknown_chunks)

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
N_ROWS = 3000
BOTH = (False, True)   # missing='zero', missing='skip'


def contract_of(reader, rows, offsets, chunk, modes=('sum', 'mean'), skips=BOTH, by_the_contract=chunked_by_the_contract):
    """{(mode, skip): (vectors, counts)}: R1 over the reader's own fp32 rows"""
    rows = np.asarray(rows, dtype=np.uint32)
    values = reader.rows_embedding(rows) if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)
    return {(mode, skip): by_the_contract(values, rows, offsets, len(reader), mode, skip, chunk) for mode in modes for skip in skips}


def check_first(reader, rows, offsets, want, context, col_off=0, spare=0, dtype=None):
    """The call for every (mode, skip) of `want` against R1 -- R1 .to(dtype) for a narrow result -- with the counts.
    Returns {(mode, skip): the result on the host}."""
    import torch
    results = {}
    for (mode, skip), (vectors, counts) in want.items():
        got, got_counts = pooled(reader, rows, offsets, mode, skip, col_off, spare, dtype)
        reference = torch.from_numpy(vectors).to(dtype or torch.float32)
        if not np.array_equal(narrow_bits(got), narrow_bits(reference)):
            bad = np.nonzero((narrow_bits(got) != narrow_bits(reference)).any(axis=1))[0]
            raise AssertionError('{} {} skip={} {}: {} of {} bags differ, first {}'.format(
                context, mode, skip, dtype, len(bad), len(vectors), bad[:8]))
        assert not skip or np.array_equal(got_counts, counts), (context, mode, 'counts')
        results[(mode, skip)] = got
    return results


def check_second(reader, rows, offsets, chunk, results, want, context):
    """R2: the sequential 'sum' over the derived offsets, one bag per chunk, then the in-order loop over those sums."""
    derived, first = derived_offsets(offsets, len(rows), chunk)
    for skip in sorted({skip for _, skip in results}):
        partial, chunk_counts = pooled(reader, rows, derived, 'sum', skip, reduction='sequential')
        if not skip:
            chunk_counts = derived[1:] - derived[:-1]
        for (mode, skipped), got in results.items():
            if skipped == skip:
                again = from_partial_sums(partial.numpy(), chunk_counts, first, mode, want[(mode, skip)][1], reader.dim)
                assert bits_equal(got.numpy(), again), (context, mode, skip, 'R2')


# ---- A. the plan ----

@pytest.mark.parametrize('bags', PLAN_BAG_COUNTS)
def test_plan_sizes(native, make_model, bags):
    """1, 7 / 8 / 9 (a thread's bags), a block of the plan less one / exactly / and one more, two blocks likewise, and three
    blocks and k = 1..8: the last bag, which also stores bagStart[bags], in each of a thread's slots."""
    chunk = native.POOL_CHUNK
    path, _ = make_model(600, 6, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = plan_batch(chunk, bags, 600, bags)
    assert len(offsets) == bags + 1
    want = contract_of(reader, rows, offsets, chunk, by_the_contract=chunked_side_by_side)
    results = check_first(reader, rows, offsets, want, bags, col_off=1, spare=1)
    check_second(reader, rows, offsets, chunk, results, want, bags)


def test_more_plan_blocks_than_one_round_of_the_scan(native, make_model):
    """PLAN_THREADS blocks of the plan, one more and 3 bags: chunk_scan_sums goes round twice, with a carry. Every bag is
    compared; six long bags sit at the first and last bag and on both sides of the first block's and the first round's
    edge. Those and 1 000 of the short bags as a batch of their own have the same bits: no bag depends on its neighbours."""
    chunk = native.POOL_CHUNK
    path, _ = make_model(600, 8, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets, long = second_round_batch(chunk, 600, 3)
    bags = len(offsets) - 1
    assert bags == PLAN_THREADS * PLAN_BAGS_PER_BLOCK + PLAN_BAGS_PER_BLOCK + 3 and -(-bags // PLAN_BAGS_PER_BLOCK) == PLAN_THREADS + 2
    assert (offsets[long + 1] - offsets[long] == 5 * chunk + 3).all()
    want = contract_of(reader, rows, offsets, chunk, by_the_contract=chunked_side_by_side)
    results = check_first(reader, rows, offsets, want, 'second round')
    picked = np.sort(np.concatenate([long, np.random.default_rng(4).choice(np.setdiff1d(np.arange(bags), long), size=1000, replace=False)]))
    few_rows, few_offsets = sub_batch(rows, offsets, picked)
    few = check_first(reader, few_rows, few_offsets, contract_of(reader, few_rows, few_offsets, chunk), 'the picked bags alone')
    for key, got in few.items():
        assert bits_equal(got.numpy(), results[key].numpy()[picked]), key


# ---- B. the batches of pool_chunks ----

def test_bags_on_every_edge_of_a_batch_of_chunks(native, make_model):
    """Bags of exactly 1..20, 24, 25, 32 and 33 chunks: missing='zero' loads its batches of 8 from the second chunk on
    (edges at 9 / 10 / 17 / 18 / 25 / 33 chunks), 'skip' from the first (8 / 9 / 16 / 17 / 24 / 25 / 32 / 33)."""
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = edge_batch(chunk, N_ROWS, 23)
    assert offsets[0] == 3 and [-(-int(length) // chunk) for length in offsets[1:] - offsets[:-1]] == EDGE_CHUNK_COUNTS
    want = contract_of(reader, rows, offsets, chunk)
    values = reader.rows_embedding(rows)
    for skip in BOTH:   # on the host, before the GPU sees the batch: it can tell the two orders apart
        sequential, _ = sequential_by_the_contract(values, rows, offsets, N_ROWS, 'sum', skip)
        assert not bits_equal(want[('sum', skip)][0], sequential)
    results = check_first(reader, rows, offsets, want, 'edges')
    check_second(reader, rows, offsets, chunk, results, want, 'edges')
    for dtype in (torch.bfloat16, torch.float16):
        check_first(reader, rows, offsets, want, 'edges', col_off=1, spare=2, dtype=dtype)


def test_whole_chunks_without_a_known_entry(native, make_model, tmp_path):
    """missing='skip' over the bags of 1..33 chunks with whole chunks made unknown: the first known chunk at the start, in
    the middle and at the end of a batch of 8 and in the second batch; a hole in the middle; nothing known at all. Once
    more on a model of -0.0 and subnormals, where a +0.0 added for an unknown chunk shows as a lost -0.0."""
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    signed_path, _ = signed_zero_model(native, tmp_path)
    signed = native.Reader(signed_path)
    rows, offsets = edge_batch(chunk, N_ROWS, 23)
    for which in UNKNOWN_CHUNKS:
        holes = with_unknown_chunks(rows, offsets, chunk, which)
        want = contract_of(reader, holes, offsets, chunk, skips=(True,))
        results = check_first(reader, holes, offsets, want, which)
        check_second(reader, holes, offsets, chunk, results, want, which)
        check_first(reader, holes, offsets, {('mean', True): want[('mean', True)]}, which, col_off=1, dtype=torch.bfloat16)
        if which == 'all chunks':
            for got in results.values():
                assert not got.numpy().any() and not np.signbit(got.numpy()).any()   # +0.0, and the counts are R1's zeros
            assert not want[('sum', True)][1].any()
        holes = signed_zero_rows(holes)
        sums, counts = check_negative_zeros_survive(signed, holes, offsets, chunk)   # (the contract's, on the host)
        check_first(signed, holes, offsets, {('sum', True): (sums, counts)}, ('signed zeros', which))


# ---- C. columns ----

@pytest.mark.parametrize('dim', COLUMN_DIMS)
@pytest.mark.parametrize('storage,bits', COLUMN_STORAGES)
def test_column_blocks_and_strided_outputs(native, make_model, storage, bits, dim):
    """One wavefront of pool_chunks per 64 columns: one block of 1, 2, 3, 63 and 64 columns, two of 65, 127 and 128, three
    of 129, and 9 and 17 blocks; the stores of a bf16 / fp16 element at odd and even 2-byte columns."""
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(COLUMN_ROWS, dim, storage, bits, seed=dim)
    reader = native.Reader(path)
    rows, offsets = column_batch(chunk, COLUMN_ROWS, dim)
    want = contract_of(reader, rows, offsets, chunk)
    for col_off, spare in ((0, 0), (1, 2), (3, 1), (4, 4)):
        for dtype in (None, torch.bfloat16, torch.float16):
            results = check_first(reader, rows, offsets, want, (storage, dim, col_off, spare), col_off, spare, dtype)
            if dtype is None and col_off == 0:
                check_second(reader, rows, offsets, chunk, results, want, (storage, dim))


@pytest.mark.parametrize('storage,bits,dim,count', WIDE_MODELS)
def test_very_wide_rows(native, make_model, storage, bits, dim, count):
    """Rows beyond the row-record layout, up to one word per wavefront in stage (b) and 313 column blocks in pool_chunks."""
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(count, dim, storage, bits, seed=dim)
    reader = native.Reader(path)
    if storage == 'trained':
        assert reader.info()['row_layout'] != 2
    rows, offsets = wide_batch(chunk, count, dim)
    want = contract_of(reader, rows, offsets, chunk)
    results = check_first(reader, rows, offsets, want, (storage, dim))
    check_second(reader, rows, offsets, chunk, results, want, (storage, dim))
    check_first(reader, rows, offsets, want, (storage, dim, 'col_off'), col_off=1, spare=2)
    check_first(reader, rows, offsets, {('mean', True): want[('mean', True)]}, (storage, dim, 'bf16'), col_off=3, spare=1, dtype=torch.bfloat16)


# ---- D. the geometry of the partial sums ----

GEOMETRY_ROWS = 20000   # the models of test_key_forms_tables_and_row_layouts in tests/test_gpu_pooled_known.py


def test_key_forms_tables_and_row_layouts(native, make_model, monkeypatch):
    """Stage (b) under nibble keys, byte keys with a one-level table (MEMB_HIP_NO_FAST) and with two-level tables
    (max_direct_decode_bits=1); row records, compact streams with rowMeta records and with the two index arrays; 1 to 64
    lanes per word, blocks of 1 to 8 wavefronts. The 2-bit model once, at default geometry."""
    import torch
    chunk = native.POOL_CHUNK
    rows, offsets = contract_batch(chunk, GEOMETRY_ROWS, 11)
    want = {}

    def check(reader, context):
        check_chunked(reader, rows, offsets, chunk, context)
        if context[0] not in want:   # (the model's rows: one R1 per model)
            want[context[0]] = contract_of(reader, rows, offsets, chunk, modes=('mean',))
        check_first(reader, rows, offsets, want[context[0]], context + ('fp16',), col_off=1, dtype=torch.float16)

    for_every_key_form(native, make_model, monkeypatch, GEOMETRY_ROWS, check)   # (the forms of the sequential tests' three models)
    for_every_key_form(native, make_model, monkeypatch, GEOMETRY_ROWS, check, [(2, 'normal')], [({}, 0)], all_forms=False)


def test_results_do_not_depend_on_options(native, make_model):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = contract_batch(chunk, N_ROWS, 11)
    want = contract_of(reader, rows, offsets, chunk)
    sweep_options(reader, lambda waves, tiles: check_first(reader, rows, offsets, want, (waves, tiles)))


# ---- E. a caller-owned workspace, whatever it held before ----

GUARD = 256   # bytes (and counts) on each side of what the call owns


class RawCall:
    """reader._impl.pool_rows_chunked_to_device into a workspace of exactly pool_chunked_workspace_bytes(n, bags) bytes
    between two guard regions; `out` and `counts` between guards too."""

    def __init__(self, native, reader, n, bags):
        import torch
        self.native, self.reader, self.n, self.bags = native, reader, n, bags
        self.bytes = reader._impl.pool_chunked_workspace_bytes(n, bags)
        self.buffer = torch.full((GUARD + self.bytes + GUARD,), 0x5A, dtype=torch.uint8, device='cuda')
        assert (self.buffer.data_ptr() + GUARD) % 16 == 0
        self.workspace = self.buffer[GUARD:GUARD + self.bytes]

    def fill(self, how):
        import torch
        if how == 'random':
            noise = np.random.default_rng(self.bytes).integers(0, 256, size=self.bytes, dtype=np.uint8)
            self.workspace.copy_(torch.from_numpy(noise).cuda())
        else:
            self.workspace.fill_(how)

    def __call__(self, rows, offsets, mode, skip):
        """(vectors, counts or None) on the host; the guards are checked"""
        import torch
        native, dim, bags = self.native, self.reader.dim, self.bags
        assert len(rows) == self.n and len(offsets) == bags + 1
        device_rows, device_offsets = to_device(rows), to_device(offsets)
        out_buffer = torch.full((bags + 2, dim + 2), SENTINEL, dtype=torch.float32, device='cuda')
        count_buffer = torch.full((GUARD + bags + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        out = out_buffer[1:1 + bags]
        self.reader._impl.pool_rows_chunked_to_device(
            device_rows.data_ptr(), self.n, device_offsets.data_ptr(), bags, out.data_ptr(), out.stride(0), 1,
            native._memb.POOL_MEAN if mode == 'mean' else native._memb.POOL_SUM, torch.cuda.current_stream().cuda_stream,
            native._memb.OUT_F32, skip, count_buffer[GUARD:].data_ptr() if skip else 0, self.workspace.data_ptr(), self.bytes)
        torch.cuda.synchronize()
        edges = self.buffer.cpu().numpy()
        assert (edges[:GUARD] == 0x5A).all() and (edges[GUARD + self.bytes:] == 0x5A).all()
        host = out_buffer.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()
        assert (host[:, 0] == SENTINEL).all() and (host[:, -1] == SENTINEL).all()
        counted = count_buffer.cpu().numpy()
        assert (counted[:GUARD] == 0x5A5A5A5A).all() and (counted[GUARD + bags:] == 0x5A5A5A5A).all()
        assert skip or (counted == 0x5A5A5A5A).all()
        return host[1:1 + bags, 1:1 + dim], counted[GUARD:GUARD + bags].view(np.uint32) if skip else None


def workspace_batches(native, make_model, which):
    chunk = native.POOL_CHUNK
    if which == 'plan':
        path, _ = make_model(600, 6, 'trained', 4)
        rows, offsets = plan_batch(chunk, 2 * PLAN_BAGS_PER_BLOCK + 1, 600, 7)
        return native.Reader(path), rows, offsets, chunked_side_by_side
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    rows, offsets = edge_batch(chunk, N_ROWS, 23)
    if which != 'edges':
        rows = with_unknown_chunks(rows, offsets, chunk, which)
    return native.Reader(path), rows, offsets, chunked_by_the_contract


@pytest.mark.parametrize('which', ['plan', 'edges', 'chunks 0..8', 'all but chunk 8'])
def test_a_dirty_workspace_changes_nothing(native, make_model, which):
    """The workspace full of 0x00, of 0xFF -- NaNs where the partial sums go, 2^32 - 1 where the chunks' counts and the plan
    go -- and of seeded random bytes: the same bits, R1's, and nothing outside it is written. A stage that read a slot
    which no earlier stage of the same call wrote would differ in one of the three."""
    chunk = native.POOL_CHUNK
    reader, rows, offsets, by_the_contract = workspace_batches(native, make_model, which)
    want = contract_of(reader, rows, offsets, chunk, by_the_contract=by_the_contract)
    call = RawCall(native, reader, len(rows), len(offsets) - 1)
    for (mode, skip), (vectors, counts) in want.items():
        for how in (0x00, 0xFF, 'random'):
            call.fill(how)
            got, got_counts = call(rows, offsets, mode, skip)
            assert bits_equal(got, vectors), (which, mode, skip, how)
            assert not skip or np.array_equal(got_counts, counts), (which, mode, how)


@pytest.mark.parametrize('which', ['plan', 'edges'])
def test_nothing_survives_in_a_workspace_from_the_call_before(native, make_model, which):
    """Two batches of the same n and bags, one after the other into the same workspace: the second one's result is the
    second one's reference."""
    chunk = native.POOL_CHUNK
    reader, rows, offsets, by_the_contract = workspace_batches(native, make_model, which)
    other_rows, other_offsets = reversed_batch(rows, offsets)
    assert len(other_rows) == len(rows) and len(other_offsets) == len(offsets) and not np.array_equal(other_offsets, offsets)
    want = contract_of(reader, rows, offsets, chunk, modes=('mean',), by_the_contract=by_the_contract)
    other_want = contract_of(reader, other_rows, other_offsets, chunk, modes=('mean',), by_the_contract=by_the_contract)
    call = RawCall(native, reader, len(rows), len(offsets) - 1)
    call.fill(0xFF)
    for skip in BOTH:
        for batch_rows, batch_offsets, reference in ((other_rows, other_offsets, other_want), (rows, offsets, want),
                                                     (other_rows, other_offsets, other_want)):
            got, got_counts = call(batch_rows, batch_offsets, 'mean', skip)
            assert bits_equal(got, reference[('mean', skip)][0]), (which, skip)
            assert not skip or np.array_equal(got_counts, reference[('mean', skip)][1]), which


# ---- F. captured into a graph ----

def replay_batches(chunk, n_rows):
    """Three batches of one n and one number of bags whose chunk counts differ: bags of at most C entries; one bag that
    holds nearly everything; the bags of 1..33 chunks, padded with short bags."""
    rng = np.random.default_rng(31)
    edge_rows, edge_offsets = edge_batch(chunk, n_rows, 23)
    padding = [0, 1, 2, 3] * 4
    n, bags = len(edge_rows) + 50, len(edge_offsets) - 1 + len(padding)
    ids = lambda: np.where(rng.random(n) < 0.15, UNKNOWN, rng.integers(0, n_rows, size=n)).astype(np.uint32)   # noqa: E731
    short = offsets_of(rng.integers(0, chunk + 1, size=bags))
    one = np.zeros(bags, dtype=np.int64)
    one[[0, 5, 6, bags - 1]] = [1, n - 10, 2, 3]
    padded_rows = ids()
    padded_rows[:len(edge_rows)] = edge_rows
    padded = np.concatenate([edge_offsets, edge_offsets[-1] + np.cumsum(padding)])
    batches = [('short bags', ids(), short), ('one bag', ids(), offsets_of(one)), ('1..33 chunks', padded_rows, padded)]
    assert all(len(rows) == n and len(offsets) == bags + 1 and offsets[-1] <= n for _, rows, offsets in batches)
    return batches


def test_captured_into_a_graph(native, make_model):
    """The chunked call captured once and replayed over other CONTENTS of rows and offsets: each replay gives that batch's
    R1, so the plan is made on the device at replay and the host knew no chunk count when it enqueued the launches. The
    same for one sequential bf16 call."""
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    dim = reader.dim
    batches = replay_batches(chunk, N_ROWS)
    _, first_rows, first_offsets = batches[-1]
    rows, offsets = to_device(first_rows), to_device(first_offsets)
    bags = len(first_offsets) - 1
    out = torch.full((bags, dim + 2), SENTINEL, dtype=torch.float32, device='cuda')
    narrow = torch.full((bags, dim + 2), SENTINEL, dtype=torch.bfloat16, device='cuda')

    def enqueue():
        _, counts = reader.bags_embedding_device(rows, offsets, mode='mean', out=out, col_off=1, missing='skip', return_counts=True,
                                                 reduction='chunked')
        reader.bags_embedding_device(rows, offsets, mode='mean', out=narrow, col_off=1, dtype=torch.bfloat16)
        return counts

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        enqueue()   # (warm-up: stages the model, configures the kernels)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        counts = enqueue()
    for name, batch_rows, batch_offsets in batches:
        out.fill_(SENTINEL)
        narrow.fill_(SENTINEL)
        counts.fill_(-7)
        rows.copy_(to_device(batch_rows))
        offsets.copy_(to_device(batch_offsets))
        graph.replay()
        torch.cuda.synchronize()
        values = reader.rows_embedding(batch_rows)
        want, want_counts = chunked_by_the_contract(values, batch_rows, batch_offsets, N_ROWS, 'mean', True, chunk)
        host = out.cpu().numpy()
        assert (host[:, 0] == SENTINEL).all() and (host[:, -1] == SENTINEL).all(), name
        assert bits_equal(host[:, 1:1 + dim], want), name
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts), name
        sequential, _ = sequential_by_the_contract(values, batch_rows, batch_offsets, N_ROWS, 'mean', False)
        host = narrow.cpu()
        sentinel = torch.tensor(SENTINEL, dtype=torch.bfloat16)
        assert (host[:, 0] == sentinel).all() and (host[:, -1] == sentinel).all(), name
        assert np.array_equal(narrow_bits(host[:, 1:1 + dim]), narrow_bits(torch.from_numpy(sequential).to(torch.bfloat16))), name
