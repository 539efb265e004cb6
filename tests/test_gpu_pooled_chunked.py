"""Pooled lookups under the chunked order on the GPU (memb_hip_pooled_chunked.hip; include/memb_hip_pooled_chunked.h):
bags_embedding_device / sentences_embedding_device / bags_embedding with reduction='chunked'.

Two references, both compared bit for bit (the tolerance is zero):
  R1  the contract's explicit float32 loop over reader.rows_embedding(rows) (tests/pooled_reference.py);
  R2  the SEQUENTIAL call (reduction left out) with mode='sum' over the derived offsets, one bag per chunk, then the
      in-order numpy loop over those partial sums.
A bf16 / fp16 result is R1 .to(dtype) on the CPU. Lengths around a chunk are named by C = memb_amd.POOL_CHUNK."""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal
from pooled_device import check_chunked, narrow_bits, pooled, run_on_two_streams, to_device
from pooled_reference import (LONGEST, UNKNOWN, check_skip_cases, chunked_by_the_contract, contract_batch, inner_batches, offsets_of,
                              sequential_by_the_contract, signed_zero_model, skip_cases)

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
N_ROWS = 3000
SEED = 11   # of contract_batch: tests/test_pooled_chunked_host.py shows on the host that the two orders differ for it


# ---- 1. the contract, both references ----

@pytest.mark.parametrize('dim,storage,bits', [(300, 'trained', 4), (300, 'trained', 6), (300, 'uniform', 8), (300, 'full', 32),
                                              (77, 'trained', 4)])
def test_the_contract_by_both_references(native, make_model, dim, storage, bits):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, dim, storage, bits)
    reader = native.Reader(path)
    rows, offsets = contract_batch(chunk, N_ROWS, SEED)
    check_chunked(reader, rows, offsets, chunk, (dim, storage, bits), col_off=1, spare=1)
    check_chunked(reader, rows, offsets, chunk, (dim, storage, bits, 'aligned'), modes=('mean',), second=False)


# ---- 2. the new order is really used ----

def test_the_result_has_the_chunked_bits_not_the_sequential_ones(native, make_model):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = contract_batch(chunk, N_ROWS, SEED)
    values = native.Reader(path, device='cpu').rows_embedding(rows)
    for skip in (False, True):
        chunked, _ = chunked_by_the_contract(values, rows, offsets, N_ROWS, 'sum', skip, chunk)
        sequential, _ = sequential_by_the_contract(values, rows, offsets, N_ROWS, 'sum', skip)
        differing = chunked[LONGEST].view(np.uint32) != sequential[LONGEST].view(np.uint32)
        assert differing.any()   # (on the host, before the GPU sees the batch: else pick another SEED)
        got, _ = pooled(reader, rows, offsets, 'sum', skip)
        assert bits_equal(got.numpy()[LONGEST][differing], chunked[LONGEST][differing])
        assert bits_equal(got.numpy(), chunked)
        old, _ = pooled(reader, rows, offsets, 'sum', skip, reduction='sequential')
        assert bits_equal(old.numpy(), sequential)   # the default order stays what it was


# ---- 3. bags of at most C entries: the sequential bits ----

@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_bags_of_at_most_one_chunk_have_the_sequential_bits(native, make_model, storage, bits):
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader = native.Reader(path)
    rng = np.random.default_rng(5)
    lengths = np.concatenate([[0, chunk, 1, chunk], rng.integers(0, chunk + 1, size=2500)])   # more than one block of the plan
    rows = rng.integers(0, N_ROWS, size=int(lengths.sum())).astype(np.uint32)
    rows[::5] = UNKNOWN
    offsets = offsets_of(lengths)
    for mode in ('sum', 'mean'):
        for dtype, skip in ((None, False), (torch.bfloat16, False), (None, True), (torch.bfloat16, True)):
            chunked, chunked_counts = pooled(reader, rows, offsets, mode, skip, dtype=dtype)
            sequential, counts = pooled(reader, rows, offsets, mode, skip, dtype=dtype, reduction='sequential')
            assert np.array_equal(narrow_bits(chunked), narrow_bits(sequential)), (mode, dtype, skip)
            assert not skip or np.array_equal(chunked_counts, counts)


# ---- 4. skipped chunks add nothing, not even +0.0 ----

def test_skipped_chunks_add_nothing(native, tmp_path):
    chunk = native.POOL_CHUNK
    path, count = signed_zero_model(native, tmp_path)
    reader = native.Reader(path)
    rows, offsets = skip_cases(chunk, count)
    values = reader.rows_embedding(rows)
    result, counts = pooled(reader, rows, offsets, 'sum', True)
    check_skip_cases(result.numpy(), counts, values, rows, offsets, count, chunk)
    mean, mean_counts = pooled(reader, rows, offsets, 'mean', True)
    want, want_counts = chunked_by_the_contract(values, rows, offsets, count, 'mean', True, chunk)
    assert bits_equal(mean.numpy(), want) and np.array_equal(mean_counts, want_counts)
    zero, _ = pooled(reader, rows, offsets, 'sum', False)
    assert not zero.numpy()[0][:30].any() and not np.signbit(zero.numpy()[0][:30]).any()   # unknown entries that count: +0.0


# ---- 5. bf16 / fp16: the fp32 result rounded once ----

@pytest.mark.parametrize('dim', [300, 77])
def test_narrow_results_are_the_fp32_result_rounded_once(native, make_model, tmp_path, dim):
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, dim, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = contract_batch(chunk, N_ROWS, SEED)
    for mode in ('sum', 'mean'):
        for skip in (False, True):
            fp32, fp32_counts = pooled(reader, rows, offsets, mode, skip)
            for dtype in (torch.bfloat16, torch.float16):
                got, counts = pooled(reader, rows, offsets, mode, skip, col_off=1, spare=2, dtype=dtype)
                assert np.array_equal(narrow_bits(got), narrow_bits(fp32.to(dtype))), (mode, skip, dtype)
                assert not skip or np.array_equal(counts, fp32_counts)
    # [1, 2^-8 | 2^-8] over two chunks: 1 + 2^-8 is a tie that rounds to 1 in bf16, so a partial sum narrowed on its way
    # through the workspace would end at 1, not at 1 + 2^-7
    values = np.array([1.0, 2.0 ** -8, 0.0], dtype=np.float32)
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['w{}'.format(i) for i in range(len(values))], np.repeat(values[:, None], dim, axis=1))
    tie_path = str(tmp_path / 'tie_{}.bin'.format(dim))
    builder.save(tie_path)
    tie = native.Reader(tie_path)
    one, tiny, nothing = (int(tie.resolve_rows(['w{}'.format(i)])[0]) for i in range(3))
    bag = np.full(chunk + 1, nothing, dtype=np.uint32)
    bag[0], bag[chunk - 1], bag[chunk] = one, tiny, tiny
    for skip in (False, True):
        got, _ = pooled(tie, bag, offsets_of([chunk + 1]), 'sum', skip, dtype=torch.bfloat16)
        assert (got.to(torch.float32) == 1.0 + 2.0 ** -7).all()


# ---- 6. launch geometry never changes a result ----

def test_results_do_not_depend_on_geometry(native, make_model, monkeypatch):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    rows, offsets = contract_batch(chunk, N_ROWS, SEED)
    values = native.Reader(path, device='cpu').rows_embedding(rows)
    want = {(mode, skip): chunked_by_the_contract(values, rows, offsets, N_ROWS, mode, skip, chunk)
            for mode in ('sum', 'mean') for skip in (False, True)}

    def check(reader, context):
        for (mode, skip), (vectors, counts) in want.items():
            got, got_counts = pooled(reader, rows, offsets, mode, skip)
            assert bits_equal(got.numpy(), vectors), (context, mode, skip)
            assert not skip or np.array_equal(got_counts, counts), (context, mode)

    reader = native.Reader(path)
    try:
        for tiles in (1, 4):
            reader.set_option('tiles_per_wave', tiles)
            check(reader, ('tiles_per_wave', tiles))
    finally:
        reader.set_option('tiles_per_wave', 0)
    monkeypatch.setenv('MEMB_HIP_NO_FAST', '1')
    check(native.Reader(path), 'MEMB_HIP_NO_FAST')


# ---- 7. two threads, two streams, two workspaces ----

def test_two_threads_on_two_streams(native, make_model):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    jobs = []
    for thread in range(2):
        rows, offsets = contract_batch(chunk, N_ROWS, 20 + thread)
        if thread:
            offsets = offsets[2:]   # another batch: other bags, other chunk counts
        values = reader.rows_embedding(rows)
        jobs.append((to_device(rows), to_device(offsets),
                     {mode: chunked_by_the_contract(values, rows, offsets, N_ROWS, mode, True, chunk) for mode in ('sum', 'mean')}))

    def call(thread, repeat):
        mode = ('sum', 'mean')[repeat % 2]
        got = reader.bags_embedding_device(jobs[thread][0], jobs[thread][1], mode=mode, missing='skip', return_counts=True,
                                           reduction='chunked')
        return got, jobs[thread][2][mode], mode

    run_on_two_streams(jobs, call, repeats=10)


# ---- 8. one long bag; empty batches; offsets beyond n ----

def test_one_long_bag(native, make_model):
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows = np.random.default_rng(8).integers(0, N_ROWS, size=20000).astype(np.uint32)
    rows[::11] = UNKNOWN
    check_chunked(reader, rows, np.array([0, 20000]), chunk, 'one long bag', modes=('mean',), second=False)


def test_empty_batches_and_offsets_beyond_n(native, make_model):
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    no_rows = np.zeros(0, dtype=np.uint32)
    for skip in (False, True):   # n == 0: every bag is +0.0 and counts nothing
        got, counts = pooled(reader, no_rows, np.array([0, 0, 0, 7]), 'mean', skip, col_off=1)
        assert tuple(got.shape) == (3, 300) and not got.numpy().any() and not np.signbit(got.numpy()).any()
        assert not skip or not counts.any()
    empty = reader.bags_embedding_device(to_device(np.arange(5)), to_device([0]), reduction='chunked')   # bags == 0
    assert tuple(empty.shape) == (0, 300)
    rows = np.random.default_rng(9).integers(0, N_ROWS, size=3 * chunk + 10).astype(np.uint32)
    rows[::7] = UNKNOWN
    n = len(rows)
    offsets = np.array([0, chunk + 1, n - 1, n + 5, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.int64)   # clamped to n
    check_chunked(reader, rows, offsets, chunk, 'beyond n', second=False)
    got, counts = pooled(reader, rows, offsets, 'sum', True)
    assert counts[2] == int(rows[n - 1] < N_ROWS) and counts[3] == 0 and counts[4] == 0 and not got.numpy()[3:].any()


@pytest.mark.parametrize('storage,bits', [('trained', 4), ('uniform', 8)])
def test_entries_outside_the_bags_belong_to_no_bag(native, make_model, storage, bits):
    """The first offset lies behind entry 0 and the last one well before n: the last bag's last chunk ends where the bag
    ends, not where the batch does. Against R1 and R2, the sequential call for bags of at most one chunk, and the
    device='cpu' reader."""
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, storage, bits)
    reader, host = native.Reader(path), native.Reader(path, device='cpu')
    for name, rows, offsets in inner_batches(chunk, N_ROWS, 13):
        assert offsets[-1] < len(rows)
        check_chunked(reader, rows, offsets, chunk, (storage, name), col_off=1, spare=1)
        short = np.nonzero(offsets[1:] - offsets[:-1] <= chunk)[0]
        for mode in ('sum', 'mean'):
            for skip in (False, True):
                got, counts = pooled(reader, rows, offsets, mode, skip)
                sequential, sequential_counts = pooled(reader, rows, offsets, mode, skip, reduction='sequential')
                assert bits_equal(got.numpy()[short], sequential.numpy()[short]), (name, mode, skip)
                missing = 'skip' if skip else 'zero'
                through = reader.bags_embedding(rows, offsets, mode=mode, missing=missing, return_counts=skip, reduction='chunked')
                on_host = host.bags_embedding(rows, offsets, mode=mode, missing=missing, return_counts=skip, reduction='chunked')
                if skip:
                    assert np.array_equal(counts, sequential_counts) and np.array_equal(through[1], on_host[1]), (name, mode)
                    assert np.array_equal(counts, on_host[1]), (name, mode)
                    through, on_host = through[0], on_host[0]
                assert bits_equal(through, on_host) and bits_equal(got.numpy(), on_host), (name, mode, skip)


# ---- 9. offsets that decrease: the call ends and writes nothing it does not own ----

def test_decreasing_offsets_harm_nothing(native, make_model):
    import torch
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    dim, n, bags, guard = reader.dim, 50, 3, 64
    rows = np.random.default_rng(10).integers(0, N_ROWS, size=n).astype(np.uint32)
    rows[::7] = UNKNOWN
    values = reader.rows_embedding(rows)
    # the caller's buffers, each between two canaries
    row_buffer = torch.full((guard + n + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    row_buffer[guard:guard + n] = to_device(rows)
    before = row_buffer.clone()
    device_offsets = to_device([0, 40, 10, 50])
    for skip in (False, True):
        out_buffer = torch.full((bags + 2, dim + 2), SENTINEL, dtype=torch.float32, device='cuda')
        count_buffer = torch.full((guard + bags + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        workspace_bytes = reader._impl.pool_chunked_workspace_bytes(n, bags)
        workspace = torch.full((guard + workspace_bytes + guard,), 0x5A, dtype=torch.uint8, device='cuda')
        assert (workspace.data_ptr() + guard) % 16 == 0
        out = out_buffer[1:1 + bags]
        reader._impl.pool_rows_chunked_to_device(
            row_buffer[guard:].data_ptr(), n, device_offsets.data_ptr(), bags, out.data_ptr(), out.stride(0), 1, native._memb.POOL_SUM,
            torch.cuda.current_stream().cuda_stream, native._memb.OUT_F32, skip,
            count_buffer[guard:].data_ptr() if skip else 0, workspace[guard:].data_ptr(), workspace_bytes)
        torch.cuda.synchronize()   # the call returned, and its kernels end
        assert torch.equal(row_buffer, before)
        host = out_buffer.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()
        assert (host[:, 0] == SENTINEL).all() and (host[:, -1] == SENTINEL).all()
        if skip:
            counted = count_buffer.cpu().numpy()
            assert (counted[:guard] == 0x5A5A5A5A).all() and (counted[guard + bags:] == 0x5A5A5A5A).all()
        edges = workspace.cpu().numpy()
        assert (edges[:guard] == 0x5A).all() and (edges[guard + workspace_bytes:] == 0x5A).all()
        # bag 0 lies before the decrease: its value is the contract's (bags 1 and 2 are not asserted)
        want, _ = chunked_by_the_contract(values, rows, np.array([0, 40]), N_ROWS, 'sum', skip, native.POOL_CHUNK)
        assert bits_equal(host[1, 1:1 + dim], want[0])


# ---- 10. the Python surface and the C ABI's refusals ----

def test_python_entry_points_and_their_errors(native, make_model):
    import torch
    chunk = native.POOL_CHUNK
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    rows, offsets = contract_batch(chunk, N_ROWS, SEED)
    device_rows, device_offsets = to_device(rows), to_device(offsets)
    for call in (lambda: reader.bags_embedding_device(device_rows, device_offsets, reduction='tree'),
                 lambda: reader.sentences_embedding_device([['a']], reduction='tree'),
                 lambda: reader.bags_embedding(rows, offsets, reduction='tree')):
        with pytest.raises(ValueError, match='reduction'):
            call()
    with pytest.raises(ValueError, match='return_counts'):
        reader.bags_embedding_device(device_rows, device_offsets, return_counts=True, reduction='chunked')
    vocabulary = sorted(words)
    sentences = [vocabulary[:5], [], ['not-in-the-model'], ['nor-this'] + vocabulary[100:100 + 3 * chunk + 2] + ['nor-this'],
                 [vocabulary[7]] * (chunk + 1)]
    flat = [word for sentence in sentences for word in sentence]
    resolved = reader.resolve_rows(flat)
    sentence_offsets = offsets_of([len(sentence) for sentence in sentences])
    for mode in ('sum', 'mean'):
        got = reader.sentences_embedding_device(sentences, mode=mode, reduction='chunked')
        want = reader.bags_embedding_device(to_device(resolved), to_device(sentence_offsets), mode=mode, reduction='chunked')
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        got, counts = reader.sentences_embedding_device(sentences, mode=mode, missing='skip', return_counts=True, reduction='chunked')
        want, want_counts = reader.bags_embedding_device(
            to_device(resolved), to_device(sentence_offsets), mode=mode, missing='skip', return_counts=True, reduction='chunked')
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(counts, want_counts)
        assert counts.cpu().tolist() == [5, 0, 0, 3 * chunk + 2, chunk + 1]
    host = native.Reader(path, device='cpu')
    for mode in ('sum', 'mean'):
        assert bits_equal(reader.bags_embedding(rows, offsets, mode=mode, reduction='chunked'),
                          host.bags_embedding(rows, offsets, mode=mode, reduction='chunked'))
        got = reader.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked')
        want = host.bags_embedding(rows, offsets, mode=mode, missing='skip', return_counts=True, reduction='chunked')
        assert bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == np.uint32
    union = native.ReadersUnion([reader, native.Reader(path)], 'average')
    with pytest.raises(NotImplementedError):
        union.bags_embedding_device(device_rows, device_offsets, reduction='chunked')


def test_the_c_abi_sizes_the_workspace_and_refuses_bad_calls(native, make_model):
    import torch
    chunk = native.POOL_CHUNK
    path, _ = make_model(N_ROWS, 300, 'trained', 4)
    reader = native.Reader(path)
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    sizes = library.memb_hip_pool_chunked_workspace_bytes
    sizes.restype = ctypes.c_size_t
    sizes.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]
    assert sizes(None, 1000, 10) == 0
    n, bags = 1000, 10
    needed = reader._impl.pool_chunked_workspace_bytes(n, bags)

    def layout(entries, count, dim=300):
        """the sections of include/memb_hip_pooled_chunked.h's workspace, each rounded up to 16 bytes"""
        slots = count + -(-entries // chunk)
        sections = (4 * (count + 1), 8 * -(-count // 2048), 4 * (slots + 1), 4 * slots, 4 * slots * dim)
        return sum(-(-section // 16) * 16 for section in sections)

    context = ctypes.c_void_p(reader._impl.context_handle())
    for entries, count in ((n, bags), (0, 1), (1, 1), (5, 3), (100000, 1), (2049 * 3, 2049), (123457, 4097)):
        assert sizes(context, entries, count) == layout(entries, count), (entries, count)
        assert reader._impl.pool_chunked_workspace_bytes(entries, count) == layout(entries, count)
    rows = to_device(np.arange(n) % N_ROWS)
    offsets = to_device(np.arange(bags + 1) * (n // bags))
    out = torch.full((bags, 300), SENTINEL, device='cuda')
    counts = torch.zeros((bags,), dtype=torch.int32, device='cuda')
    workspace = torch.zeros((needed,), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call(skip=False, counts_ptr=0, workspace_ptr=workspace.data_ptr(), workspace_bytes=needed, ld=300, mode=native._memb.POOL_MEAN,
             out_type=native._memb.OUT_F32):
        reader._impl.pool_rows_chunked_to_device(
            rows.data_ptr(), n, offsets.data_ptr(), bags, out.data_ptr(), ld, 0, mode, stream, out_type, skip, counts_ptr,
            workspace_ptr, workspace_bytes)

    for refused, reason in ((dict(workspace_ptr=0), 'workspace'), (dict(workspace_bytes=needed - 1), 'workspace'),
                            (dict(workspace_ptr=workspace.data_ptr() + 4, workspace_bytes=needed - 4), 'workspace'),
                            (dict(counts_ptr=counts.data_ptr()), 'counts'), (dict(ld=299), 'ld must be at least'),
                            (dict(mode=7), 'unknown pooling mode'), (dict(out_type=9), 'unknown out_type')):
        with pytest.raises(RuntimeError, match=reason):
            call(**refused)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()   # a refused call launches nothing
    call(skip=True, counts_ptr=counts.data_ptr())
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [n // bags] * bags
    want = reader.bags_embedding_device(rows, offsets, missing='skip', reduction='chunked')
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
