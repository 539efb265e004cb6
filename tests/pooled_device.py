"""What the GPU tests of the pooled lookups (tests/test_gpu_pooled*.py) share on the device side: arrays to the device and
bits back, the environment switches of a reader's kernels, the key-form and row-layout cases, two threads on two streams,
the sweep over the launch options and an `out` tensor inside a frame of sentinels. torch is imported where it is used, as
the tests do. The references themselves are tests/pooled_reference.py."""
import itertools
import threading

import numpy as np

from conftest import bits_equal
from pooled_reference import chunked_by_the_contract, derived_offsets, from_partial_sums, merged_rows

SENTINEL = -1234.5   # (the narrow tests pass -1536.0, which is exact in bf16 and fp16)


def to_device(array, kind=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).astype(np.uint32).view(kind)).cuda()


def narrow_bits(tensor):
    """the bits of a CPU tensor of any of the three types, as a numpy array"""
    import torch
    if tensor.dtype == torch.float32:
        return tensor.contiguous().numpy().view(np.uint32)
    return tensor.contiguous().view(torch.int16).numpy().view(np.uint16)


def same_bits(got, want):
    """got, want: tensors (float32, bf16, fp16, or the int32 of counts; on any device) or numpy arrays of 2- or 4-byte
    elements. The same shape and the same bits."""
    import torch

    def unsigned(value):
        if isinstance(value, torch.Tensor):
            value = value.cpu().contiguous()
            value = value.view(torch.int16 if value.element_size() == 2 else torch.int32).numpy()
        return np.ascontiguousarray(value).view(np.uint16 if value.itemsize == 2 else np.uint32)

    return np.array_equal(unsigned(got), unsigned(want))


# ---- the switches of a reader's kernels ----

ENVIRONMENT = ('MEMB_HIP_LANES', 'MEMB_HIP_WAVES', 'MEMB_HIP_ROOT_BITS', 'MEMB_HIP_NO_FAST', 'MEMB_HIP_ROW_RECORDS', 'MEMB_HIP_ROW_META')


def set_environment(monkeypatch, **values):
    for key in ENVIRONMENT:
        monkeypatch.delenv(key, raising=False)
    for key, value in values.items():
        monkeypatch.setenv(key, str(value))


def kernel_form(reader):
    """(HAS_SUB, FAST) of the reader's own decode kernel, decode_trained<HAS_SUB, MODE, FAST>"""
    name = reader.info(1)['kernel']
    has_sub, _, fast = [argument.strip() for argument in name[len('decode_trained<'):-1].split(',')]
    return has_sub == 'true', fast == 'true'


# (environment, max_direct_decode_bits): nibble keys, byte keys with a one-level table (MEMB_HIP_NO_FAST), two-level tables
# through max_direct_decode_bits=1; row records, compact streams with rowMeta records and with the two index arrays; lanes
# per word from 1 to 64 with spare lanes, blocks of 1 to 8 wavefronts
KEY_FORM_CASES = [({}, 0), ({}, 1), ({'MEMB_HIP_ROW_RECORDS': '0'}, 0), ({'MEMB_HIP_ROW_META': '0'}, 1), ({'MEMB_HIP_NO_FAST': 1}, 0),
                  ({'MEMB_HIP_LANES': 1, 'MEMB_HIP_WAVES': 1}, 0), ({'MEMB_HIP_LANES': 3, 'MEMB_HIP_WAVES': 2}, 0),
                  ({'MEMB_HIP_LANES': 5, 'MEMB_HIP_WAVES': 8}, 1), ({'MEMB_HIP_LANES': 25}, 0), ({'MEMB_HIP_LANES': 64}, 0)]
KEY_FORM_MODELS = [(4, 'normal'), (6, 'student'), (8, 'student')]   # (bits, distribution) of 300-column trained models
ALL_KEY_FORMS = {(False, True), (False, False), (True, False)}


def for_every_key_form(native, make_model, monkeypatch, n_rows, check, models=KEY_FORM_MODELS, cases=KEY_FORM_CASES,
                       all_forms=True):
    """check(reader, context) for a reader of every model under every case, context = (bits, environment,
    max_direct_decode_bits). all_forms: these models and cases must between them run all three key forms."""
    forms = set()
    for bits, distribution in models:
        path, _ = make_model(n_rows, 300, 'trained', bits, distribution=distribution)
        for environment, max_direct_bits in cases:
            set_environment(monkeypatch, **environment)
            reader = native.Reader(path, max_direct_decode_bits=max_direct_bits)
            if all_forms:
                forms.add(kernel_form(reader))
            check(reader, (bits, environment, max_direct_bits))
    assert not all_forms or forms == ALL_KEY_FORMS, forms


# ---- callers at once, launch options ----

def run_on_two_streams(jobs, call, repeats=20):
    """One thread per job, each on a stream of its own, all started together. call(thread, repeat) enqueues a lookup of
    jobs[thread] and returns (got, want, label): tensors and the arrays whose bits they must have once the stream is
    synchronized. A call that needs another comparison makes it itself and raises."""
    import torch
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(jobs))
    failures = []

    def run(thread):
        try:
            stream = torch.cuda.Stream()
            barrier.wait()
            with torch.cuda.stream(stream):
                for repeat in range(repeats):
                    got, want, label = call(thread, repeat)
                    stream.synchronize()
                    if not all(same_bits(one, other) for one, other in zip(got, want)):
                        failures.append((thread, repeat, label))
        except Exception as error:   # (a thread's exception is a failure of the test, not a line on stderr)
            failures.append((thread, repr(error)))

    threads = [threading.Thread(target=run, args=(thread,)) for thread in range(len(jobs))]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join()
    assert not failures, failures


WAVES_PER_BLOCK = (1, 2, 4, 7, 8)
TILES_PER_WAVE = (1, 2, 5, 64)


def sweep_options(reader, run, pairs=None):
    """run(waves, tiles) under every (waves_per_block, tiles_per_wave) of `pairs` -- WAVES_PER_BLOCK x TILES_PER_WAVE unless
    given --, and the reader back at its defaults whatever happens."""
    try:
        for waves, tiles in pairs or itertools.product(WAVES_PER_BLOCK, TILES_PER_WAVE):
            reader.set_option('waves_per_block', waves)
            reader.set_option('tiles_per_wave', tiles)
            run(waves, tiles)
    finally:
        reader.set_option('waves_per_block', 0)
        reader.set_option('tiles_per_wave', 0)


# ---- an `out` inside a frame of sentinels ----

def into_a_frame(run, bags, dim, context, col_off=0, spare=0, dtype=None, sentinel=SENTINEL, shifted=False):
    """run(out) pools into out[:, col_off:col_off + dim] of a (bags, col_off + dim + spare) tensor of `dtype` (float32 unless
    given) full of `sentinel` and returns the tensor the call returned: that must be `out`, and the columns around the
    block, like the one element of the buffer that lies outside `out`, must keep the sentinel. shifted: `out` starts one
    element into its buffer (a 2-byte type: 2-byte aligned only). Returns the block on the host."""
    import torch
    dtype = dtype or torch.float32
    width = col_off + dim + spare
    buffer = torch.full((bags * width + 1,), float(sentinel), dtype=dtype, device='cuda')
    out = buffer[1:].view(bags, width) if shifted else buffer[:bags * width].view(bags, width)
    assert out.data_ptr() % 4 == (out.element_size() % 4 if shifted else 0)
    returned = run(out)
    torch.cuda.synchronize()
    assert returned.data_ptr() == out.data_ptr() and returned.dtype == dtype, context
    host = out.cpu()
    guard = torch.tensor(float(sentinel), dtype=dtype)
    assert (host[:, :col_off] == guard).all() and (host[:, col_off + dim:] == guard).all(), context
    assert (buffer[:1] if shifted else buffer[-1:]).cpu()[0] == guard, context   # (outside the view)
    return host[:, col_off:col_off + dim]


# ---- reduction='chunked': the call and its two references ----

def pooled(reader, rows, offsets, mode, skip, col_off=0, spare=0, dtype=None, reduction='chunked'):
    """(vectors on the host, counts or None): bags_embedding_device(reduction=...) into a frame of sentinels, missing='skip'
    with its counts where `skip`"""
    import torch
    bags = len(offsets) - 1
    counted = []

    def run(out):
        result = reader.bags_embedding_device(
            to_device(rows), to_device(offsets), mode=mode, out=out, col_off=col_off, dtype=dtype, missing='skip' if skip else 'zero',
            return_counts=skip, reduction=reduction)
        returned, counts = result if skip else (result, None)
        counted.append(counts)
        return returned

    block = into_a_frame(run, bags, reader.dim, (mode, skip, reduction), col_off, spare, dtype)
    counts = counted[0]
    if skip:
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (bags,) and counts.is_cuda
        counts = counts.cpu().numpy().view(np.uint32)
    return block, counts


def check_chunked(reader, rows, offsets, chunk, context, modes=('sum', 'mean'), col_off=0, spare=0, second=True):
    """Both modes, missing='zero' and 'skip', against R1, the contract's loop over the reader's own rows, and (second) R2,
    the sequential sums of the chunks as bags put together in order."""
    n_rows, dim = len(reader), reader.dim
    rows = np.asarray(rows, dtype=np.uint32)
    values = reader.rows_embedding(rows) if len(rows) else np.zeros((0, dim), dtype=np.float32)
    derived, first = derived_offsets(offsets, len(rows), chunk)
    for skip in (False, True):
        if second:   # today's sums of the chunks as bags
            partial, chunk_counts = pooled(reader, rows, derived, 'sum', skip, reduction='sequential')
            partial = partial.numpy()
            if not skip:
                chunk_counts = derived[1:] - derived[:-1]
        for mode in modes:
            got, counts = pooled(reader, rows, offsets, mode, skip, col_off, spare)
            want, want_counts = chunked_by_the_contract(values, rows, offsets, n_rows, mode, skip, chunk)
            assert bits_equal(got.numpy(), want), (context, mode, skip, 'R1')
            if skip:
                assert np.array_equal(counts, want_counts), (context, mode, 'counts')
            if second:
                again = from_partial_sums(partial, chunk_counts, first, mode, want_counts, dim)
                assert bits_equal(got.numpy(), again), (context, mode, skip, 'R2')


# ---- a ReadersUnion's rows, from the readers on the device ----

def union_values(union_mode, readers, rows):
    n = len(rows[0])
    if not n:
        return np.zeros((0, sum(reader.dim for reader in readers) if union_mode == 'concatenate' else readers[0].dim), dtype=np.float32)
    return merged_rows(union_mode, [reader.rows_embedding_device(to_device(ids)).cpu().numpy() for reader, ids in zip(readers, rows)])
