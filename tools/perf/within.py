"""similarity_within_device against what a caller had before it on ONE Reader -- the cosine matrix slice after slice, the
predicate in torch comparisons, the list's columns masked out and torch.nonzero --, with A/A controls, the default call with
its count pass, and the three kernels alone as a rate. The method of tools/perf/ranks.py.

    python tools/perf/within.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--queries 1,16,64] [--found 100,100000]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    fill            similarity_within_device(queries, None, thresholds, marks, exclude=the word itself, offsets=precomputed,
                    capacity=their last entry, workspace=the recommended one, allocated once): the fill call alone
    fillb           the same again: the A/A spread below which no difference stands
    torch           the baseline, over slices as wide as the fused call's in temporaries allocated once:
                    similarity_matrix_device, cos >= t in torch, the list's column masked out, torch.nonzero (which
                    synchronises per slice) and the values gathered. Checked against the call before anything is timed:
                    equal positions and equal bits per row
    default         similarity_within_device with offsets=None: the count pass, the running sum, one synchronisation, the fill
Configurations on the 4-bit trained model of `words` words, every word a candidate: Q in {1, 16, 64} queries, the unit rows
of words, thresholds set per query so that a row finds about 100 and about 100 000 entries (the cosine of that rank, mark
INT64_MAX: words_within's question). Reports medians over rounds and whether the expectation holds: the fill no slower than
the baseline by more than the A/A spread plus 5 %. Then within_count, within_starts and within_write alone over a
(Q, words) matrix of random cosines that lists about a twentieth of it: 8 bytes read per element against STREAM_RATE.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import memb_amd
from memb_amd import _memb_within, synthetic

MARGIN = 0.05
STREAM_RATE = 6.3e12   # bytes per second: what a streaming kernel reaches on this part
INT64_MAX = np.iinfo(np.int64).max


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def measure(reader, own, found, rounds, reps):
    """own: int32 (Q,) rows of the model, the queries' words; found: the entries a row is to find, about"""
    count, n = own.shape[0], len(reader)
    queries = reader.unit_rows_embedding_device(own)
    everything = reader._all_rows_device(torch, 0)
    width = min(n, (32 << 20) // (4 * count) // 64 * 64)
    cosines = torch.empty((count, width), dtype=torch.float32, device='cuda')
    thresholds = torch.empty((count,), dtype=torch.float32, device='cuda')
    for q in range(count):   # (the cosine of rank `found`, one row of the matrix at a time)
        row = reader.similarity_matrix_device(queries[q:q + 1], everything)
        thresholds[q] = torch.topk(row[0], min(found, n)).values[-1]
    marks = torch.full((count,), INT64_MAX, dtype=torch.int64, device='cuda')
    lists = own.to(torch.int64).unsqueeze(1).contiguous()
    workspace = torch.empty((_memb_within.query_within_workspace_bytes(reader._impl.context_handle(), count, n),), dtype=torch.uint8, device='cuda')
    offsets = reader.similarity_within_device(queries, None, thresholds, marks, exclude=lists, workspace=workspace)[0]
    total = int(offsets[-1])
    listed = torch.empty((count, width), dtype=torch.bool, device='cuda')
    rows_of_lists = torch.arange(count, device='cuda').unsqueeze(1)
    kept = {}

    def fill():
        kept['fill'] = reader.similarity_within_device(queries, None, thresholds, marks, exclude=lists, offsets=offsets, capacity=total,
                                                       workspace=workspace)

    def default():
        kept['default'] = reader.similarity_within_device(queries, None, thresholds, marks, exclude=lists, workspace=workspace)

    def baseline():
        pieces = []
        for start in range(0, n, width):
            size = min(n, start + width) - start
            part = cosines[:, :size]
            reader.similarity_matrix_device(queries, everything[start:start + size], out=part)
            torch.ge(part, thresholds.unsqueeze(1), out=listed[:, :size])
            inside = (lists >= start) & (lists < start + size)
            listed[rows_of_lists[inside], (lists - start)[inside]] = False
            where = torch.nonzero(listed[:, :size])
            pieces.append((where[:, 0], where[:, 1] + start, part[where[:, 0], where[:, 1]]))
        kept['torch'] = pieces

    variants = {'fill': fill, 'fillb': fill, 'torch': baseline, 'default': default}
    for call in variants.values():
        call()
    kernel = reader.last_within_kernel
    torch.cuda.synchronize()
    # equal output: the baseline's pieces put row by row (a stable sort by row keeps the slices' ascending order)
    of_row = torch.cat([piece[0] for piece in kept['torch']])
    order = torch.sort(of_row, stable=True).indices
    assert torch.equal(torch.cat([piece[1] for piece in kept['torch']])[order], kept['fill'][1]), 'the fill and the baseline list differently'
    assert torch.equal(torch.cat([piece[2] for piece in kept['torch']])[order].view(torch.int32), kept['fill'][2].view(torch.int32))
    assert torch.equal(torch.bincount(of_row, minlength=count), kept['fill'][3]) and torch.equal(kept['default'][1], kept['fill'][1])
    kept.clear()
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    ms = result['fill']['median_ms']
    spread = abs(result['fillb']['median_ms'] - ms) / ms
    result['summary'] = {
        'candidates': n, 'queries': count, 'found_per_row': total / count, 'kernel': kernel, 'slice': width,
        'fill_ms': ms, 'aa_spread': spread, 'torch_ms': result['torch']['median_ms'], 'fill_over_torch': ms / result['torch']['median_ms'],
        'default_ms': result['default']['median_ms'], 'holds': ms <= result['torch']['median_ms'] * (1 + spread + MARGIN),
    }
    return result


def measure_kernels(count, n, rounds, reps):
    """within_count, within_starts and within_write alone over a (count, n) matrix of random cosines, cos > 0.9 listed"""
    matrix = torch.rand((count, n), dtype=torch.float32, device='cuda') * 2 - 1
    thresholds = torch.full((count,), 0.9, dtype=torch.float32, device='cuda')
    marks = torch.full((count,), -1, dtype=torch.int64, device='cuda')
    sizes = (matrix > 0.9).sum(dim=1)
    offsets = torch.zeros((count + 1,), dtype=torch.int64, device='cuda')
    torch.cumsum(sizes, 0, out=offsets[1:])
    total = int(offsets[-1])
    positions = torch.empty((total,), dtype=torch.int64, device='cuda')
    values = torch.empty((total,), dtype=torch.float32, device='cuda')
    cursors = torch.empty((count,), dtype=torch.int64, device='cuda')
    workspace = torch.empty((_memb_within.dense_within_workspace_bytes(count, n),), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _memb_within.dense_within_to_device(
            0, matrix.data_ptr(), count, n, n, 0, thresholds.data_ptr(), marks.data_ptr(), 0, 0, 0, False, offsets.data_ptr(),
            cursors.data_ptr(), positions.data_ptr(), values.data_ptr(), total, workspace.data_ptr(), workspace.numel(), stream)

    series = [timed(call, reps) for _ in range(rounds)]
    torch.cuda.synchronize()
    assert torch.equal(cursors, sizes) and torch.equal(positions, torch.nonzero(matrix > 0.9)[:, 1])
    ms = float(np.median(series))
    moved = 8 * count * n + 12 * total   # (the matrix twice, a position and a value per entry)
    return {'queries': count, 'columns': n, 'listed': total, 'bytes': moved, 'median_ms': ms, 'ms': series,
            'bytes_per_second': moved / (ms * 1e-3), 'share_of_stream_rate': moved / (ms * 1e-3) / STREAM_RATE}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--queries', default='1,16,64')
    parser.add_argument('--found', default='100,100000')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('within.py measures on a GPU; none found')
    results = {}

    def save():
        if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
            with open(args.out, 'w') as f:
                json.dump(results, f, indent=1)

    for count in (int(value) for value in args.queries.split(',')):
        name = 'kernels_{}x{}'.format(count, args.words)
        results[name] = measure_kernels(count, args.words, args.rounds, args.reps)
        print('{:28s} {:.4f} ms  {:.2f} TB/s  {:.1%} of the streaming rate'.format(
            name, results[name]['median_ms'], results[name]['bytes_per_second'] / 1e12, results[name]['share_of_stream_rate']), flush=True)
        save()
    generator = torch.Generator(device='cuda').manual_seed(1)
    path, _ = synthetic.cached_model(args.words, 300, 'trained', 4)
    reader = memb_amd.Reader(path)
    for count in (int(value) for value in args.queries.split(',')):
        own = torch.randint(0, args.words, (count,), device='cuda', generator=generator, dtype=torch.int32)
        for found in (int(value) for value in args.found.split(',')):
            name = '4bit_{}xall_find{}'.format(count, found)
            results[name] = measure(reader, own, found, args.rounds, args.reps)
            summary = results[name]['summary']
            print('{:24s} fill {:.4f} ms  A/A {:.1%} | matrix, torch and nonzero {:.4f} ms  x{:.3f} of it ({}) | default {:.4f} ms | {:.0f} found per row | {}'.format(
                name, summary['fill_ms'], summary['aa_spread'], summary['torch_ms'], summary['fill_over_torch'],
                'holds' if summary['holds'] else 'DOES NOT HOLD', summary['default_ms'], summary['found_per_row'], summary['kernel']), flush=True)
            save()


if __name__ == '__main__':
    main()
