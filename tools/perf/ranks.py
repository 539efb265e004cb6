"""similarity_ranks_device against what a caller had before it on ONE Reader -- the cosine matrix slice after slice, the
predicate and a sum in torch operations --, with A/A controls, and rank_count alone as a share of the HBM peak. The method
of tools/perf/cosmul.py.

    python tools/perf/ranks.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--queries 1,16,64]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    fused           similarity_ranks_device(queries, None, thresholds, marks, exclude=lists or None, workspace=the recommended
                    one, allocated once)
    fusedb          the same again: the A/A spread below which no difference stands
    torch           the baseline, over slices as wide as the fused call's in temporaries allocated once:
                    similarity_matrix_device, then (cos > t) | ((cos == t) & (position < mark)) in torch, the columns of the
                    list masked out, and a sum. Checked against the call before anything is timed: equal counts (the
                    cosines of a trained model hold no NaN and the thresholds are no zeros, so the float comparison is the
                    contract's)
Configurations on the 4-bit trained model of `words` words, every word a candidate: Q in {1, 16, 64} queries, the unit rows
of words, the mark of each the row of another word with its cosine as the threshold (rank_device's question), with and
without a 3-entry list of non-candidates. Reports medians over rounds and whether the expectation holds: no slower than the
baseline by more than the A/A spread plus 5 %. Then rank_count and rank_fold alone over a (Q, words) matrix: 4 bytes per
element against HBM_PEAK.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import memb_amd
from memb_amd import _memb_ranks, synthetic

EXCLUDED = 3
MARGIN = 0.05
HBM_PEAK = 8.0e12   # bytes per second, the MI355X's specification


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def measure(reader, word_rows, with_list, rounds, reps):
    """word_rows: int32 (Q, 2 + EXCLUDED) rows of the model -- the query's word, the marked word, the list"""
    count, n = word_rows.shape[0], len(reader)
    queries = reader.unit_rows_embedding_device(word_rows[:, 0].contiguous())
    marked = word_rows[:, 1].contiguous()
    thresholds = reader.query_similarity_device(queries, marked, torch.arange(count + 1, dtype=torch.int32, device='cuda'))
    marks = marked.to(torch.int64)
    lists = word_rows[:, 2:].to(torch.int64).contiguous() if with_list else None
    everything = reader._all_rows_device(torch, 0)
    needed = _memb_ranks.query_ranks_workspace_bytes(reader._impl.context_handle(), count, n)
    workspace = torch.empty((needed,), dtype=torch.uint8, device='cuda')
    width = min(n, (32 << 20) // (4 * count) // 64 * 64)
    cosines = torch.empty((count, width), dtype=torch.float32, device='cuda')
    precedes = torch.empty((count, width), dtype=torch.bool, device='cuda')
    equal = torch.empty((count, width), dtype=torch.bool, device='cuda')
    positions = torch.arange(n, dtype=torch.int64, device='cuda')
    rows_of_lists = torch.arange(count, device='cuda').unsqueeze(1).expand(count, EXCLUDED)
    kept = {}

    def fused():
        kept['fused'] = reader.similarity_ranks_device(queries, None, thresholds, marks, exclude=lists, workspace=workspace)

    def baseline():
        counts = torch.zeros((count,), dtype=torch.int64, device='cuda')
        for start in range(0, n, width):
            size = min(n, start + width) - start
            part = cosines[:, :size]
            reader.similarity_matrix_device(queries, everything[start:start + size], out=part)
            torch.gt(part, thresholds.unsqueeze(1), out=precedes[:, :size])
            torch.eq(part, thresholds.unsqueeze(1), out=equal[:, :size])
            equal[:, :size] &= positions[start:start + size].unsqueeze(0) < marks.unsqueeze(1)
            precedes[:, :size] |= equal[:, :size]
            if lists is not None:
                inside = (lists >= start) & (lists < start + size)
                precedes[rows_of_lists[inside], (lists - start)[inside]] = False
            counts += precedes[:, :size].sum(dim=1)
        kept['torch'] = counts

    variants = {'fused': fused, 'fusedb': fused, 'torch': baseline}
    for call in variants.values():
        call()
    kernel = reader.last_ranks_kernel
    torch.cuda.synchronize()
    assert torch.equal(kept['fused'], kept['torch']), 'the fused call and the baseline count differently'
    kept.clear()
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    ms = result['fused']['median_ms']
    spread = abs(result['fusedb']['median_ms'] - ms) / ms
    result['summary'] = {
        'candidates': n, 'queries': count, 'excluded': EXCLUDED if with_list else 0, 'kernel': kernel, 'slice': width,
        'fused_ms': ms, 'aa_spread': spread, 'torch_ms': result['torch']['median_ms'], 'fused_over_torch': ms / result['torch']['median_ms'],
        'holds': ms <= result['torch']['median_ms'] * (1 + spread + MARGIN),
    }
    return result


def measure_count(count, n, rounds, reps):
    """rank_count and rank_fold alone over a (count, n) matrix of random cosines"""
    matrix = torch.rand((count, n), dtype=torch.float32, device='cuda') * 2 - 1
    thresholds = torch.zeros((count,), dtype=torch.float32, device='cuda')
    marks = torch.full((count,), -1, dtype=torch.int64, device='cuda')
    counts = torch.empty((count,), dtype=torch.int64, device='cuda')
    workspace = torch.empty((_memb_ranks.dense_ranks_workspace_bytes(count, n),), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _memb_ranks.dense_ranks_to_device(0, matrix.data_ptr(), count, n, n, 0, thresholds.data_ptr(), marks.data_ptr(), 0, 0, 0, False,
                                          counts.data_ptr(), workspace.data_ptr(), workspace.numel(), stream)

    series = [timed(call, reps) for _ in range(rounds)]
    torch.cuda.synchronize()
    assert torch.equal(counts, (matrix > 0).sum(dim=1))
    ms = float(np.median(series))
    moved = 4 * count * n
    return {'queries': count, 'columns': n, 'bytes': moved, 'median_ms': ms, 'ms': series, 'bytes_per_second': moved / (ms * 1e-3),
            'share_of_hbm_peak': moved / (ms * 1e-3) / HBM_PEAK}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--queries', default='1,16,64')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('ranks.py measures on a GPU; none found')
    results = {}

    def save():
        if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
            with open(args.out, 'w') as f:
                json.dump(results, f, indent=1)

    for count in (int(value) for value in args.queries.split(',')):
        name = 'rank_count_{}x{}'.format(count, args.words)
        results[name] = measure_count(count, args.words, args.rounds, args.reps)
        print('{:28s} {:.4f} ms  {:.2f} TB/s  {:.1%} of the HBM peak'.format(
            name, results[name]['median_ms'], results[name]['bytes_per_second'] / 1e12, results[name]['share_of_hbm_peak']), flush=True)
        save()
    generator = torch.Generator(device='cuda').manual_seed(1)
    path, _ = synthetic.cached_model(args.words, 300, 'trained', 4)
    reader = memb_amd.Reader(path)
    for count in (int(value) for value in args.queries.split(',')):
        word_rows = torch.randint(0, args.words, (count, 2 + EXCLUDED), device='cuda', generator=generator, dtype=torch.int32)
        for with_list in (False, True):
            name = '4bit_{}xall_{}'.format(count, 'excluding3' if with_list else 'plain')
            results[name] = measure(reader, word_rows, with_list, args.rounds, args.reps)
            summary = results[name]['summary']
            print('{:22s} fused {:.4f} ms  A/A {:.1%} | matrix and torch {:.4f} ms  x{:.3f} of it ({}) | {}'.format(
                name, summary['fused_ms'], summary['aa_spread'], summary['torch_ms'], summary['fused_over_torch'],
                'holds' if summary['holds'] else 'DOES NOT HOLD', summary['kernel']), flush=True)
            save()


if __name__ == '__main__':
    main()
