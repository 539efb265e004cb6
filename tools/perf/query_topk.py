"""The k nearest candidates of every query (similarity_topk_device) against what a caller had before on ONE Reader, with
A/A controls. The method of tools/perf/query_matrix.py.

    python tools/perf/query_topk.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit] [--queries 1,16,64] [--ks 10,64] [--slices 8,128]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    topk            similarity_topk_device(queries, rows, k, workspace=the recommended one, allocated once)
    topkb           the same again: the A/A spread below which no difference stands
    matrix_topk     (a) similarity_matrix_device into a (Q, n) tensor + torch.topk(k): its values are checked against the
                    call's before anything is timed (its indices may differ among ties)
    matrix_sort     (b) similarity_matrix_device + torch.sort(descending=True, stable=True) cut to k: the only baseline with
                    the same indices, checked equal before anything is timed
    matrix          similarity_matrix_device alone: what is left of `topk` is the selection's share
    topk_<M>mib     the call with a workspace whose slice of the matrix is M MiB instead of the recommended 32 (--slices)
Configurations on the 4-bit and the 6-bit trained model of `words` words: Q in {1, 16, 64} queries (rows of the model)
against 50 000 candidates and against the whole vocabulary, k in {10, 64}. Reports medians over rounds, the peak device
memory each of `topk` and (a) allocates on top of its inputs, and the fraction of 8 TB/s that the call's algorithmic bytes
stand for (memb_hip_query_topk_algorithmic_bytes).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import memb_amd
from memb_amd import synthetic

HBM_BYTES_PER_S = 8.0e12   # MI355X_MICROARCH.md


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def peak_bytes(call):
    """the most device memory `call` holds at once on top of what is allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    kept = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del kept
    return peak


def measure(reader, query_rows, rows, k, rounds, reps, slices):
    n, count = rows.numel(), query_rows.numel()
    queries = reader.rows_embedding_device(query_rows)
    lists = reader._impl.query_topk_workspace_bytes(count, 1, k) - 4 * count
    workspace = torch.empty((reader._impl.query_topk_workspace_bytes(count, n, k),), dtype=torch.uint8, device='cuda')
    kept = {}

    def topk(space=workspace):
        kept['topk'] = reader.similarity_topk_device(queries, rows, k, workspace=space)

    def matrix_topk():
        kept['a'] = torch.topk(reader.similarity_matrix_device(queries, rows), k, dim=1)
        return kept['a']

    def matrix_sort():
        ordered = torch.sort(reader.similarity_matrix_device(queries, rows), dim=1, descending=True, stable=True)
        kept['b'] = (ordered.values[:, :k], ordered.indices[:, :k])

    variants = {'topk': topk, 'topkb': topk, 'matrix_topk': matrix_topk, 'matrix_sort': matrix_sort,
                'matrix': lambda: reader.similarity_matrix_device(queries, rows)}
    for mib in slices:
        width = min(n, max(64, (mib << 20) // (4 * count) // 64 * 64))
        space = torch.empty((lists + 4 * count * width,), dtype=torch.uint8, device='cuda')
        variants['topk_{}mib'.format(mib)] = lambda space=space: topk(space)
    for call in variants.values():
        call()
    kernel = reader.last_query_topk_kernel
    torch.cuda.synchronize()
    values, positions = kept['topk']
    assert torch.equal(values.view(torch.int32), kept['b'][0].view(torch.int32)) and torch.equal(positions, kept['b'][1]), 'the call and the stable sort differ'
    assert torch.equal(values, kept['a'].values), 'the call and torch.topk differ in a value'
    same_indices = float((positions == kept['a'].indices).float().mean())
    peaks = {'topk': peak_bytes(lambda: reader.similarity_topk_device(queries, rows, k)), 'matrix_topk': peak_bytes(matrix_topk)}
    kept.clear()
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    counted = reader._impl.query_topk_algorithmic_bytes(rows.cpu().numpy().view(np.uint32), count, k)
    ms = result['topk']['median_ms']
    result['summary'] = {
        'candidates': n, 'queries': count, 'k': k, 'kernel': kernel, 'topk_ms': ms,
        'aa_spread': abs(result['topkb']['median_ms'] - ms) / ms,
        'matrix_topk_ms': result['matrix_topk']['median_ms'], 'topk_over_matrix_topk': ms / result['matrix_topk']['median_ms'],
        'matrix_sort_ms': result['matrix_sort']['median_ms'], 'topk_over_matrix_sort': ms / result['matrix_sort']['median_ms'],
        'matrix_ms': result['matrix']['median_ms'], 'selection_share': 1 - result['matrix']['median_ms'] / ms,
        'torch_topk_same_indices': same_indices,
        'peak_bytes_topk': peaks['topk'], 'peak_bytes_matrix_topk': peaks['matrix_topk'], 'workspace_bytes': workspace.numel(),
        'bytes': counted, 'frac_of_8TBps': counted / (ms / 1e3) / HBM_BYTES_PER_S,
    }
    for mib in slices:
        result['summary']['topk_{}mib_ms'.format(mib)] = result['topk_{}mib'.format(mib)]['median_ms']
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--models', default='4bit,6bit')
    parser.add_argument('--queries', default='1,16,64')
    parser.add_argument('--ks', default='10,64')
    parser.add_argument('--slices', default='8,128')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('query_topk.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    slices = [int(value) for value in args.slices.split(',') if value]
    for label, bits in (('4bit', 4), ('6bit', 6)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(args.words, 300, 'trained', bits)
        reader = memb_amd.Reader(path)
        for shape, n in (('50000', 50000), ('all', args.words)):
            rows = torch.arange(n, dtype=torch.int32, device='cuda') if n >= args.words else \
                torch.sort(torch.randint(0, args.words, (n,), device='cuda', generator=generator, dtype=torch.int32)).values
            for count in (int(value) for value in args.queries.split(',')):
                query_rows = torch.randint(0, args.words, (count,), device='cuda', generator=generator, dtype=torch.int32)
                for k in (int(value) for value in args.ks.split(',')):
                    name = '{}_{}x{}_k{}'.format(label, count, shape, k)
                    results[name] = measure(reader, query_rows, rows, k, args.rounds, args.reps, slices if shape == 'all' else [])
                    summary = results[name]['summary']
                    print('{:24s} {:.4f} ms  A/A {:.1%} | (a) matrix + topk {:.4f} ms  x{:.2f} of it | (b) matrix + stable sort {:.4f} ms  '
                          'x{:.2f} of it | matrix alone {:.4f} ms, selection {:.0%} | peak {:.1f} MB against {:.1f} MB | {} | {:.3f} of 8 TB/s'.format(
                              name, summary['topk_ms'], summary['aa_spread'], summary['matrix_topk_ms'], summary['topk_over_matrix_topk'],
                              summary['matrix_sort_ms'], summary['topk_over_matrix_sort'], summary['matrix_ms'], summary['selection_share'],
                              summary['peak_bytes_topk'] / 1e6, summary['peak_bytes_matrix_topk'] / 1e6,
                              ' '.join('{} MiB {:.4f} ms'.format(mib, summary['topk_{}mib_ms'.format(mib)]) for mib in (slices if shape == 'all' else [])),
                              summary['frac_of_8TBps']), flush=True)
                    if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                        with open(args.out, 'w') as f:
                            json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
