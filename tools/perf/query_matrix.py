"""Cosine similarity of many query vectors against ONE shared candidate list (similarity_matrix_device) against what a
caller had before on ONE Reader, with A/A controls. The method of tools/perf/queries.py.

    python tools/perf/query_matrix.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit,uniform_8bit_500k] [--queries 1,4,16,64]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    matrix          similarity_matrix_device(queries, rows, out=...)
    matrixb         the same again: the A/A spread below which no difference stands
    repeated        (a) query_similarity_device over the candidate ids repeated once per query, offsets [0, n, 2n, ..]: every
                    compressed row fetched and decoded Q times. Its cosines are checked bit for bit against the matrix
                    before anything is timed
    decode_matmul   (b) rows_embedding_device of the candidates into an fp32 temporary, torch.nn.functional.normalize of both
                    sides and torch.matmul: 4 * dim bytes stored per row, other bits -- its largest difference from the
                    contract's cosines is reported beside its time
    row_norms       (c) row_norms_device over the n candidates, the floor of one decode
Configurations, each in key order and shuffled, on the 4-bit and the 6-bit trained model of `words` words (the fused kernel)
and on the 500 000-word uniform model (the fallback): Q in {1, 4, 16, 64} queries (rows of the model) against 50 000
candidates and against the whole vocabulary. Reports medians over rounds, which kernel family ran, and the fraction of
8 TB/s that the call's algorithmic bytes stand for (memb_hip_query_matrix_algorithmic_bytes).
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


def measure(reader, query_rows, rows, rounds, reps):
    n, dim, count = rows.numel(), reader.dim, query_rows.numel()
    queries = reader.rows_embedding_device(query_rows)
    repeated_rows = rows.repeat(count)
    offsets = torch.from_numpy((np.arange(count + 1, dtype=np.int64) * n).astype(np.uint32).view(np.int32)).cuda()   # (up to 2^32 - 1)
    matrix = torch.empty((count, n), dtype=torch.float32, device='cuda')
    by_queries = torch.empty((count * n,), dtype=torch.float32, device='cuda')
    norms = torch.empty((n,), dtype=torch.float32, device='cuda')
    decoded = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    kept = {}

    def decode_matmul():
        reader.rows_embedding_device(rows, out=decoded)
        kept['cos'] = torch.matmul(torch.nn.functional.normalize(queries, dim=1), torch.nn.functional.normalize(decoded, dim=1).t())

    variants = {
        'matrix': lambda: reader.similarity_matrix_device(queries, rows, out=matrix),
        'matrixb': lambda: reader.similarity_matrix_device(queries, rows, out=matrix),
        'repeated': lambda: reader.query_similarity_device(queries, repeated_rows, offsets, out=by_queries),
        'decode_matmul': decode_matmul,
        'row_norms': lambda: reader.row_norms_device(rows, out=norms),
    }
    for call in variants.values():
        call()
    kernel = reader.last_query_matrix_kernel
    torch.cuda.synchronize()
    # (a) is the same contract over the same pairs: the same bits, before anything is timed; (b) adds in another order
    assert torch.equal(matrix.view(torch.int32), by_queries.view(count, n).view(torch.int32)), 'the matrix and the repeated queries differ'
    matmul_difference = float((matrix - kept['cos']).abs().max())
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    cosine_bytes = reader._impl.query_matrix_algorithmic_bytes(rows.cpu().numpy().view(np.uint32), count, True, False, False)
    ms = result['matrix']['median_ms']
    result['summary'] = {
        'candidates': n, 'queries': count, 'kernel': kernel, 'matrix_ms': ms,
        'aa_spread': abs(result['matrixb']['median_ms'] - ms) / ms,
        'repeated_ms': result['repeated']['median_ms'],
        'speedup_over_repeated': result['repeated']['median_ms'] / ms,
        'decode_matmul_ms': result['decode_matmul']['median_ms'],
        'decode_matmul_over_matrix': result['decode_matmul']['median_ms'] / ms,
        'decode_matmul_max_difference': matmul_difference,
        'row_norms_ms': result['row_norms']['median_ms'],
        'over_row_norms': ms / result['row_norms']['median_ms'],
        'bytes': cosine_bytes,
        'frac_of_8TBps': cosine_bytes / (ms / 1e3) / HBM_BYTES_PER_S,
    }
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--models', default='4bit,6bit,uniform_8bit_500k')
    parser.add_argument('--queries', default='1,4,16,64')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('query_matrix.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for shape, n in (('50000', 50000), ('all', words)):
            in_order = torch.arange(n, dtype=torch.int32, device='cuda') if n >= words else \
                torch.sort(torch.randint(0, words, (n,), device='cuda', generator=generator, dtype=torch.int32)).values
            orders = {'key_order': in_order, 'shuffled': in_order[torch.randperm(n, device='cuda', generator=generator)].contiguous()}
            for count in (int(value) for value in args.queries.split(',')):
                query_rows = torch.randint(0, words, (count,), device='cuda', generator=generator, dtype=torch.int32)
                for order, rows in orders.items():
                    name = '{}_{}x{}_{}'.format(label, count, shape, order)
                    results[name] = measure(reader, query_rows, rows, args.rounds, args.reps)
                    summary = results[name]['summary']
                    print('{:36s} {:20s} {:.4f} ms  A/A {:.1%} | (a) repeated queries {:.4f} ms  x{:.2f} | (b) decode + matmul {:.4f} ms  '
                          'x{:.2f} of it, max |diff| {:.2e} | (c) row norms {:.4f} ms  x{:.2f} of it | {:.3f} of 8 TB/s'.format(
                              name, summary['kernel'], summary['matrix_ms'], summary['aa_spread'], summary['repeated_ms'],
                              summary['speedup_over_repeated'], summary['decode_matmul_ms'], summary['decode_matmul_over_matrix'],
                              summary['decode_matmul_max_difference'], summary['row_norms_ms'], summary['over_row_norms'],
                              summary['frac_of_8TBps']), flush=True)
                    if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                        with open(args.out, 'w') as f:
                            json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
