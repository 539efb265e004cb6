"""Cosine similarity of query vectors against groups of candidate rows (query_similarity_device) against what a caller
had before on ONE Reader, with A/A controls.

    python tools/perf/queries.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit,uniform_8bit_500k]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    queries         query_similarity_device(queries, rows, offsets, out=...)
    queriesb        the same again: the A/A spread below which no difference stands
    all_three       query_similarity_device(..., return_dots=True, return_norms=True): 12 bytes per candidate instead of 4
    repeated_pairs  (a) pair_similarity_device over (query row id, candidate) pairs, the query's id repeated beside every
                    candidate: decodes twice the rows. The queries are rows of the model here, so that (a) exists at all; its
                    cosines are checked bit for bit against the fused call's before anything is timed
    decode_cos      (b) rows_embedding_device of the candidates into an fp32 temporary and
                    torch.nn.functional.cosine_similarity against the queries expanded by group: 4 * dim bytes stored per row
    row_norms       (c) row_norms_device over the candidates, the floor: the same decode with one reduction
torch's reduction adds in another order: it is there for its time only (the bits are tests/test_gpu_queries.py's).
Configurations, each in key order and shuffled, on the 4-bit and the 6-bit trained model of `words` words (the fused
kernel): one query against 50 000 candidates, one query against the whole vocabulary, 5 000 groups of 10 and 500 groups
of 100; and the same on the 500 000-word uniform model (the plain decode and the dense kernel). Reports medians over
rounds, which kernel family ran, and the fraction of 8 TB/s that the call's algorithmic bytes stand for
(memb_hip_query_algorithmic_bytes).
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


def measure(reader, query_rows, rows, offsets, rounds, reps):
    n, dim, groups = rows.numel(), reader.dim, query_rows.numel()
    queries = reader.rows_embedding_device(query_rows)
    lengths = (offsets[1:] - offsets[:-1]).to(torch.int64)
    group = torch.repeat_interleave(torch.arange(groups, device='cuda'), lengths)
    pairs = torch.stack((query_rows[group], rows), dim=1).contiguous()
    cosines = torch.empty((n,), dtype=torch.float32, device='cuda')
    by_pairs = torch.empty((n,), dtype=torch.float32, device='cuda')
    norms = torch.empty((n,), dtype=torch.float32, device='cuda')
    decoded = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    kept = {}

    def decode_cos():
        reader.rows_embedding_device(rows, out=decoded)
        kept['cos'] = torch.nn.functional.cosine_similarity(decoded, queries[group] if groups > 1 else queries, dim=1)

    variants = {
        'queries': lambda: reader.query_similarity_device(queries, rows, offsets, out=cosines),
        'queriesb': lambda: reader.query_similarity_device(queries, rows, offsets, out=cosines),
        'all_three': lambda: reader.query_similarity_device(queries, rows, offsets, return_dots=True, return_norms=True, out=cosines),
        'repeated_pairs': lambda: reader.pair_similarity_device(pairs, out=by_pairs),
        'decode_cos': decode_cos,
        'row_norms': lambda: reader.row_norms_device(rows, out=norms),
    }
    for call in variants.values():
        call()
    kernel = reader.last_query_kernel
    torch.cuda.synchronize()
    # (a) is the same contract over the same two rows: the same bits, before anything is timed; (b) adds in another order
    assert torch.equal(cosines.view(torch.int32), by_pairs.view(torch.int32)), 'the fused call and the repeated pairs differ'
    assert torch.allclose(cosines, kept['cos'], rtol=0, atol=1e-5)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    host_rows, host_offsets = rows.cpu().numpy().view(np.uint32), offsets.cpu().numpy().view(np.uint32)
    cosine_bytes = reader._impl.query_algorithmic_bytes(host_rows, host_offsets, True, False, False)
    ms = result['queries']['median_ms']
    result['summary'] = {
        'candidates': n, 'groups': groups, 'kernel': kernel, 'queries_ms': ms,
        'aa_spread': abs(result['queriesb']['median_ms'] - ms) / ms,
        'all_three_ms': result['all_three']['median_ms'],
        'repeated_pairs_ms': result['repeated_pairs']['median_ms'],
        'speedup_over_pairs': result['repeated_pairs']['median_ms'] / ms,
        'decode_cos_ms': result['decode_cos']['median_ms'],
        'speedup_over_cos': result['decode_cos']['median_ms'] / ms,
        'row_norms_ms': result['row_norms']['median_ms'],
        'over_row_norms': ms / result['row_norms']['median_ms'],
        'bytes_per_candidate': cosine_bytes / max(n, 1),
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
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('queries.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for shape, groups, per_group in (('1x50000', 1, 50000), ('1xall', 1, words), ('5000x10', 5000, 10), ('500x100', 500, 100)):
            n = groups * per_group
            in_order = torch.arange(n, dtype=torch.int32, device='cuda') if n >= words else \
                torch.sort(torch.randint(0, words, (n,), device='cuda', generator=generator, dtype=torch.int32)).values
            offsets = (torch.arange(groups + 1, dtype=torch.int64, device='cuda') * per_group).to(torch.int32)
            query_rows = torch.randint(0, words, (groups,), device='cuda', generator=generator, dtype=torch.int32)
            orders = {'key_order': in_order, 'shuffled': in_order[torch.randperm(n, device='cuda', generator=generator)].contiguous()}
            for order, rows in orders.items():
                name = '{}_{}_{}'.format(label, shape, order)
                results[name] = measure(reader, query_rows, rows, offsets, args.rounds, args.reps)
                summary = results[name]['summary']
                print('{:34s} {:13s} {:.4f} ms  A/A {:.1%}  all three {:.4f} ms | (a) repeated pairs {:.4f} ms  x{:.2f} | (b) decode + '
                      'cosine_similarity {:.4f} ms  x{:.2f} | (c) row norms {:.4f} ms  x{:.2f} of it | {:.0f} B/candidate  {:.3f} of 8 TB/s'.format(
                          name, summary['kernel'], summary['queries_ms'], summary['aa_spread'], summary['all_three_ms'],
                          summary['repeated_pairs_ms'], summary['speedup_over_pairs'], summary['decode_cos_ms'],
                          summary['speedup_over_cos'], summary['row_norms_ms'], summary['over_row_norms'],
                          summary['bytes_per_candidate'], summary['frac_of_8TBps']), flush=True)
                if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                    with open(args.out, 'w') as f:
                        json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
