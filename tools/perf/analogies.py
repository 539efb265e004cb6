"""similarity_topk_device with an exclusion list against what a caller had before it on ONE Reader -- k + E entries and the
stable-sort drop most_similar_device uses --, with A/A controls. The method of tools/perf/query_topk.py.

    python tools/perf/analogies.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--queries 1,16,64] [--ks 10,61]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    excluding       similarity_topk_device(queries, None, k, exclude=lists, workspace=the recommended one, allocated once)
    excludingb      the same again: the A/A spread below which no difference stands
    drop            the baseline: similarity_topk_device(queries, None, k + 3, workspace=...) and the stable-sort drop; its
                    result is checked equal to the call's, bit for bit, before anything is timed
    empty           the new call with a list of width 0
    plain           similarity_topk_device(queries, None, k) without a list: what `empty` must not be slower than
Configurations on the 4-bit trained model of `words` words, every word a candidate: Q in {1, 16, 64} queries (rows of the
model), k in {10, 61}, three excluded positions per query chosen among that query's top entries (ranks 0, 1 and 4), so that
they do survive the threshold. Reports medians over rounds and whether each expectation holds: no slower than its
counterpart by more than the A/A spread plus 5 %.
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

EXCLUDED = 3
MARGIN = 0.05


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def measure(reader, query_rows, k, rounds, reps):
    count, n = query_rows.numel(), len(reader)
    queries = reader.rows_embedding_device(query_rows)
    workspace = torch.empty((reader._impl.query_topk_workspace_bytes(count, n, k + EXCLUDED),), dtype=torch.uint8, device='cuda')
    lists = reader.similarity_topk_device(queries, None, 8, workspace=workspace)[1][:, [0, 1, 4]].contiguous()
    none = lists[:, :0]
    kept = {}

    def excluding():
        kept['excluding'] = reader.similarity_topk_device(queries, None, k, workspace=workspace, exclude=lists)

    def drop():
        values, positions = reader.similarity_topk_device(queries, None, k + EXCLUDED, workspace=workspace)
        named = (positions.unsqueeze(2) == lists.unsqueeze(1)).any(dim=2)
        order = torch.sort(named.to(torch.int8), dim=1, stable=True).indices[:, :k]
        kept['drop'] = (torch.gather(values, 1, order), torch.gather(positions, 1, order))

    def empty():
        kept['empty'] = reader.similarity_topk_device(queries, None, k, workspace=workspace, exclude=none)

    def plain():
        kept['plain'] = reader.similarity_topk_device(queries, None, k, workspace=workspace)

    variants = {'excluding': excluding, 'excludingb': excluding, 'drop': drop, 'empty': empty, 'plain': plain}
    kernels = {}
    for name, call in variants.items():
        call()
        kernels[name] = reader.last_query_topk_kernel
    torch.cuda.synchronize()
    for new, old in (('excluding', 'drop'), ('empty', 'plain')):
        assert torch.equal(kept[new][0].view(torch.int32), kept[old][0].view(torch.int32)) and torch.equal(kept[new][1], kept[old][1]), \
            '{} and {} differ'.format(new, old)
    assert not (kept['excluding'][1].unsqueeze(2) == lists.unsqueeze(1)).any(), 'an excluded position was returned'
    assert not torch.equal(kept['excluding'][1], kept['plain'][1]), 'the list changed nothing'
    kept.clear()
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    ms = result['excluding']['median_ms']
    spread = abs(result['excludingb']['median_ms'] - ms) / ms
    result['summary'] = {
        'candidates': n, 'queries': count, 'k': k, 'excluded': EXCLUDED, 'kernel': kernels['excluding'], 'baseline_kernel': kernels['drop'],
        'excluding_ms': ms, 'aa_spread': spread, 'drop_ms': result['drop']['median_ms'],
        'excluding_over_drop': ms / result['drop']['median_ms'],
        'empty_ms': result['empty']['median_ms'], 'plain_ms': result['plain']['median_ms'],
        'empty_over_plain': result['empty']['median_ms'] / result['plain']['median_ms'],
        'excluding_holds': ms <= result['drop']['median_ms'] * (1 + spread + MARGIN),
        'empty_holds': result['empty']['median_ms'] <= result['plain']['median_ms'] * (1 + spread + MARGIN),
    }
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--queries', default='1,16,64')
    parser.add_argument('--ks', default='10,61')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('analogies.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    path, _ = synthetic.cached_model(args.words, 300, 'trained', 4)
    reader = memb_amd.Reader(path)
    for count in (int(value) for value in args.queries.split(',')):
        query_rows = torch.randint(0, args.words, (count,), device='cuda', generator=generator, dtype=torch.int32)
        for k in (int(value) for value in args.ks.split(',')):
            name = '4bit_{}xall_k{}'.format(count, k)
            results[name] = measure(reader, query_rows, k, args.rounds, args.reps)
            summary = results[name]['summary']
            print('{:20s} excluding {:.4f} ms  A/A {:.1%} | k + 3 and drop {:.4f} ms  x{:.3f} of it ({}) | width 0 {:.4f} ms against plain '
                  '{:.4f} ms  x{:.3f} ({}) | {}'.format(
                      name, summary['excluding_ms'], summary['aa_spread'], summary['drop_ms'], summary['excluding_over_drop'],
                      'holds' if summary['excluding_holds'] else 'DOES NOT HOLD', summary['empty_ms'], summary['plain_ms'],
                      summary['empty_over_plain'], 'holds' if summary['empty_holds'] else 'DOES NOT HOLD', summary['kernel']), flush=True)
            if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                with open(args.out, 'w') as f:
                    json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
