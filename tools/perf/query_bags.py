"""Every query against every pooled bag of rows (bag_similarity_matrix_device, bag_similarity_topk_device) against what a
caller had before on ONE Reader, with A/A controls. The method of tools/perf/query_topk.py.

    python tools/perf/query_bags.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit] [--queries 1,16,64] [--ks 10,64] [--corpora 100k,1m,long]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    matrix          bag_similarity_matrix_device(queries, rows, offsets) into a (Q, bags) tensor allocated once
    matrixb         the same again: the A/A spread below which no difference stands
    pooled_pairs    (a) the same bits by the parent's API: bags_embedding_device into a (bags, 2, dim) temporary allocated once,
                    then per query its row written beside the pooled rows and the dense pair kernel -- the route the fallback
                    takes; checked equal before anything is timed
    pooled_matmul   (b) OTHER bits, for information: bags_embedding_device, torch.nn.functional.normalize, torch.matmul
    topk_k<k>       bag_similarity_topk_device with the recommended workspace, allocated once
    topkb_k<k>      the same again
    sort_k<k>       (a) + torch.sort(descending=True, stable=True) cut to k: the same indices, checked equal
    matmul_topk_k<k>  (b) + torch.topk(k)
Corpora on the 4-bit and the 6-bit trained model of `words` words: 100 000 and 1 000 000 bags of 1 .. 23 entries (mean 12)
and 1 000 bags of 2 000 entries; Q in {1, 16, 64} queries (rows of the model); k in {10, 64}. Reports medians over rounds,
the peak device memory the fused call and (a) allocate on top of their inputs, and the fraction of 8 TB/s that the call's
algorithmic bytes stand for (memb_hip_query_bags_algorithmic_bytes).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import memb_amd
from memb_amd import _memb, synthetic

HBM_BYTES_PER_S = 8.0e12   # MI355X_MICROARCH.md
CORPORA = {'100k': (100000, 12), '1m': (1000000, 12), 'long': (1000, 2000)}


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


def corpus(words, bags, length, seed):
    rng = np.random.default_rng(seed)
    lengths = np.full(bags, length) if length > 100 else rng.integers(1, 2 * length, size=bags)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = rng.integers(0, words, size=int(offsets[-1]), dtype=np.int64).astype(np.uint32)
    return rows, offsets.astype(np.uint32)


def measure(reader, query_rows, rows, offsets, ks, rounds, reps):
    count, bags, dim = query_rows.numel(), offsets.size - 1, reader.dim
    queries = reader.rows_embedding_device(query_rows)
    on_device = torch.from_numpy(rows.view(np.int32)).cuda()
    cut = torch.from_numpy(offsets.view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((count, bags), dtype=torch.float32, device='cuda')
    second = torch.empty((count, bags), dtype=torch.float32, device='cuda')
    temporary = torch.empty((bags, 2, dim), dtype=torch.float32, device='cuda')
    kept = {}

    def matrix():
        return reader.bag_similarity_matrix_device(queries, on_device, cut, out=out)

    def pooled_pairs(target=second, side=None):
        side = temporary if side is None else side
        reader.bags_embedding_device(on_device, cut, out=side.view(bags, 2 * dim), col_off=dim)
        for q in range(count):
            side[:, 0] = queries[q]
            _memb.dense_pair_similarity_to_device(0, side.data_ptr(), bags, dim, dim, target[q].data_ptr(), 0, 0, stream)
        return target

    def pooled_matmul():
        pooled = torch.nn.functional.normalize(reader.bags_embedding_device(on_device, cut), dim=1)
        return torch.matmul(torch.nn.functional.normalize(queries, dim=1), pooled.t())

    variants = {'matrix': matrix, 'matrixb': matrix, 'pooled_pairs': pooled_pairs, 'pooled_matmul': pooled_matmul}
    workspaces = {}
    for k in ks:
        workspaces[k] = torch.empty((reader._impl.query_bags_topk_workspace_bytes(count, bags, k),), dtype=torch.uint8, device='cuda')

        def topk(k=k):
            kept['topk', k] = reader.bag_similarity_topk_device(queries, on_device, cut, k, workspace=workspaces[k])

        def sort(k=k):
            ordered = torch.sort(pooled_pairs(), dim=1, descending=True, stable=True)
            kept['sort', k] = (ordered.values[:, :k], ordered.indices[:, :k])

        variants['topk_k{}'.format(k)] = topk
        variants['topkb_k{}'.format(k)] = topk
        variants['sort_k{}'.format(k)] = sort
        variants['matmul_topk_k{}'.format(k)] = lambda k=k: torch.topk(pooled_matmul(), min(k, bags), dim=1)
    for call in variants.values():
        call()
    kernel, topk_kernel = reader.last_query_bags_kernel, reader.last_query_bags_topk_kernel
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), second.view(torch.int32)), 'the fused call and pooled rows + dense pairs differ'
    for k in ks:
        found = min(k, bags)
        values, positions = kept['topk', k]
        assert torch.equal(values[:, :found].view(torch.int32), kept['sort', k][0].view(torch.int32)) and \
            torch.equal(positions[:, :found], kept['sort', k][1]), 'the top-k call and the stable sort differ'
    other = float((pooled_matmul() - out).abs().max())
    kept.clear()
    peaks = {'matrix': peak_bytes(lambda: reader.bag_similarity_matrix_device(queries, on_device, cut, out=out)),
             'pooled_pairs': peak_bytes(lambda: pooled_pairs(out, torch.empty((bags, 2, dim), dtype=torch.float32, device='cuda'))),
             'pooled_matmul': peak_bytes(pooled_matmul)}
    for k in ks:
        peaks['topk_k{}'.format(k)] = peak_bytes(lambda k=k: reader.bag_similarity_topk_device(queries, on_device, cut, k))
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    counted = reader._impl.query_bags_algorithmic_bytes(rows, offsets, count)
    ms = result['matrix']['median_ms']
    summary = {
        'bags': bags, 'entries': int(rows.size), 'queries': count, 'kernel': kernel, 'topk_kernel': topk_kernel, 'matrix_ms': ms,
        'aa_spread': abs(result['matrixb']['median_ms'] - ms) / ms,
        'pooled_pairs_ms': result['pooled_pairs']['median_ms'], 'matrix_over_pooled_pairs': ms / result['pooled_pairs']['median_ms'],
        'pooled_matmul_ms': result['pooled_matmul']['median_ms'], 'matrix_over_pooled_matmul': ms / result['pooled_matmul']['median_ms'],
        'pooled_matmul_max_abs_difference': other, 'peak_bytes': peaks,
        'bytes': counted, 'frac_of_8TBps': counted / (ms / 1e3) / HBM_BYTES_PER_S,
    }
    for k in ks:
        mine = result['topk_k{}'.format(k)]['median_ms']
        summary['k{}'.format(k)] = {
            'topk_ms': mine, 'aa_spread': abs(result['topkb_k{}'.format(k)]['median_ms'] - mine) / mine,
            'sort_ms': result['sort_k{}'.format(k)]['median_ms'], 'topk_over_sort': mine / result['sort_k{}'.format(k)]['median_ms'],
            'matmul_topk_ms': result['matmul_topk_k{}'.format(k)]['median_ms'],
            'topk_over_matmul_topk': mine / result['matmul_topk_k{}'.format(k)]['median_ms'], 'workspace_bytes': workspaces[k].numel()}
    result['summary'] = summary
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
    parser.add_argument('--corpora', default='100k,1m,long')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('query_bags.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    ks = [int(value) for value in args.ks.split(',') if value]
    for label, bits in (('4bit', 4), ('6bit', 6)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(args.words, 300, 'trained', bits)
        reader = memb_amd.Reader(path)
        for shape in args.corpora.split(','):
            bags, length = CORPORA[shape]
            rows, offsets = corpus(args.words, bags, length, bags)
            for count in (int(value) for value in args.queries.split(',')):
                query_rows = torch.randint(0, args.words, (count,), device='cuda', generator=generator, dtype=torch.int32)
                name = '{}_{}x{}'.format(label, count, shape)
                results[name] = measure(reader, query_rows, rows, offsets, ks, args.rounds, args.reps)
                summary = results[name]['summary']
                print('{:16s} {:.4f} ms  A/A {:.1%} | (a) pooled + pairs {:.4f} ms  x{:.2f} of it | (b) pooled + matmul {:.4f} ms  x{:.2f} '
                      'of it | peak {:.1f} MB against {:.1f} MB | {:.3f} of 8 TB/s | {}'.format(
                          name, summary['matrix_ms'], summary['aa_spread'], summary['pooled_pairs_ms'], summary['matrix_over_pooled_pairs'],
                          summary['pooled_matmul_ms'], summary['matrix_over_pooled_matmul'], summary['peak_bytes']['matrix'] / 1e6,
                          summary['peak_bytes']['pooled_pairs'] / 1e6, summary['frac_of_8TBps'],
                          ' | '.join('k={} {:.4f} ms A/A {:.1%}, x{:.2f} of (a) + stable sort, x{:.2f} of (b) + topk'.format(
                              k, summary['k{}'.format(k)]['topk_ms'], summary['k{}'.format(k)]['aa_spread'],
                              summary['k{}'.format(k)]['topk_over_sort'], summary['k{}'.format(k)]['topk_over_matmul_topk']) for k in ks)),
                      flush=True)
                if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                    with open(args.out, 'w') as f:
                        json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
