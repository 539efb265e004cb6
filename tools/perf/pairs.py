"""Cosine similarity of row pairs (pair_similarity_device) against the two-step paths a caller had before -- two decodes
into fp32 temporaries, then a torch reduction over them -- on ONE Reader, with A/A controls.

    python tools/perf/pairs.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit,uniform_8bit_500k]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    pairs           pair_similarity_device(pairs (n, 2), out=...)
    pairsb          the same again: the A/A spread below which no difference stands
    all_three       pair_similarity_device(pairs, return_dots=True, return_norms=True): 16 bytes per pair instead of 4
    two_step_unit   unit_rows_embedding_device(a, out=...), unit_rows_embedding_device(b, out=...), then (ua * ub).sum(1)
    two_step_cos    rows_embedding_device(a, out=...), rows_embedding_device(b, out=...), then
                    torch.nn.functional.cosine_similarity(xa, xb, dim=1)
    two_norms       row_norms_device(a, out=...), row_norms_device(b, out=...): the floor the extra product and the third
                    reduction sit on
torch's reductions add in another order: they are there for their time only (the bits are tests/test_gpu_pairs.py's).
Configurations: 50 000 pairs and len(reader) // 2 pairs, in key order and shuffled, of the 4-bit and the 6-bit trained
model of `words` words (the fused kernel), and the same of the 500 000-word uniform model (the plain decode and the dense
kernel). Reports medians over rounds, which kernel family ran, and the fraction of 8 TB/s that the call's algorithmic
bytes stand for (memb_hip_pairs_algorithmic_bytes).
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


def measure(reader, pairs, rounds, reps):
    n, dim = pairs.shape[0], reader.dim
    a, b = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    cosines = torch.empty((n,), dtype=torch.float32, device='cuda')
    norms_a = torch.empty((n,), dtype=torch.float32, device='cuda')
    norms_b = torch.empty((n,), dtype=torch.float32, device='cuda')
    rows_a = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    rows_b = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    kept = {}

    def two_step_unit():
        reader.unit_rows_embedding_device(a, out=rows_a)
        reader.unit_rows_embedding_device(b, out=rows_b)
        kept['unit'] = (rows_a * rows_b).sum(1)

    def two_step_cos():
        reader.rows_embedding_device(a, out=rows_a)
        reader.rows_embedding_device(b, out=rows_b)
        kept['cos'] = torch.nn.functional.cosine_similarity(rows_a, rows_b, dim=1)

    def two_norms():
        reader.row_norms_device(a, out=norms_a)
        reader.row_norms_device(b, out=norms_b)

    variants = {
        'pairs': lambda: reader.pair_similarity_device(pairs, out=cosines),
        'pairsb': lambda: reader.pair_similarity_device(pairs, out=cosines),
        'all_three': lambda: reader.pair_similarity_device(pairs, return_dots=True, return_norms=True, out=cosines),
        'two_step_unit': two_step_unit,
        'two_step_cos': two_step_cos,
        'two_norms': two_norms,
    }
    for call in variants.values():
        call()
    kernel = reader.last_pairs_kernel
    torch.cuda.synchronize()
    # the same quantity before anything is timed (another order of additions: close, not equal)
    assert torch.allclose(cosines, kept['unit'], rtol=0, atol=1e-5) and torch.allclose(cosines, kept['cos'], rtol=0, atol=1e-5)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    host_pairs = pairs.cpu().numpy().view(np.uint32)
    cosine_bytes = reader._impl.pairs_algorithmic_bytes(host_pairs, True, False, False)
    all_bytes = reader._impl.pairs_algorithmic_bytes(host_pairs, True, True, True)
    pairs_ms = result['pairs']['median_ms']
    result['summary'] = {
        'pairs': n, 'kernel': kernel, 'pairs_ms': pairs_ms,
        'aa_spread': abs(result['pairsb']['median_ms'] - pairs_ms) / pairs_ms,
        'all_three_ms': result['all_three']['median_ms'],
        'two_step_unit_ms': result['two_step_unit']['median_ms'],
        'speedup_over_unit': result['two_step_unit']['median_ms'] / pairs_ms,
        'two_step_cos_ms': result['two_step_cos']['median_ms'],
        'speedup_over_cos': result['two_step_cos']['median_ms'] / pairs_ms,
        'two_norms_ms': result['two_norms']['median_ms'],
        'bytes_per_pair': cosine_bytes / max(n, 1),
        'frac_of_8TBps': cosine_bytes / (pairs_ms / 1e3) / HBM_BYTES_PER_S,
        'all_three_frac_of_8TBps': all_bytes / (result['all_three']['median_ms'] / 1e3) / HBM_BYTES_PER_S,
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
        raise SystemExit('pairs.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for count in sorted({50000, words // 2}):
            entries = 2 * count
            in_order = torch.arange(entries, dtype=torch.int32, device='cuda') if entries >= words - 1 else \
                torch.sort(torch.randint(0, words, (entries,), device='cuda', generator=generator, dtype=torch.int32)).values
            orders = {'key_order': in_order.view(count, 2),
                      'shuffled': in_order[torch.randperm(entries, device='cuda', generator=generator)].contiguous().view(count, 2)}
            for order, pairs in orders.items():
                name = '{}_{}_{}'.format(label, count, order)
                results[name] = measure(reader, pairs, args.rounds, args.reps)
                summary = results[name]['summary']
                print('{:36s} {:13s} {:.4f} ms  A/A {:.1%}  all three {:.4f} ms | unit rows + sum {:.4f} ms  x{:.2f} | decodes + '
                      'cosine_similarity {:.4f} ms  x{:.2f} | two norms {:.4f} ms | {:.0f} B/pair  {:.3f} of 8 TB/s'.format(
                          name, summary['kernel'], summary['pairs_ms'], summary['aa_spread'], summary['all_three_ms'],
                          summary['two_step_unit_ms'], summary['speedup_over_unit'], summary['two_step_cos_ms'],
                          summary['speedup_over_cos'], summary['two_norms_ms'], summary['bytes_per_pair'],
                          summary['frac_of_8TBps']), flush=True)
                if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                    with open(args.out, 'w') as f:
                        json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
