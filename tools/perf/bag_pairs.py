"""Cosine similarity of pairs of bags (bag_pair_similarity_device) against the two-step paths a caller had before -- the
bags pooled into one fp32 (2 * pairs, dim) tensor, then a reduction over its even and odd rows -- on ONE Reader, with A/A
controls.

    python tools/perf/bag_pairs.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit,uniform_8bit_500k]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    fused           bag_pair_similarity_device(rows, offsets, out=...)
    fusedb          the same again: the A/A spread below which no difference stands
    all_three       bag_pair_similarity_device(rows, offsets, return_dots=True, return_norms=True): 16 bytes per pair, not 4
    pool_torch      (a) bags_embedding_device(rows, offsets, out=...), then torch.nn.functional.cosine_similarity over the
                    even and the odd rows
    pool_dense      (b) the same pooling, then _memb.dense_pair_similarity_to_device: the fallback's two kernels
    pool_alone      (c) the pooling alone, as the floor: the same decode and additions, plus the row stores the fused kernel
                    does not make
torch's reduction adds in another order: it is there for its time only (the bits are tests/test_gpu_bag_pairs.py's; (b)
must have the fused call's bits and is checked before anything is timed).
Configurations: bags of 8 and of 32 entries; 50 000 pairs (ids drawn with repeats) and the largest pair count the
vocabulary gives without a repeat, len(reader) // (2 * entries); entries in key order and shuffled; the 4-bit and the 6-bit
trained model of `words` words (the fused kernel) and the 500 000-word uniform model (the pooled lookup and the dense
kernel). Reports medians over rounds, which kernel family ran, and the fraction of 8 TB/s that the call's algorithmic bytes
stand for (memb_hip_bag_pairs_algorithmic_bytes).
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
BAG_LENGTHS = (8, 32)


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def measure(reader, rows, offsets, rounds, reps):
    n, dim = offsets.numel() // 2, reader.dim
    index = reader.device
    cosines = torch.empty((n,), dtype=torch.float32, device='cuda')
    second = torch.empty((n,), dtype=torch.float32, device='cuda')
    pooled = torch.empty((2 * n, dim), dtype=torch.float32, device='cuda')
    kept = {}

    def pool_torch():
        reader.bags_embedding_device(rows, offsets, out=pooled)
        kept['cos'] = torch.nn.functional.cosine_similarity(pooled[0::2], pooled[1::2], dim=1)

    def pool_dense():
        reader.bags_embedding_device(rows, offsets, out=pooled)
        _memb.dense_pair_similarity_to_device(
            index, pooled.data_ptr(), n, dim, dim, second.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)

    variants = {
        'fused': lambda: reader.bag_pair_similarity_device(rows, offsets, out=cosines),
        'fusedb': lambda: reader.bag_pair_similarity_device(rows, offsets, out=cosines),
        'all_three': lambda: reader.bag_pair_similarity_device(rows, offsets, return_dots=True, return_norms=True, out=cosines),
        'pool_torch': pool_torch,
        'pool_dense': pool_dense,
        'pool_alone': lambda: reader.bags_embedding_device(rows, offsets, out=pooled),
    }
    for call in variants.values():
        call()
    kernel = reader.last_bag_pairs_kernel
    torch.cuda.synchronize()
    # the same quantity before anything is timed: (b) bit for bit, torch's close (another order of additions)
    assert torch.equal(cosines.view(torch.int32), second.view(torch.int32))
    assert torch.allclose(cosines, kept['cos'], rtol=0, atol=1e-5)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    host_rows, host_offsets = rows.cpu().numpy().view(np.uint32), offsets.cpu().numpy().view(np.uint32)
    cosine_bytes = reader._impl.bag_pairs_algorithmic_bytes(host_rows, host_offsets, True, False, False)
    fused_ms = result['fused']['median_ms']
    result['summary'] = {
        'pairs': n, 'entries': rows.numel(), 'kernel': kernel, 'fused_ms': fused_ms,
        'aa_spread': abs(result['fusedb']['median_ms'] - fused_ms) / fused_ms,
        'all_three_ms': result['all_three']['median_ms'],
        'pool_torch_ms': result['pool_torch']['median_ms'],
        'speedup_over_pool_torch': result['pool_torch']['median_ms'] / fused_ms,
        'pool_dense_ms': result['pool_dense']['median_ms'],
        'speedup_over_pool_dense': result['pool_dense']['median_ms'] / fused_ms,
        'pool_alone_ms': result['pool_alone']['median_ms'],
        'fused_over_pool_alone': fused_ms / result['pool_alone']['median_ms'],
        'bytes_per_pair': cosine_bytes / max(n, 1),
        'frac_of_8TBps': cosine_bytes / (fused_ms / 1e3) / HBM_BYTES_PER_S,
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
        raise SystemExit('bag_pairs.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for length in BAG_LENGTHS:
            for count in sorted({50000, words // (2 * length)}):
                entries = 2 * length * count
                in_order = torch.arange(entries, dtype=torch.int32, device='cuda') if count == words // (2 * length) else \
                    torch.sort(torch.randint(0, words, (entries,), device='cuda', generator=generator, dtype=torch.int32)).values
                offsets = (torch.arange(2 * count + 1, dtype=torch.int64, device='cuda') * length).to(torch.int32)
                orders = {'key_order': in_order,
                          'shuffled': in_order[torch.randperm(entries, device='cuda', generator=generator)].contiguous()}
                for order, rows in orders.items():
                    name = '{}_{}x{}_{}'.format(label, count, length, order)
                    results[name] = measure(reader, rows, offsets, args.rounds, args.reps)
                    summary = results[name]['summary']
                    print('{:40s} {:17s} {:.4f} ms  A/A {:.1%}  all three {:.4f} ms | (a) pool + cosine_similarity {:.4f} ms  x{:.2f} | '
                          '(b) pool + pairs_dense {:.4f} ms  x{:.2f} | (c) pool alone {:.4f} ms  fused / (c) {:.2f} | {:.0f} B/pair  '
                          '{:.3f} of 8 TB/s'.format(
                              name, summary['kernel'], summary['fused_ms'], summary['aa_spread'], summary['all_three_ms'],
                              summary['pool_torch_ms'], summary['speedup_over_pool_torch'], summary['pool_dense_ms'],
                              summary['speedup_over_pool_dense'], summary['pool_alone_ms'], summary['fused_over_pool_alone'],
                              summary['bytes_per_pair'], summary['frac_of_8TBps']), flush=True)
                    if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                        with open(args.out, 'w') as f:
                            json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
