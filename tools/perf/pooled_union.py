"""Pooled lookups of an averaged ReadersUnion (pooled_rows_device) against what a caller had before -- the union's decode
into an fp32 (n, dim) temporary, then a torch reduction over the bags -- with an A/A control, in pooled.py's style.

    python tools/perf/pooled_union.py [--rounds 5] [--reps 10] [--words 500000] [--out FILE.json] [--lengths 4,16,64]
                                      [--pairs 4bit_4bit,4bit_6bit] [--entries 100000,500000]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    fused      pooled_rows_device(rows, offsets, mode='mean', out=...): pool_trained_union, one kernel
    fusedb     the same again: the A/A spread below which no difference stands
    dense      the fallback on the same inputs (option union_fused = 0 on the first reader): the union's decode through the
               per-reader accumulate path into an fp32 temporary, then pool_dense
    merged_dense  the union's FUSED decode (decode_union_split / decode_trained_union) into an fp32 temporary, then
               pool_dense through the C entry point: the baseline's first step, the project's own second step
    two_step   the same fused decode, then out.index_add_(0, bag_of_entry, fp32) and a division by the counts
    two_step_sr  the same decode, then torch.segment_reduce(fp32, 'mean', offsets=...) (where this torch has it on the GPU)
The reductions of the two-step paths may add in another order: they are there for their time only; fused, dense and
merged_dense have the same bits, asserted before anything is timed.
Configurations: pairs of trained models of `words` words and dim 300 (4-bit / 4-bit of two seeds, 4-bit / 6-bit), seeded
geometric bag lengths over 100 000 and 500 000 entries, row ids in key order and shuffled (the same permutation for
both readers: an entry is one word). Reports medians over rounds, the speed-up over the faster two-step path and the
fraction of 8 TB/s that the fused call's algorithmic bytes stand for: per entry and reader the id, the metadata and the
stream (memb_hip_pooled_algorithmic_bytes of each reader, whose per-bag share is counted once).
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

from pooled import HBM_BYTES_PER_S, bag_offsets, timed


def measure(union, readers, rows, offsets, rounds, reps):
    n, bags, dim = rows[0].numel(), len(offsets) - 1, union.dim
    device_offsets = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    long_offsets = torch.from_numpy(offsets).cuda()
    counts = (long_offsets[1:] - long_offsets[:-1])
    bag_of_entry = torch.repeat_interleave(torch.arange(bags, device='cuda'), counts)
    divisor = counts.clamp(min=1).to(torch.float32)[:, None]
    fp32 = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    fused = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    dense = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    merged_dense_out = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    reduced = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def decode():
        union._merge_rows_device(rows, fp32, stream)

    def fallback():
        readers[0].set_option('union_fused', 0)
        try:
            union.pooled_rows_device(rows, device_offsets, mode='mean', out=dense)
        finally:
            readers[0].set_option('union_fused', 1)

    def merged_dense():
        decode()
        _memb.pool_dense_rows_to_device(0, fp32.data_ptr(), n, dim, dim, device_offsets.data_ptr(), bags,
                                        merged_dense_out.data_ptr(), dim, 0, _memb.POOL_MEAN, stream, _memb.OUT_F32)

    def two_step():
        decode()
        reduced.zero_()
        reduced.index_add_(0, bag_of_entry, fp32)
        reduced.div_(divisor)

    def two_step_sr():
        decode()
        return torch.segment_reduce(fp32, 'mean', offsets=long_offsets, axis=0, initial=0.0)

    variants = {
        'fused': lambda: union.pooled_rows_device(rows, device_offsets, mode='mean', out=fused),
        'fusedb': lambda: union.pooled_rows_device(rows, device_offsets, mode='mean', out=fused),
        'dense': fallback,
        'merged_dense': merged_dense,
        'two_step': two_step,
    }
    try:
        close = torch.allclose(two_step_sr(), union.pooled_rows_device(rows, device_offsets), rtol=1e-4, atol=1e-5)
        torch.cuda.synchronize()
        if close:
            variants['two_step_sr'] = two_step_sr
    except (RuntimeError, NotImplementedError, TypeError):
        pass
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    variants['dense']()
    fallback_kernel = union.last_pooled_kernel
    variants['fused']()
    fused_kernel = union.last_pooled_kernel
    assert fused_kernel.startswith('pool_trained_union<') and fallback_kernel.startswith('pool_dense<'), (fused_kernel, fallback_kernel)
    # the project's three paths agree in bits, the torch reduction to its reassociation, before anything is timed
    assert torch.equal(fused.view(torch.int32), dense.view(torch.int32))
    assert torch.equal(fused.view(torch.int32), merged_dense_out.view(torch.int32))
    assert torch.allclose(fused, reduced, rtol=1e-4, atol=1e-5)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    best_two_step = min(result[name]['median_ms'] for name in result if name.startswith('two_step'))
    fused_ms = result['fused']['median_ms']
    host_offsets = offsets.astype(np.uint32)
    per_bag = 8 * bags + 4 * dim * bags
    algorithmic = per_bag + sum(
        reader._impl.pooled_algorithmic_bytes(ids.cpu().numpy().view(np.uint32), host_offsets) - per_bag
        for reader, ids in zip(readers, rows))
    result['summary'] = {
        'entries': n, 'bags': bags, 'kernel': fused_kernel, 'fallback_kernel': fallback_kernel, 'fused_ms': fused_ms,
        'dense_ms': result['dense']['median_ms'], 'merged_dense_ms': result['merged_dense']['median_ms'], 'two_step_ms': best_two_step,
        'aa_spread': abs(result['fusedb']['median_ms'] - fused_ms) / fused_ms,
        'speedup': best_two_step / fused_ms, 'merged_dense_speedup': best_two_step / result['merged_dense']['median_ms'],
        'algorithmic_bytes': algorithmic, 'bytes_per_entry': algorithmic / n,
        'frac_of_8TBps': algorithmic / (fused_ms / 1e3) / HBM_BYTES_PER_S,
    }
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=500000)
    parser.add_argument('--out', default='')
    parser.add_argument('--lengths', default='4,16,64', help='mean bag lengths')
    parser.add_argument('--pairs', default='4bit_4bit,4bit_6bit')
    parser.add_argument('--entries', default='100000,500000')
    args = parser.parse_args()
    lengths = [int(length) for length in args.lengths.split(',')]
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('pooled_union.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, specs in (('4bit_4bit', ((4, 1234), (4, 77))), ('4bit_6bit', ((4, 1234), (6, 1234)))):
        if label not in args.pairs.split(','):
            continue
        readers = [memb_amd.Reader(synthetic.cached_model(args.words, 300, 'trained', bits, seed=seed)[0]) for bits, seed in specs]
        union = memb_amd.ReadersUnion(readers, 'average')
        for entries in sorted(int(value) for value in args.entries.split(',')):
            in_order = torch.arange(entries, dtype=torch.int32, device='cuda') if entries == args.words else \
                torch.sort(torch.randint(0, args.words, (entries,), device='cuda', generator=generator, dtype=torch.int32)).values
            orders = {'key_order': in_order,
                      'shuffled': in_order[torch.randperm(entries, device='cuda', generator=generator)].contiguous()}
            for order, ids in orders.items():
                for mean_length in lengths:
                    name = '{}_{}_{}_bags_of_{}'.format(label, entries, order, mean_length)
                    offsets = bag_offsets(entries, mean_length, mean_length)
                    results[name] = measure(union, readers, [ids, ids.clone()], offsets, args.rounds, args.reps)
                    summary = results[name]['summary']
                    print('{:44s} fused {:.4f} ms  A/A {:.1%}  dense {:.4f}  merged+dense {:.4f}  two-step {:.4f} ms  x{:.2f}  {:.0f} B/entry  {:.3f} of 8 TB/s'.format(
                        name, summary['fused_ms'], summary['aa_spread'], summary['dense_ms'], summary['merged_dense_ms'],
                        summary['two_step_ms'], summary['speedup'], summary['bytes_per_entry'], summary['frac_of_8TBps']), flush=True)
                    if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                        with open(args.out, 'w') as f:
                            json.dump(results, f, indent=1)
        del union, readers
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
