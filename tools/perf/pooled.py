"""Pooled lookups (bags_embedding_device) against the two-step path a caller had before -- rows_embedding_device into an
fp32 temporary, then a torch reduction over the bags -- on ONE Reader, with an A/A control.

    python tools/perf/pooled.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json]
                                [--dtype bfloat16|float16] [--lengths 1,4,16,64] [--models 4bit]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    pooled     bags_embedding_device(rows, offsets, mode='mean', out=...)
    pooledb    the same again: the A/A spread below which no difference stands
    two_step   rows_embedding_device(rows, out=fp32), then out.index_add_(0, bag_of_entry, fp32) and a division by the counts
    two_step_sr  the same decode, then torch.segment_reduce(fp32, 'mean', offsets=...) (where this torch has it on the GPU)
The reductions of the two-step paths may add in another order: they are there for their time only.
Configurations: seeded geometric bag lengths of mean 4, 16 and 64 over 100 000 entries and over `words` entries, row ids in
key order and shuffled, on the 4-bit and the 6-bit trained model of `words` words and on the 500 000-word uniform model.
Reports medians over rounds and, for the pooled call, the fraction of 8 TB/s that its algorithmic bytes stand for
(memb_hip_pooled_algorithmic_bytes, DESIGN.md section 5.6: per entry the id, the metadata and the stream, per bag two
offsets and 4 dim bytes).
With --dtype bfloat16 / float16 `pooled` and `pooledb` are the one-kernel narrow call (dtype=...), and two more variants are
timed in the same rounds: `fp32_then_cast` (the float32 pooled call, then .to(dtype): what a caller had before) and `fp32`
(the float32 pooled call alone). The fraction of 8 TB/s then comes from the typed byte count
(memb_hip_pooled_algorithmic_bytes_typed: 2 dim bytes stored per bag); the two-step paths are left out.
With --missing skip [--missing-share P[,P..]] a seeded share P of the entries is set to 0xFFFFFFFF and three variants are timed in
the same rounds (float32): `skip` / `skipb` (bags_embedding_device(..., missing='skip'), and again: the A/A spread),
`compact_then_pool` (what a caller had before: the ids compacted and the offsets rebuilt by torch on the device, then the
existing call -- the same bits, asserted before anything is timed) and `zero` (the existing call on the same uncompacted
inputs, missing='zero': another result, the cost floor).

With --reduction sequential,chunked the two summation orders of bags_embedding_device are timed in the same rounds (float32,
mean): `chunked` / `chunkedb` (reduction='chunked', and again: the A/A spread), `sequential` (the default order: one wavefront
walks a whole bag) and the two-step paths above. --fixed BAGSxLENGTH[,..] adds batches of equal bags (1x100000: one bag of
100 000 entries; 1000x2000), shuffled rows of the model.
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


def bag_offsets(entries, mean_length, seed):
    """seeded geometric bag lengths of this mean that cover `entries` entries exactly"""
    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / mean_length, size=int(entries / mean_length * 1.2) + 16)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    offsets = offsets[:np.searchsorted(offsets, entries)]
    return np.append(offsets, entries).astype(np.int64)


OUT_TYPES = {'float32': (torch.float32, 0), 'bfloat16': (torch.bfloat16, 1), 'float16': (torch.float16, 2)}   # MEMB_HIP_OUT_*


def measure_narrow(reader, rows, offsets, rounds, reps, dtype_name):
    dtype, out_type = OUT_TYPES[dtype_name]
    n, bags, dim = rows.numel(), len(offsets) - 1, reader.dim
    device_offsets = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    narrow = torch.empty((bags, dim), dtype=dtype, device='cuda')
    fp32 = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    cast = torch.empty((bags, dim), dtype=dtype, device='cuda')

    def fp32_then_cast():
        reader.bags_embedding_device(rows, device_offsets, mode='mean', out=fp32)
        cast.copy_(fp32)

    variants = {
        'pooled': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=narrow, dtype=dtype),
        'pooledb': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=narrow, dtype=dtype),
        'fp32_then_cast': fp32_then_cast,
        'fp32': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=fp32),
    }
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    assert torch.equal(narrow.view(torch.int16), cast.view(torch.int16))   # the same bits before anything is timed
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    host_rows, host_offsets = rows.cpu().numpy().view(np.uint32), offsets.astype(np.uint32)
    typed = reader._impl.pooled_algorithmic_bytes(host_rows, host_offsets, out_type)
    fp32_bytes = reader._impl.pooled_algorithmic_bytes(host_rows, host_offsets)
    pooled_ms = result['pooled']['median_ms']
    result['summary'] = {
        'dtype': dtype_name, 'entries': n, 'bags': bags, 'pooled_ms': pooled_ms,
        'fp32_then_cast_ms': result['fp32_then_cast']['median_ms'], 'fp32_ms': result['fp32']['median_ms'],
        'aa_spread': abs(result['pooledb']['median_ms'] - pooled_ms) / pooled_ms,
        'algorithmic_bytes': typed, 'fp32_algorithmic_bytes': fp32_bytes, 'bytes_ratio': typed / fp32_bytes,
        'frac_of_8TBps': typed / (pooled_ms / 1e3) / HBM_BYTES_PER_S,
        'fp32_frac_of_8TBps': fp32_bytes / (result['fp32']['median_ms'] / 1e3) / HBM_BYTES_PER_S,
    }
    return result


def measure_skip(reader, rows, offsets, rounds, reps, share, seed):
    n, bags, dim = rows.numel(), len(offsets) - 1, reader.dim
    rows = rows.clone()
    generator = torch.Generator(device='cuda').manual_seed(seed)
    rows[torch.rand(n, device='cuda', generator=generator) < share] = -1   # 0xFFFFFFFF
    device_offsets = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    long_offsets = torch.from_numpy(offsets).cuda()
    skipped = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    compact = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    counted = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    zero = torch.zeros(1, dtype=torch.int64, device='cuda')

    def compact_then_pool():
        keep = rows != -1
        before = torch.cat([zero, torch.cumsum(keep, 0)])
        reader.bags_embedding_device(rows[keep], before[long_offsets].to(torch.int32), mode='mean', out=compact)

    variants = {
        'skip': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=skipped, missing='skip'),
        'skipb': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=skipped, missing='skip'),
        'compact_then_pool': compact_then_pool,
        'zero': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=counted),
    }
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    assert torch.equal(skipped.view(torch.int32), compact.view(torch.int32))   # the same bits before anything is timed
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    skip_ms = result['skip']['median_ms']
    result['summary'] = {
        'entries': n, 'bags': bags, 'missing_share': share, 'unknown_entries': int((rows == -1).sum()), 'skip_ms': skip_ms,
        'compact_then_pool_ms': result['compact_then_pool']['median_ms'], 'zero_ms': result['zero']['median_ms'],
        'aa_spread': abs(result['skipb']['median_ms'] - skip_ms) / skip_ms,
        'skip_over_compact': skip_ms / result['compact_then_pool']['median_ms'],
        'skip_over_zero': skip_ms / result['zero']['median_ms'],
    }
    return result


def measure(reader, rows, offsets, rounds, reps):
    n, bags, dim = rows.numel(), len(offsets) - 1, reader.dim
    device_offsets = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    long_offsets = torch.from_numpy(offsets).cuda()
    counts = (long_offsets[1:] - long_offsets[:-1])
    bag_of_entry = torch.repeat_interleave(torch.arange(bags, device='cuda'), counts)
    divisor = counts.clamp(min=1).to(torch.float32)[:, None]
    fp32 = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    pooled = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    reduced = torch.empty((bags, dim), dtype=torch.float32, device='cuda')

    def two_step():
        reader.rows_embedding_device(rows, out=fp32)
        reduced.zero_()
        reduced.index_add_(0, bag_of_entry, fp32)
        reduced.div_(divisor)

    def two_step_sr():
        reader.rows_embedding_device(rows, out=fp32)
        return torch.segment_reduce(fp32, 'mean', offsets=long_offsets, axis=0, initial=0.0)

    variants = {
        'pooled': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=pooled),
        'pooledb': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=pooled),
        'two_step': two_step,
    }
    try:
        close = torch.allclose(two_step_sr(), reader.bags_embedding_device(rows, device_offsets), rtol=1e-4, atol=1e-5)
        torch.cuda.synchronize()
        if close:
            variants['two_step_sr'] = two_step_sr
    except (RuntimeError, NotImplementedError, TypeError):
        pass
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    # the paths agree (to the reassociation of the torch reduction) before anything is timed
    assert torch.allclose(pooled, reduced, rtol=1e-4, atol=1e-5)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    best_two_step = min(result[name]['median_ms'] for name in result if name.startswith('two_step'))
    pooled_ms = result['pooled']['median_ms']
    algorithmic = reader._impl.pooled_algorithmic_bytes(rows.cpu().numpy().view(np.uint32), offsets.astype(np.uint32))
    result['summary'] = {
        'entries': n, 'bags': bags, 'pooled_ms': pooled_ms, 'two_step_ms': best_two_step,
        'aa_spread': abs(result['pooledb']['median_ms'] - pooled_ms) / pooled_ms,
        'speedup': best_two_step / pooled_ms,
        'algorithmic_bytes': algorithmic, 'bytes_per_entry': algorithmic / n,
        'frac_of_8TBps': algorithmic / (pooled_ms / 1e3) / HBM_BYTES_PER_S,
    }
    return result


def measure_reduction(reader, rows, offsets, rounds, reps):
    n, bags, dim = rows.numel(), len(offsets) - 1, reader.dim
    device_offsets = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    long_offsets = torch.from_numpy(offsets).cuda()
    counts = (long_offsets[1:] - long_offsets[:-1])
    bag_of_entry = torch.repeat_interleave(torch.arange(bags, device='cuda'), counts)
    divisor = counts.clamp(min=1).to(torch.float32)[:, None]
    fp32 = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    chunked = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    sequential = torch.empty((bags, dim), dtype=torch.float32, device='cuda')
    reduced = torch.empty((bags, dim), dtype=torch.float32, device='cuda')

    def two_step():
        reader.rows_embedding_device(rows, out=fp32)
        reduced.zero_()
        reduced.index_add_(0, bag_of_entry, fp32)
        reduced.div_(divisor)

    def two_step_sr():
        reader.rows_embedding_device(rows, out=fp32)
        return torch.segment_reduce(fp32, 'mean', offsets=long_offsets, axis=0, initial=0.0)

    variants = {
        'chunked': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=chunked, reduction='chunked'),
        'chunkedb': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=chunked, reduction='chunked'),
        'sequential': lambda: reader.bags_embedding_device(rows, device_offsets, mode='mean', out=sequential),
        'two_step': two_step,
    }
    try:
        close = torch.allclose(two_step_sr(), reader.bags_embedding_device(rows, device_offsets), rtol=1e-3, atol=1e-4)
        torch.cuda.synchronize()
        if close:
            variants['two_step_sr'] = two_step_sr
    except (RuntimeError, NotImplementedError, TypeError):
        pass
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    # the orders agree to their reassociation before anything is timed; bags of at most a chunk in bits
    assert torch.allclose(chunked, sequential, rtol=1e-3, atol=1e-4)
    short = (counts <= memb_amd.POOL_CHUNK)
    assert torch.equal(chunked[short].view(torch.int32), sequential[short].view(torch.int32))
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    best_two_step = min(result[name]['median_ms'] for name in result if name.startswith('two_step'))
    chunked_ms = result['chunked']['median_ms']
    result['summary'] = {
        'entries': n, 'bags': bags, 'chunk': memb_amd.POOL_CHUNK, 'chunked_ms': chunked_ms,
        'sequential_ms': result['sequential']['median_ms'], 'two_step_ms': best_two_step,
        'aa_spread': abs(result['chunkedb']['median_ms'] - chunked_ms) / chunked_ms,
        'chunked_over_sequential': result['sequential']['median_ms'] / chunked_ms,
        'chunked_over_two_step': best_two_step / chunked_ms,
        'sequential_over_two_step': best_two_step / result['sequential']['median_ms'],
        'workspace_bytes': reader._impl.pool_chunked_workspace_bytes(n, bags),
    }
    return result


def report_reduction(results, name, reader, rows, offsets, args):
    results[name] = measure_reduction(reader, rows, offsets, args.rounds, args.reps)
    summary = results[name]['summary']
    print('{:48s} chunked {:.4f} ms  A/A {:.1%}  sequential {:.4f} ms (x{:.2f})  two-step {:.4f} ms (x{:.2f})'.format(
        name, summary['chunked_ms'], summary['aa_spread'], summary['sequential_ms'], summary['chunked_over_sequential'],
        summary['two_step_ms'], summary['chunked_over_two_step']), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--dtype', default='float32', choices=sorted(OUT_TYPES))
    parser.add_argument('--lengths', default='4,16,64', help='mean bag lengths (1: every bag one entry)')
    parser.add_argument('--models', default='4bit,6bit,uniform_8bit_500k')
    parser.add_argument('--missing', default='zero', choices=['zero', 'skip'], help="skip: time missing='skip' (float32)")
    parser.add_argument('--missing-share', default='0', help='seeded share(s) of the entries set to 0xFFFFFFFF, e.g. 0,0.1,0.5')
    parser.add_argument('--reduction', default='', help="sequential,chunked: time reduction='chunked' beside the default order")
    parser.add_argument('--fixed', default='', help='with --reduction: batches of equal bags, BAGSxLENGTH[,..] (shuffled rows)')
    args = parser.parse_args()
    if args.reduction and sorted(args.reduction.split(',')) != ['chunked', 'sequential']:
        raise SystemExit('--reduction takes sequential,chunked')
    lengths = [int(length) for length in args.lengths.split(',')]
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('pooled.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for shape in (args.fixed.split(',') if args.reduction and args.fixed else ()):
            bags, length = (int(value) for value in shape.split('x'))
            rows = torch.randint(0, words, (bags * length,), device='cuda', generator=generator, dtype=torch.int32)
            report_reduction(results, '{}_{}_bags_of_exactly_{}'.format(label, bags, length), reader, rows,
                             np.arange(bags + 1, dtype=np.int64) * length, args)
        for entries in sorted({100000, words}):
            in_order = torch.arange(entries, dtype=torch.int32, device='cuda') if entries == words else \
                torch.sort(torch.randint(0, words, (entries,), device='cuda', generator=generator, dtype=torch.int32)).values
            orders = {'key_order': in_order,
                      'shuffled': in_order[torch.randperm(entries, device='cuda', generator=generator)].contiguous()}
            for order, rows in orders.items():
                for mean_length in lengths:
                    name = '{}_{}_{}_bags_of_{}'.format(label, entries, order, mean_length)
                    offsets = bag_offsets(entries, mean_length, mean_length)
                    if args.reduction:
                        report_reduction(results, name, reader, rows, offsets, args)
                        continue
                    if args.missing == 'skip':
                        for share in (float(share) for share in args.missing_share.split(',')):
                            shared = '{}_missing_{:g}'.format(name, share)
                            results[shared] = measure_skip(reader, rows, offsets, args.rounds, args.reps, share, mean_length)
                            summary = results[shared]['summary']
                            print('{:60s} skip {:.4f} ms  A/A {:.1%}  compact + pool {:.4f} ms (x{:.2f})  zero {:.4f} ms (x{:.3f})'.format(
                                shared, summary['skip_ms'], summary['aa_spread'], summary['compact_then_pool_ms'],
                                1 / summary['skip_over_compact'], summary['zero_ms'], summary['skip_over_zero']), flush=True)
                            if args.out:
                                with open(args.out, 'w') as f:
                                    json.dump(results, f, indent=1)
                        continue
                    if args.dtype != 'float32':
                        results[name] = measure_narrow(reader, rows, offsets, args.rounds, args.reps, args.dtype)
                        summary = results[name]['summary']
                        print('{:48s} {} {:.4f} ms  A/A {:.1%}  fp32 + cast {:.4f} ms  fp32 {:.4f} ms  bytes x{:.3f}  {:.3f} of 8 TB/s'.format(
                            name, args.dtype, summary['pooled_ms'], summary['aa_spread'], summary['fp32_then_cast_ms'], summary['fp32_ms'],
                            summary['bytes_ratio'], summary['frac_of_8TBps']), flush=True)
                        if args.out:
                            with open(args.out, 'w') as f:
                                json.dump(results, f, indent=1)
                        continue
                    results[name] = measure(reader, rows, offsets, args.rounds, args.reps)
                    summary = results[name]['summary']
                    print('{:48s} pooled {:.4f} ms  A/A {:.1%}  two-step {:.4f} ms  x{:.2f}  {:.0f} B/entry  {:.3f} of 8 TB/s'.format(
                        name, summary['pooled_ms'], summary['aa_spread'], summary['two_step_ms'], summary['speedup'],
                        summary['bytes_per_entry'], summary['frac_of_8TBps']), flush=True)
                    if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                        with open(args.out, 'w') as f:
                            json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
