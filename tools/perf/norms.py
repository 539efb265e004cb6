"""Row norms and unit rows (row_norms_device, unit_rows_embedding_device) against the two-step paths a caller had before --
rows_embedding_device into an fp32 temporary, then a torch reduction over it -- on ONE Reader, with A/A controls.

    python tools/perf/norms.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--models 4bit,6bit,uniform_8bit_500k]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    norms           row_norms_device(rows, out=...)
    normsb          the same again: the A/A spread below which no difference stands
    two_step_norms  rows_embedding_device(rows, out=fp32), then torch.linalg.vector_norm(fp32, dim=1, out=...)
    unit            unit_rows_embedding_device(rows, out=...)
    unitb           the same again
    two_step_unit   rows_embedding_device(rows, out=fp32), then torch.nn.functional.normalize(fp32, dim=1, out=...)
    decode          rows_embedding_device(rows, out=fp32) alone: what both two-step paths start with
torch's reductions add in another order: they are there for their time only (the bits are tests/test_gpu_norms.py's).
Configurations: 100 000 rows and all `words` rows, in key order and shuffled, of the 4-bit and the 6-bit trained model of
`words` words (the fused kernels), and the same of the 500 000-word uniform model (the plain decode and the dense kernels).
Reports medians over rounds, which kernel family ran, and for the one-call paths the fraction of 8 TB/s that their
algorithmic bytes stand for (memb_hip_norms_algorithmic_bytes).
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


def measure(reader, rows, rounds, reps):
    n, dim = rows.numel(), reader.dim
    norms = torch.empty((n,), dtype=torch.float32, device='cuda')
    other_norms = torch.empty((n,), dtype=torch.float32, device='cuda')
    unit = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    fp32 = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    normalized = torch.empty((n, dim), dtype=torch.float32, device='cuda')

    def two_step_norms():
        reader.rows_embedding_device(rows, out=fp32)
        torch.linalg.vector_norm(fp32, dim=1, out=other_norms)

    def two_step_unit():
        reader.rows_embedding_device(rows, out=fp32)
        torch.nn.functional.normalize(fp32, dim=1, out=normalized)

    variants = {
        'norms': lambda: reader.row_norms_device(rows, out=norms),
        'normsb': lambda: reader.row_norms_device(rows, out=norms),
        'two_step_norms': two_step_norms,
        'unit': lambda: reader.unit_rows_embedding_device(rows, out=unit),
        'unitb': lambda: reader.unit_rows_embedding_device(rows, out=unit),
        'two_step_unit': two_step_unit,
        'decode': lambda: reader.rows_embedding_device(rows, out=fp32),
    }
    kernels = {}
    for name, call in variants.items():
        call()
        if name in ('norms', 'unit'):
            kernels[name] = reader.last_norms_kernel
    torch.cuda.synchronize()
    # the same quantity before anything is timed (another order of additions: close, not equal)
    assert torch.allclose(norms, other_norms, rtol=1e-5, atol=0) and torch.allclose(unit, normalized, rtol=1e-5, atol=1e-12)
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}
    host_rows = rows.cpu().numpy().view(np.uint32)
    norm_bytes = reader._impl.norms_algorithmic_bytes(host_rows, False, True)
    unit_bytes = reader._impl.norms_algorithmic_bytes(host_rows, True, False)
    norms_ms, unit_ms = result['norms']['median_ms'], result['unit']['median_ms']
    result['summary'] = {
        'rows': n, 'norms_kernel': kernels['norms'], 'unit_kernel': kernels['unit'],
        'norms_ms': norms_ms, 'two_step_norms_ms': result['two_step_norms']['median_ms'],
        'norms_speedup': result['two_step_norms']['median_ms'] / norms_ms,
        'norms_aa_spread': abs(result['normsb']['median_ms'] - norms_ms) / norms_ms,
        'unit_ms': unit_ms, 'two_step_unit_ms': result['two_step_unit']['median_ms'],
        'unit_speedup': result['two_step_unit']['median_ms'] / unit_ms,
        'unit_aa_spread': abs(result['unitb']['median_ms'] - unit_ms) / unit_ms,
        'decode_ms': result['decode']['median_ms'],
        'norms_bytes_per_row': norm_bytes / max(n, 1), 'unit_bytes_per_row': unit_bytes / max(n, 1),
        'norms_frac_of_8TBps': norm_bytes / (norms_ms / 1e3) / HBM_BYTES_PER_S,
        'unit_frac_of_8TBps': unit_bytes / (unit_ms / 1e3) / HBM_BYTES_PER_S,
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
        raise SystemExit('norms.py measures on a GPU; none found')
    results = {}
    generator = torch.Generator(device='cuda').manual_seed(1)
    for label, words, storage, bits in (('4bit', args.words, 'trained', 4), ('6bit', args.words, 'trained', 6),
                                        ('uniform_8bit_500k', 500000, 'uniform', 8)):
        if label not in args.models.split(','):
            continue
        path, _ = synthetic.cached_model(words, 300, storage, bits)
        reader = memb_amd.Reader(path)
        for entries in sorted({100000, words}):
            in_order = torch.arange(entries, dtype=torch.int32, device='cuda') if entries == words else \
                torch.sort(torch.randint(0, words, (entries,), device='cuda', generator=generator, dtype=torch.int32)).values
            orders = {'key_order': in_order,
                      'shuffled': in_order[torch.randperm(entries, device='cuda', generator=generator)].contiguous()}
            for order, rows in orders.items():
                name = '{}_{}_{}'.format(label, entries, order)
                results[name] = measure(reader, rows, args.rounds, args.reps)
                summary = results[name]['summary']
                print('{:36s} {:13s} {:.4f} ms  A/A {:.1%}  two-step {:.4f} ms  x{:.2f}  {:.3f} of 8 TB/s | {:12s} {:.4f} ms  A/A {:.1%}  '
                      'two-step {:.4f} ms  x{:.2f}  {:.3f} of 8 TB/s | decode {:.4f} ms'.format(
                          name, summary['norms_kernel'], summary['norms_ms'], summary['norms_aa_spread'], summary['two_step_norms_ms'],
                          summary['norms_speedup'], summary['norms_frac_of_8TBps'], summary['unit_kernel'], summary['unit_ms'],
                          summary['unit_aa_spread'], summary['two_step_unit_ms'], summary['unit_speedup'],
                          summary['unit_frac_of_8TBps'], summary['decode_ms']), flush=True)
                if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
                    with open(args.out, 'w') as f:
                        json.dump(results, f, indent=1)
        del reader
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
