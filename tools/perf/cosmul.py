"""cosmul_topk_device against what a caller had before it on ONE Reader -- the cosine matrix of the terms slice after slice,
the 3CosMul formula in torch elementwise operations, dense_topk_excluding_to_device --, with A/A controls, and cosmul_scores
alone as a share of the HBM peak. The method of tools/perf/analogies.py.

    python tools/perf/cosmul.py [--rounds 5] [--reps 10] [--words 2196017] [--out FILE.json] [--questions 1,16,64] [--ks 10,64]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around `reps`
calls after a warm-up) of
    fused           cosmul_topk_device(terms, offsets, negatives_from, None, k, exclude=lists, workspace=the recommended one,
                    allocated once)
    fusedb          the same again: the A/A spread below which no difference stands
    torch           the baseline, over slices as wide as the fused call's in temporaries allocated once:
                    similarity_matrix_device of the terms, ((1 + c) / 2) multiplied out and divided in torch,
                    dense_topk_excluding_to_device with merge. Checked against the call before anything is timed: equal
                    positions, values within (2 T + 2) * 2^-23 relative (torch's operation order is its own)
Configurations on the 4-bit trained model of `words` words, every word a candidate: Q in {1, 16, 64} questions of three
terms (rows of the model: two positive, one negative, as in analogy(a, b, c)), k in {10, 64}, each question's three words
excluded. Reports medians over rounds and whether the expectation holds: no slower than the baseline by more than the A/A
spread plus 5 %. Then cosmul_scores alone over a (3 Q, words) matrix: (3 + 1) * 4 bytes per element against HBM_PEAK.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import memb_amd
from memb_amd import _memb, _memb_cosmul, synthetic

TERMS = 3
MARGIN = 0.05
HBM_PEAK = 8.0e12   # bytes per second, the MI355X's specification


def timed(call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def questions(count):
    offsets = np.arange(count + 1, dtype=np.int64) * TERMS
    return offsets, offsets[:-1] + 2


def measure(reader, term_rows, k, rounds, reps):
    count, n = term_rows.numel() // TERMS, len(reader)
    offsets, negatives_from = questions(count)
    terms = reader.unit_rows_embedding_device(term_rows)
    lists = term_rows.to(torch.int64).view(count, TERMS).contiguous()
    everything = reader._all_rows_device(torch, 0)
    needed = _memb_cosmul.query_cosmul_workspace_bytes(reader._impl.context_handle(), TERMS * count, count, n, k)
    workspace = torch.empty((needed,), dtype=torch.uint8, device='cuda')
    width = min(n, (32 << 20) // (4 * (TERMS + 1) * count) // 64 * 64)
    cosines = torch.empty((TERMS * count, width), dtype=torch.float32, device='cuda')
    scores = torch.empty((count, width), dtype=torch.float32, device='cuda')
    list_bytes = max(_memb.dense_topk_workspace_bytes(count, size, k) for size in {width, n % width or width})
    segment_lists = torch.empty((list_bytes,), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    kept = {}

    def fused():
        kept['fused'] = reader.cosmul_topk_device(terms, offsets, negatives_from, None, k, exclude=lists, workspace=workspace)

    def baseline():
        values = torch.empty((count, k), dtype=torch.float32, device='cuda')
        positions = torch.empty((count, k), dtype=torch.int64, device='cuda')
        for start in range(0, n, width):
            size = min(n, start + width) - start
            reader.similarity_matrix_device(terms, everything[start:start + size], out=cosines[:, :size])
            shifted = ((1.0 + cosines[:, :size]) * 0.5).view(count, TERMS, size)
            torch.div(shifted[:, 0] * shifted[:, 1], shifted[:, 2] + 0.000001, out=scores[:, :size])
            _memb.dense_topk_excluding_to_device(
                0, scores.data_ptr(), count, size, width, start, k, start > 0, lists.data_ptr(), TERMS, TERMS, values.data_ptr(),
                positions.data_ptr(), k, segment_lists.data_ptr(), segment_lists.numel(), stream)
        kept['torch'] = (values, positions)

    variants = {'fused': fused, 'fusedb': fused, 'torch': baseline}
    for call in variants.values():
        call()
    kernel = reader.last_cosmul_kernel
    torch.cuda.synchronize()
    assert torch.equal(kept['fused'][1], kept['torch'][1]), 'the fused call and the baseline select other positions'
    assert torch.allclose(kept['fused'][0], kept['torch'][0], rtol=(2 * TERMS + 2) * 2.0 ** -23, atol=0), 'values beyond the tolerance'
    assert not (kept['fused'][1].unsqueeze(2) == lists.unsqueeze(1)).any(), 'an excluded position was returned'
    kept.clear()
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    result = {name: {'median_ms': float(np.median(series)), 'ms': series} for name, series in times.items()}
    ms = result['fused']['median_ms']
    spread = abs(result['fusedb']['median_ms'] - ms) / ms
    result['summary'] = {
        'candidates': n, 'questions': count, 'terms': TERMS * count, 'k': k, 'kernel': kernel, 'slice': width,
        'fused_ms': ms, 'aa_spread': spread, 'torch_ms': result['torch']['median_ms'], 'fused_over_torch': ms / result['torch']['median_ms'],
        'holds': ms <= result['torch']['median_ms'] * (1 + spread + MARGIN),
    }
    return result


def measure_scores(count, n, rounds, reps):
    """cosmul_scores alone over a (3 count, n) matrix of random cosines"""
    offsets, negatives_from = questions(count)
    cosines = torch.rand((TERMS * count, n), dtype=torch.float32, device='cuda') * 2 - 1
    scores = torch.empty((count, n), dtype=torch.float32, device='cuda')
    where = torch.from_numpy(np.concatenate([offsets, negatives_from]).astype(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _memb_cosmul.cosmul_scores_to_device(0, cosines.data_ptr(), n, where.data_ptr(), where[count + 1:].data_ptr(), count, n, scores.data_ptr(), n, stream)

    series = [timed(call, reps) for _ in range(rounds)]
    ms = float(np.median(series))
    moved = (TERMS + 1) * 4 * count * n
    return {'questions': count, 'columns': n, 'bytes': moved, 'median_ms': ms, 'ms': series, 'bytes_per_second': moved / (ms * 1e-3),
            'share_of_hbm_peak': moved / (ms * 1e-3) / HBM_PEAK}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--reps', type=int, default=10)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    parser.add_argument('--questions', default='1,16,64')
    parser.add_argument('--ks', default='10,64')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('cosmul.py measures on a GPU; none found')
    results = {}

    def save():
        if args.out:   # (kept up to date: a run that is cut short leaves what it measured)
            with open(args.out, 'w') as f:
                json.dump(results, f, indent=1)

    for count in (int(value) for value in args.questions.split(',')):
        name = 'cosmul_scores_{}x{}'.format(count, args.words)
        results[name] = measure_scores(count, args.words, args.rounds, args.reps)
        print('{:28s} {:.4f} ms  {:.2f} TB/s  {:.1%} of the HBM peak'.format(
            name, results[name]['median_ms'], results[name]['bytes_per_second'] / 1e12, results[name]['share_of_hbm_peak']), flush=True)
        save()
    generator = torch.Generator(device='cuda').manual_seed(1)
    path, _ = synthetic.cached_model(args.words, 300, 'trained', 4)
    reader = memb_amd.Reader(path)
    for count in (int(value) for value in args.questions.split(',')):
        term_rows = torch.randint(0, args.words, (TERMS * count,), device='cuda', generator=generator, dtype=torch.int32)
        for k in (int(value) for value in args.ks.split(',')):
            name = '4bit_{}xall_k{}'.format(count, k)
            results[name] = measure(reader, term_rows, k, args.rounds, args.reps)
            summary = results[name]['summary']
            print('{:20s} fused {:.4f} ms  A/A {:.1%} | matrix, torch and selection {:.4f} ms  x{:.3f} of it ({}) | {}'.format(
                name, summary['fused_ms'], summary['aa_spread'], summary['torch_ms'], summary['fused_over_torch'],
                'holds' if summary['holds'] else 'DOES NOT HOLD', summary['kernel']), flush=True)
            save()


if __name__ == '__main__':
    main()
