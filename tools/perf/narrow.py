"""bf16 rows straight from the decoder against fp32 rows, on ONE Reader (one allocation), with an A/A control.

    python tools/perf/narrow.py [--rounds 6] [--reps 20] [--out FILE.json]

Per configuration and round, in an order that alternates between rounds, the mean device time (CUDA events around
`reps` launches after a warm-up) of
    fp32       rows_embedding_device(rows, out=fp32)                        the float path as it is
    fp32b      the same again: the A/A floor below which no difference stands
    fp32+to    the float path, then out.to(torch.bfloat16) into a preallocated tensor (a second kernel, an fp32 temporary)
    bf16       rows_embedding_device(rows, out=bf16): decode_trained_narrow / dequant_uniform_narrow
    bf16v      bf16 into a dense buffer 8 bytes past a 16-byte boundary: the same rows through the 8-byte store mode
               (OUT_VEC4) instead of the 16-byte one (OUT_FLAT) -- the store-width comparison of DESIGN.md section 5.5
Configurations: the 2 196 017 x 300 4-bit dump in key order and shuffled, 100 000 random rows of it (BASELINE
configs[1]) and the 500 000-word uniform 8-bit dump. Reports medians over rounds, and for the headline dump the fraction
of 8 TB/s the bytes per word (row metadata + output + Huffman stream) stand for.
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
    n = rows.numel()
    dim = reader.dim
    fp32 = torch.empty((n, dim), dtype=torch.float32, device='cuda')
    bf16 = torch.empty((n, dim), dtype=torch.bfloat16, device='cuda')
    converted = torch.empty_like(bf16)
    shifted = torch.empty((n * dim + 8,), dtype=torch.bfloat16, device='cuda')[4:4 + n * dim].view(n, dim)   # 8 B past 16
    variants = {
        'fp32': lambda: reader.rows_embedding_device(rows, out=fp32),
        'fp32b': lambda: reader.rows_embedding_device(rows, out=fp32),
        'fp32+to': lambda: converted.copy_(reader.rows_embedding_device(rows, out=fp32)),
        'bf16': lambda: reader.rows_embedding_device(rows, out=bf16),
        'bf16v': lambda: reader.rows_embedding_device(rows, out=shifted),
    }
    for call in variants.values():
        call()
    torch.cuda.synchronize()
    # the outputs agree before anything is timed
    assert torch.equal(bf16.view(torch.int16), fp32.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(shifted.view(torch.int16), bf16.view(torch.int16))
    times = {name: [] for name in variants}
    names = list(variants)
    for round_ in range(rounds):
        for name in (names if round_ % 2 == 0 else names[::-1]):
            times[name].append(timed(variants[name], reps))
    return {name: {'median_ms': float(np.median(values)), 'ms': values} for name, values in times.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=6)
    parser.add_argument('--reps', type=int, default=20)
    parser.add_argument('--words', type=int, default=2196017)
    parser.add_argument('--out', default='')
    args = parser.parse_args()
    if not torch.cuda.is_available() or memb_amd.hip_device_count() < 1:
        raise SystemExit('narrow.py measures on a GPU; none found')
    results = {}
    path, _ = synthetic.cached_model(args.words, 300, 'trained', 4)
    reader = memb_amd.Reader(path)
    generator = torch.Generator(device='cuda').manual_seed(1)
    dump = torch.arange(args.words, dtype=torch.int32, device='cuda')
    cases = {
        'dump_4bit_key_order': dump,
        'dump_4bit_shuffled': dump[torch.randperm(args.words, device='cuda', generator=generator)].contiguous(),
        'random_100k_4bit': torch.randint(0, args.words, (100000,), device='cuda', generator=generator, dtype=torch.int32),
    }
    for name, rows in cases.items():
        results[name] = measure(reader, rows, args.rounds, args.reps)
        print(name, {k: round(v['median_ms'], 4) for k, v in results[name].items()}, flush=True)
    # bytes per word of the headline dump: 8 B of row metadata, the output, the Huffman stream
    info = reader.info(args.words)
    stream_bytes = reader.info()['device_bytes'] / args.words   # (upper bound: streams, index and tables over the words)
    for label, out_bytes in (('fp32', 4), ('bf16', 2)):
        per_word = 8 + 300 * out_bytes + 131
        seconds = results['dump_4bit_key_order'][label]['median_ms'] / 1e3
        results['dump_4bit_key_order'][label]['bytes_per_word'] = per_word
        results['dump_4bit_key_order'][label]['frac_of_8TBps'] = per_word * args.words / seconds / HBM_BYTES_PER_S
    results['dump_4bit_key_order']['info'] = {'waves_per_block': info['waves_per_block'], 'device_bytes_per_word': stream_bytes}
    del reader, cases, dump
    torch.cuda.empty_cache()
    path, _ = synthetic.cached_model(500000, 300, 'uniform', 8)
    uniform = memb_amd.Reader(path)
    rows = torch.arange(500000, dtype=torch.int32, device='cuda')
    results['dump_uniform_8bit_500k'] = measure(uniform, rows, args.rounds, args.reps)
    print('dump_uniform_8bit_500k', {k: round(v['median_ms'], 4) for k, v in results['dump_uniform_8bit_500k'].items()}, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
