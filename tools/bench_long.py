"""Times the enhancement of long recordings on the GPU: the whole-utterance `predict` against the chunked `LongEnhancer` (4 s chunks,
0.5 s crossfade, 8 chunks per forward) at 10 s, 30 s and 60 s, and the LongEnhancer alone at 10 min.

    python tools/bench_long.py [--out profiles/long_enhance.json] [--reps 5] [--warmup 1] [--budget 90]

Randomly initialised weights (seed 0) and a seeded noise signal: the times do not depend on the values.  Per case: milliseconds per
recording as a caller sees them (host clock around a call that ends with the copy of the result to the host), the median, minimum
and maximum of --reps calls after --warmup calls; torch.cuda.max_memory_allocated over the timed calls; for the LongEnhancer the
number of chunks and of generator forwards per recording, which must be ceil(chunks / batch).  A case stops repeating once it has
used --budget seconds (at least one timed call is kept, the number taken is recorded).  A whole-utterance case that runs out of
memory, or that a kernel refuses, is recorded as such and not retried.  The record is rewritten after every case; one JSON line on
stdout at the end."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE = 16000


def timed(fn, reps, warmup, budget):
    t_begin = time.perf_counter()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                    # ends with the copy of the result to the host: the device is idle afterwards
        ms.append((time.perf_counter() - t0) * 1e3)
        if time.perf_counter() - t_begin > budget:
            break
    return {'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms), 'reps': len(ms),
            'max_memory_allocated_mb': torch.cuda.max_memory_allocated() / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'long_enhance.json'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--budget', type=float, default=90.0, help='seconds per case after which it stops repeating')
    ap.add_argument('--seconds', type=int, nargs='+', default=[10, 30, 60, 600])
    ap.add_argument('--whole-up-to', type=int, default=60, help='longest recording the whole-utterance predict is tried on')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_long needs a GPU: timings taken anywhere else say nothing')
    import __graft_entry__
    __graft_entry__.build()
    import speech_enhancement_amd as S
    cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=RATE)
    torch.manual_seed(0)
    model = S.TSCNet(64, 201)
    model.apply(S.kaiming_init)
    model.cuda().eval()
    enh = S.LongEnhancer(model, cfg)           # the defaults: 4 s chunks, 0.5 s crossfade, 8 chunks per forward
    res = {'device': torch.cuda.get_device_name(0), 'chunk_samples': enh.S, 'overlap_samples': enh.V, 'batch': enh.batch,
           'warmup_calls': a.warmup, 'weights': 'kaiming_init, seed 0', 'cases': {}}

    def record():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')

    rs = np.random.RandomState(0)
    for seconds in a.seconds:
        x = (0.1 * rs.randn(RATE * seconds - 37)).astype(np.float32)
        case = res['cases'][f'{seconds}s'] = {'samples': int(x.size)}
        chunks = len(S.chunk_plan(x.size, enh.S, enh.V))
        before = enh.forwards
        r = timed(lambda: enh(x), a.reps, a.warmup, a.budget)
        per_call = (enh.forwards - before) / (r['reps'] + a.warmup)
        want = -(-chunks // enh.batch)
        if per_call != want:
            raise SystemExit(f'{seconds} s: {per_call} forwards per recording, expected ceil({chunks} / {enh.batch}) = {want}')
        case['long_enhancer'] = dict(r, chunks=chunks, forwards=int(per_call))
        print(seconds, 's long_enhancer', case['long_enhancer'], flush=True)
        record()
        if seconds <= a.whole_up_to:
            torch.cuda.empty_cache()
            try:
                case['predict'] = timed(lambda: S.predict(model, cfg, x), a.reps, a.warmup, a.budget)
                case['long_over_predict'] = case['long_enhancer']['ms_median'] / case['predict']['ms_median']
            except torch.cuda.OutOfMemoryError as e:
                case['predict'] = {'out_of_memory': True, 'message': str(e).split('\n')[0][:200]}
            except S._lib.SeHipError as e:
                case['predict'] = {'refused': True, 'message': str(e)[:200]}
            torch.cuda.empty_cache()
            print(seconds, 's predict', case['predict'], flush=True)
            record()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
