"""Times the objective-metric stage (metrics.measures: WSS + LLR + segSNR + trimmed means + STOI, 8 launches) on the GPU, beside
the GraphedEnhancer replay of the same utterance in the same process: the evaluation loop stays bound by the generator as long
as the metric stage of an utterance costs less than its enhancement.

    python tools/bench_metrics.py [--out profiles/metrics_eval.json] [--reps 50]

Host clock around work that ends in a device synchronise, after warm-up of every shape; median and spread over --reps calls."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def signal_pair(seed, n):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000
    c = 0.1 * rs.randn(n) * (0.2 + 0.8 * np.sin(2 * np.pi * 1.7 * t) ** 2) + 1e-4 * rs.randn(n)
    return c.astype(np.float32), (0.9 * c + 0.02 * rs.randn(n)).astype(np.float32)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {'median_ms': float(np.median(ts)), 'min_ms': float(ts.min()), 'p90_ms': float(np.percentile(ts, 90)), 'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_eval.json'))
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics needs a GPU: timings taken anywhere else say nothing')
    import __graft_entry__
    __graft_entry__.build()
    import speech_enhancement_amd as S
    from speech_enhancement_amd import inference as INF, metrics as M
    res = {'device': torch.cuda.get_device_name(0)}
    c10, e10 = signal_pair(1, 160000)
    c, e = torch.from_numpy(c10).cuda(), torch.from_numpy(e10).cuda()
    res['metrics_10s_pair'] = timed(lambda: M.measures(c, e), args.reps)
    cs, es = zip(*[tuple(torch.from_numpy(v).cuda() for v in signal_pair(10 + i, 48000 - 37 * i)) for i in range(16)])
    res['metrics_batch16_3s'] = timed(lambda: M.measures(list(cs), list(es)), args.reps)
    res['metrics_batch16_3s']['per_utterance_ms'] = res['metrics_batch16_3s']['median_ms'] / 16
    torch.manual_seed(0)
    g = S.TSCNet(64, 201)
    g.apply(S.kaiming_init)
    g.cuda().eval()
    enh = INF.GraphedEnhancer(g, types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100), 160000)
    res['graphed_enhancer_10s'] = timed(lambda: enh.enhance_device(e10), max(10, args.reps // 2), warmup=3)
    res['enhance_plus_metrics_10s'] = timed(lambda: M.measures(c, enh.enhance_device(e10)), max(10, args.reps // 2), warmup=3)
    res['metric_stage_over_enhancement'] = res['metrics_10s_pair']['median_ms'] / res['graphed_enhancer_10s']['median_ms']
    res['accepted'] = res['metric_stage_over_enhancement'] < 1.0
    gm = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_metrics.npz'))
    res['context_reference_cpu_seconds'] = {f"{gm[f'clean_{i}'].size} samples": float(gm[f'ref_cpu_seconds_{i}']) for i in range(int(gm['n_pairs']))}
    res['context_note'] = 'reference numpy / scipy time measured on the host that generated the golden file: context, not a bar'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res['accepted']:
        raise SystemExit('the metric stage costs more than the enhancement')


if __name__ == '__main__':
    main()
