"""Times the TSC-diffusion reverse process at batch 1 on the GPU: the eager `predict_tsc` against the graph-replayed
`GraphedTSCSampler`, at a 2 s and a 10 s clip, on the 6-step (fast) and the 50-step schedule.

    python tools/bench_sampler.py [--out profiles/sampler.json] [--utts 5] [--warmup 2]

Milliseconds per utterance from HIP events around --utts utterances (each one ends with its copy to the host, as a caller sees it),
after --warmup utterances; the host wall clock of the same span next to it.  The first use of a length bucket (two eager warm-up
steps + the capture of one reverse step) is timed separately with the host clock.  One JSON line on stdout, the same record in --out."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def per_utterance(fn, utts, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(utts):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return {'ms_per_utt_events': e0.elapsed_time(e1) / utts, 'ms_per_utt_host': (time.perf_counter() - t0) * 1e3 / utts, 'utts': utts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sampler.json'))
    ap.add_argument('--utts', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sampler needs a GPU: timings taken anywhere else say nothing')
    if a.utts < 5:
        raise SystemExit('--utts: at least 5 utterances per measurement')
    import __graft_entry__
    __graft_entry__.build()
    import formula
    import speech_enhancement_amd as S
    cfg = types.SimpleNamespace(NOISE_SCHEDULE=np.linspace(1e-4, 0.035, 50).tolist(),
                                INFERENCE_NOISE_SCHEDULE=[0.0001, 0.001, 0.01, 0.05, 0.2, 0.35], N_FFT=400, HOP_SAMPLES=100)
    args = types.SimpleNamespace(comp_type='pow')
    model = S.TSCNetDiffusion(64, 201, cfg.NOISE_SCHEDULE)
    model.load_state_dict(formula.tsc_state())
    model.cuda().eval()
    rs = np.random.RandomState(0)
    res = {'device': torch.cuda.get_device_name(0), 'batch': 1, 'warmup_utts': a.warmup}
    for fast in (True, False):
        sched = S.inference_schedule(cfg, fast_sampling=fast)
        steps = len(sched[0])
        for seconds in (2, 10):
            x = (0.1 * rs.randn(16000 * seconds - 37)).astype(np.float32)
            smp = S.GraphedTSCSampler(model, args, cfg, fast=fast)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp._bucket(int(np.ceil(x.size / cfg.HOP_SAMPLES)), False)
            torch.cuda.synchronize()
            capture_ms = (time.perf_counter() - t0) * 1e3
            eager = per_utterance(lambda: S.predict_tsc(model, args, cfg, x, *sched), a.utts, a.warmup)
            graphed = per_utterance(lambda: smp(x), a.utts, a.warmup)
            res[f'steps{steps}_{seconds}s'] = {'steps': steps, 'samples': int(x.size), 'eager_predict_tsc': eager, 'graphed_sampler': graphed,
                                               'bucket_first_use_ms': capture_ms,
                                               'speedup_events': eager['ms_per_utt_events'] / graphed['ms_per_utt_events']}
            del smp
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
