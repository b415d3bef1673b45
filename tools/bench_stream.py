"""Times one step of streaming enhancement (inference.StreamEnhancer) on the GPU: `streams` 1, 4 and 16 at a window of 2 s and of 1 s,
blocks of 0.1 s, look-ahead 0.05 s, crossfade 0.01 s; the same launches issued eagerly and replayed as one HIP graph.

    python tools/bench_stream.py [--out profiles/stream_enhance.json] [--steps 40] [--reps 5] [--warmup 10]

Randomly initialised weights (seed 0) and seeded noise blocks already on the device: the times do not depend on the values.  A
timed window is --steps pushes followed by one device synchronise, on the host clock; ms per step = window / steps.  Per case
--reps windows of each kind are taken after --warmup pushes, eager and graph alternating so that both see the same neighbours on a
shared host; the median, minimum and maximum over the windows are recorded.  real_time_factor = median step time / block time:
below 1 the GPU keeps up with `streams` live streams, and 1 / real_time_factor times as many would fill it.  The algorithmic
latency (block + look-ahead + crossfade) is recorded beside it; a caller waits that long plus one step.  The library must have been
built (python __graft_entry__.py); the record is rewritten after every case; one JSON line on stdout at the end."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE = 16000


def window_ms(enh, blocks, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        enh.push(blocks[k % blocks.shape[0]])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(ms):
    return {'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms), 'windows': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_enhance.json'))
    ap.add_argument('--steps', type=int, default=40, help='pushes per timed window')
    ap.add_argument('--reps', type=int, default=5, help='timed windows per case and kind')
    ap.add_argument('--warmup', type=int, default=10, help='untimed pushes per case and kind')
    ap.add_argument('--windows', type=float, nargs='+', default=[2.0, 1.0], help='window lengths in seconds')
    ap.add_argument('--streams', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--block', type=float, default=0.1)
    ap.add_argument('--lookahead', type=float, default=0.05)
    ap.add_argument('--fade', type=float, default=0.01)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stream needs a GPU: timings taken anywhere else say nothing')
    import speech_enhancement_amd as S
    cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=RATE)
    torch.manual_seed(0)
    model = S.TSCNet(64, 201)
    model.apply(S.kaiming_init)
    model.cuda().eval()
    props = torch.cuda.get_device_properties(0)
    res = {'device': torch.cuda.get_device_name(0), 'arch': props.gcnArchName, 'compute_units': props.multi_processor_count,
           'block_seconds': a.block, 'lookahead_seconds': a.lookahead,
           'fade_seconds': a.fade, 'steps_per_window': a.steps, 'warmup_pushes': a.warmup, 'weights': 'kaiming_init, seed 0',
           'timing': 'host clock around steps_per_window pushes and one device synchronise', 'cases': {}}

    def record():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')

    gen = torch.Generator(device='cuda').manual_seed(0)
    for seconds in a.windows:
        for streams in a.streams:
            kw = dict(window_seconds=seconds, block_seconds=a.block, lookahead_seconds=a.lookahead, fade_seconds=a.fade, streams=streams)
            kinds = {'eager': S.StreamEnhancer(model, cfg, graph=False, **kw), 'graph': S.StreamEnhancer(model, cfg, graph=True, **kw)}
            enh = kinds['graph']
            blocks = 0.1 * torch.randn(8, streams, enh.H, device='cuda', generator=gen)
            for e in kinds.values():
                window_ms(e, blocks, a.warmup)
            ms = {k: [] for k in kinds}
            for _ in range(a.reps):
                for k, e in kinds.items():
                    ms[k].append(window_ms(e, blocks, a.steps))
            case = {'window_samples': enh.W, 'block_samples': enh.H, 'delay_samples': enh.delay, 'streams': streams,
                    'algorithmic_latency_ms': 1e3 * enh.latency_seconds}
            for k in kinds:
                case[k] = summary(ms[k])
                case[k]['real_time_factor'] = case[k]['ms_median'] / (1e3 * enh.H / RATE)
            case['eager_over_graph'] = case['eager']['ms_median'] / case['graph']['ms_median']
            res['cases'][f'window_{seconds:g}s_streams_{streams}'] = case
            print(f'window {seconds:g} s, {streams} streams:', case, flush=True)
            record()
            del kinds, enh
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
