#!/usr/bin/env python3
"""Headline benchmark: utterances/sec of the CMGAN train step (generator fwd+bwd+AdamW, discriminator 3x fwd +
bwd + AdamW, 2 STFT + 1 iSTFT fwd + 1 iSTFT bwd) on synthetic 2 s / 16 kHz clips, batch 16 per MI355X
(BASELINE.json configs[1]).  One process per GPU; N > 1 is launched by torch.distributed.run (RCCL).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times `--steps` steps and prints the headline
(`value`, `ms_per_step`, losses of the last timed step); `--dump-outputs DIR` also writes what the last timed step computed.
`--full` adds everything else, measured after the timed steps: `roofline` (HIP events around every launch of each kernel family
on extra steps), `clocks`, `secondary` configurations, and first of all `cpu_baseline`, which times the CPU oracle (a torch-CPU
port of the same step) on a bounded sample on the host cores (rank 0, N = 1 only).
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_* dense peak (== fp32 vector peak)
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA peak
PEAK_HBM_GBS = 8000.0
GFLOP_PER_UTT_STEP = 440.0        # 3 x 145.96 (G fwd+bwd) + ~1.9 (D)


def synth_batch(B, L, seed, device):
    """BASELINE.md section 2 inputs: clean = 0.1 N(0,1), noisy = clean + 0.05 N(0,1), Q ~ U(0.2, 0.9)."""
    g = torch.Generator().manual_seed(seed)
    clean = 0.1 * torch.randn(B, L, generator=g)
    noisy = clean + 0.05 * torch.randn(B, L, generator=g)
    q = 0.2 + 0.7 * torch.rand(B, generator=torch.Generator().manual_seed(seed + 1))
    return clean.to(device), noisy.to(device), q.to(device)


def _oracle_step(B, threads):
    from oracle import se_oracle as Or
    import formula
    torch.set_num_threads(threads)
    gsd, dsd = formula.formula_state('generator'), formula.formula_state('discriminator')
    clean, noisy, q = synth_batch(B, 32000, 1, 'cpu')
    t0 = time.time()
    Or.train_step(gsd, dsd, clean, noisy, q, 'cmgan', (0.1, 0.9, 0.2, 0.05), lr=5e-4)
    return time.time() - t0


try:
    _DW_TWIN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r04_dwconv_twin.json')))['inside_step']
except Exception:
    _DW_TWIN = {}


def _pipe16_parts(key):
    """16-bit MFMAs a kernel family executes per fp32-equivalent product (None: fp32 MFMA / no MFMA)"""
    if 'f16x3' in key or 'bf16x3' in key:
        return 3
    if 'bf16x6' in key:
        return 6
    return None


def _family_entry(key, v, steps, pmc):
    """one line of roofline.families: time per step + the rate against the roof that bounds the family; every scaled-fp16 /
    split-bf16 family ALSO carries frac_of_16bit_pipe (executed 16-bit MFMA rate / 2.5 PFLOP/s: the same arithmetic, one peak)"""
    e = {'ms_per_step': round(v['ms'] / steps, 3), 'launches_per_step': round(v['launches'] / steps, 2)}
    sec = v['ms'] * 1e-3
    if key in ('stft_fused', 'istft_fused'):
        # 0.64 MB per utterance and transform: latency-sized launches (0.2 % of the step); both roofs stated, neither binds
        nbytes = v['flops'] / (2.0 * 400 * 402) * (400 + 402) * 4.0          # frames x (400 samples in + 402 plane floats out)
        e.update({'tflops': round(v['flops'] / sec / 1e12, 2), 'gbs': round(nbytes / sec / 1e9, 1),
                  'frac_of_hbm_peak': round(nbytes / sec / 1e9 / PEAK_HBM_GBS, 4), 'bound': 'latency (10 MB per launch)'})
    elif v['flops'] > 0:
        tf = v['flops'] / sec / 1e12
        e['tflops'] = round(tf, 2)
        if _pipe16_parts(key):
            e['frac_of_16bit_pipe'] = round(tf * _pipe16_parts(key) / PEAK_BF16_MFMA_TFLOPS, 4)
        else:
            e['frac_of_f32_mfma'] = round(tf / PEAK_F32_MFMA_TFLOPS, 4)
    else:                                                                     # HBM-bound families: algorithmic bytes
        e.update({'gbs': round(v['bytes'] / sec / 1e9, 1), 'frac_of_hbm_peak': round(v['bytes'] / sec / 1e9 / PEAK_HBM_GBS, 3)})
    if key in _DW_TWIN:          # committed measurement of the access-pattern twin (profiles/r04_dwconv_twin.json): the structure's ceiling
        e['access_pattern_twin_gbs'] = _DW_TWIN[key]['twin_gbs']
        e['access_pattern_twin_frac_of_hbm_peak'] = round(_DW_TWIN[key]['twin_gbs'] / PEAK_HBM_GBS, 3)
        e['twin_source'] = 'profiles/r04_dwconv_twin.json (same loads / LDS staging / stores without the 31-tap FIR, inside the step)'
    p = pmc.get(key, {})
    if p.get('traffic_bytes_per_launch') is not None:
        e['traffic_bytes_per_launch_pmc'] = p['traffic_bytes_per_launch']
    if p.get('mfma_busy_pct'):
        e['mfma_busy_pct_pmc'] = p['mfma_busy_pct']
    return e


def cpu_baseline(budget_s=48.0):
    """The CPU oracle's CMGAN train step (torch-CPU port of the reference step: AdamW, PESQ labels supplied) timed on the host cores.
    Protocol (bounded so that the default run stays within minutes): (1) thread sweep 16 / 32 / 64 / 128
    (capped at the host's cores, and at OMP_NUM_THREADS when set) on a generator-only forward, stopped at the first count that
    is slower than the best (torch-CPU oversubscribes a 256-core host: on the round-6 box 16 threads 3.7 s, 64 5.3 s, 128 10.1 s
    -- the sweep says so in two forwards instead of spending the budget proving it); (2) at the best count: 3 warm-up + 5 timed
    batch-2 steps, fewer when the budget runs out (what ran is stated); (3) one batch-16 step if the measured batch-2 rate says it
    fits 30 s.  `reference_in_build_container`: the IMPORTED reference's own train_gan at the same
    protocol, measured in the build container (tools/time_reference_cpu.py; the reference cannot travel to this box)."""
    from oracle import se_oracle as Or
    import formula
    ncpu = os.cpu_count() or 1
    cap = min(ncpu, int(os.environ.get('OMP_NUM_THREADS') or ncpu))     # the process's thread allowance, when one is set
    gsd = formula.formula_state('generator')
    clean, noisy, _ = synth_batch(2, 32000, 1, 'cpu')
    cn, nn_, _c = Or.normalize_pair(clean, noisy)
    spec = Or.compressed_stft(nn_)
    sweep = {}
    t_start = time.time()
    best = None
    torch.set_num_threads(min(cap, 16))
    with torch.no_grad():
        Or.tscnet_forward(gsd, spec, False)                  # warm once (allocator, thread pool)
    stop = False
    for th in sorted({min(cap, v) for v in (16, 32, 64, 128)}):
        if stop:
            sweep[th] = None                                 # skipped: an earlier count was already slower than the best
            continue
        torch.set_num_threads(th)
        with torch.no_grad():
            t0 = time.time()
            Or.tscnet_forward(gsd, spec, False)
        sweep[th] = round(time.time() - t0, 3)
        stop = best is not None and sweep[th] > sweep[best]
        best = th if best is None or sweep[th] < sweep[best] else best
    threads = best
    warm = []
    while len(warm) < 3 and (not warm or (time.time() - t_start) + (8 - len(warm)) * warm[-1] < budget_s):
        warm.append(_oracle_step(2, threads))                # fewer warm-ups when 3 + 5 steps do not fit the budget
    times = []
    while len(times) < 5 and (not times or (time.time() - t_start) + times[-1] < budget_s):
        times.append(_oracle_step(2, threads))
    dt = sum(times) / len(times)
    res = {'value': round(2.0 / dt, 4), 'unit': 'utterances/sec', 'cores': threads, 'host_cores': ncpu, 'kind': 'port',
           'thread_sweep_forward_s': {str(k): v for k, v in sweep.items()},
           'sample': f'CMGAN train step of the CPU oracle (torch-CPU port of the reference step), batch 2, 2 s clips, '
                     f'AdamW, PESQ labels supplied: {len(warm)} warm-up ({", ".join("%.1f" % x for x in warm)} s) + {len(times)} timed steps '
                     f'({", ".join("%.1f" % x for x in times)} s) on {threads} threads (the best of the forward-only sweep; '
                     f'null = skipped, the previous count was already slower than the best)'}
    if os.environ.get('SE_CPU_BASELINE_B16') == '1':      # opt-in only: one batch-16 oracle step took 97 s on the round-5 driver box
        t16 = _oracle_step(16, threads)
        res['batch16'] = {'value': round(16.0 / t16, 4), 'seconds': round(t16, 1)}
    else:
        res['batch16'] = None
        res['batch16_note'] = ('not run (SE_CPU_BASELINE_B16=1 runs it): measured once on the round-5 driver box (BENCH_r05.json): 97.3 s '
                               'per batch-16 step = 0.1645 utterances/s, 2.8x slower per clip than batch 2 on the same host')
    try:
        rp = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r05_reference_cpu_build_container.json')
        res['reference_in_build_container'] = json.load(open(rp))
    except Exception:
        res['reference_in_build_container'] = None
    return res


class ClockSampler:
    """shader clock and board power of this rank's GPU, sampled from sysfs on a host thread during the timed loop (20 Hz): the
    boxes of the pool differ by up to 5 % at identical code -- with the clock in the line an A/B across rounds can be normalised.
    Sources: /sys/class/drm/card*/device/pp_dpm_sclk (the level marked '*') and hwmon power1_average / power1_input (microwatts);
    the card is matched by PCI address when torch reports one, else the first amdgpu card that exposes both.  Everything is
    best-effort: unreadable files leave nulls, never an exception."""

    def __init__(self, dev_index):
        import glob
        self.samples, self.stop_flag, self.thread = [], False, None
        self.sclk_path = self.power_path = self.card = None
        want = None
        try:
            pr = torch.cuda.get_device_properties(dev_index)
            if hasattr(pr, 'pci_bus_id'):
                want = f'{getattr(pr, "pci_domain_id", 0):04x}:{pr.pci_bus_id:02x}:{getattr(pr, "pci_device_id", 0):02x}'
        except Exception:
            pass
        cards = []
        for c in sorted(glob.glob('/sys/class/drm/card[0-9]*/device')):
            if not os.path.exists(os.path.join(c, 'pp_dpm_sclk')):
                continue
            pw = [q for h in glob.glob(os.path.join(c, 'hwmon', 'hwmon*')) for q in (os.path.join(h, 'power1_average'), os.path.join(h, 'power1_input'))
                  if os.path.exists(q)]
            cards.append((os.path.realpath(c), os.path.join(c, 'pp_dpm_sclk'), pw[0] if pw else None))
        pick = [c for c in cards if want and os.path.basename(c[0]).startswith(want)] or cards[dev_index:dev_index + 1] or cards[:1]
        if pick:
            self.card, self.sclk_path, self.power_path = pick[0]

    def _read(self):
        mhz = watts = None
        try:
            for line in open(self.sclk_path):
                if '*' in line:
                    mhz = float(line.split(':')[1].lower().replace('mhz', '').replace('*', '').strip())
        except Exception:
            pass
        try:
            watts = float(open(self.power_path).read()) / 1e6
        except Exception:
            pass
        return mhz, watts

    def start(self):
        import threading
        if self.sclk_path is None:
            return
        self.samples, self.stop_flag = [], False

        def run():
            while not self.stop_flag:
                self.samples.append(self._read())
                time.sleep(0.05)
        self.thread = threading.Thread(target=run, daemon=True)
        self.thread.start()

    def stop(self):
        self.stop_flag = True
        if self.thread is not None:
            self.thread.join(timeout=1.0)
        ck = [m for m, _ in self.samples if m is not None]
        pw = [w for _, w in self.samples if w is not None]
        st = lambda v: {'mean': round(sum(v) / len(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)} if v else None
        return {'sclk_mhz': st(ck), 'power_w': st(pw), 'samples': len(self.samples), 'card': os.path.basename(self.card) if self.card else None,
                'source': 'sysfs pp_dpm_sclk (active level) / hwmon power1_average, 20 Hz host thread over an untimed pass of the same steps right after the timed loop; the in-kernel clock '
                          'of an MFMA-dense kernel reads up to ~10 % below pp_dpm_sclk (MI355X_MICROARCH.md, DVFS)'}


def state_checksums(G, D, og, od):
    """two wrapping 64-bit sums (plain and position-weighted) over the BIT PATTERNS of every flat parameter buffer of both models
    and of the BatchNorm running statistics: data-parallel ranks must hold identical values after any number of steps"""
    parts = [g['flat'] for o in (og, od) for g in o.param_groups]
    parts += [b.detach().reshape(-1).float() for m in (G, D) for b in m.buffers() if b.dtype.is_floating_point]
    out = []
    for t in parts:
        v = t.contiguous().view(torch.int32).to(torch.int64)
        w = torch.arange(1, v.numel() + 1, device=v.device, dtype=torch.int64)
        out += [v.sum(), (v * w).sum()]
    return torch.stack(out)


def secondary_configs(G, D, og, od, dev, budget_s=25.0):
    """BASELINE configs 3 / 4 / 5 witnessed in the same process after the headline loop (bounded: ~25 s): the per-rank share of the
    scp recipe (batch 8), the 10 s batch-1 HIP-graph replay, the CDiffuSE sampler at batch 32.  Each entry is independent; a failure
    is reported as an `error` string, never raised (the headline line must survive it)."""
    import numpy as np
    import speech_enhancement_amd as S
    from speech_enhancement_amd import train as TR, inference as INF
    res = {}
    t_all = time.time()

    def timed(fn, warm, n):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.time() - t0) / n
    try:        # config 3, per-rank share: scp recipe (self-correcting + consistency), batch 8 per GPU
        c8, n8, q8 = synth_batch(8, 32000, 5, dev)
        lab = {'est': q8, 'clean': torch.full_like(q8, 0.97), 'noisy': q8 * 0.5}
        dt = timed(lambda: TR.gan_step(G, D, og, od, c8, n8, 'scp', (0.3, 0.7, 0.2, 0.05), labels=lab), 2, 8)
        res['config3_scp_per_rank_step'] = {'workload': 'scp generator+discriminator train step (adaptive-weighted discriminator, consistency path), batch 8 '
                                                        '= the per-rank share of batch 64 over 8 GPUs; no exchange (1 rank)',
                                            'ms_per_step': round(dt * 1e3, 2), 'utterances_per_sec': round(8 / dt, 1), 'steps': 8, 'warmup': 2}
    except Exception as e:      # noqa: BLE001
        res['config3_scp_per_rank_step'] = {'error': repr(e)[:300]}
    try:        # config 4: batch-1 inference of a 10 s utterance, whole pipeline replayed from one HIP graph
        cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100)
        was_training = G.training
        G.eval()
        x = (0.1 * np.random.RandomState(0).randn(160000)).astype(np.float32)
        enh = INF.GraphedEnhancer(G, cfg, 160000, device=dev)
        dt = timed(lambda: enh(x), 2, 10)
        res['config4_10s_graph_replay'] = {'workload': 'inference_gan predict on one 10 s @ 16 kHz utterance (T = 1601), STFT + generator + iSTFT captured '
                                                       'in one HIP graph; host copy in / out included', 'ms_per_utterance': round(dt * 1e3, 2),
                                           'realtime_factor': round(10.0 / dt, 1), 'replays': 10}
        del enh
        G.train(was_training)
    except Exception as e:      # noqa: BLE001
        G.train(True)
        res['config4_10s_graph_replay'] = {'error': repr(e)[:300]}
    try:        # config 5: CDiffuSE 50-step supportive reverse diffusion, batch 32
        if time.time() - t_all > budget_s:
            raise RuntimeError('secondary budget used up before config 5')
        sched_tr = np.linspace(1e-4, 0.035, 50).tolist()
        cfg5 = types.SimpleNamespace(NOISE_SCHEDULE=sched_tr, INFERENCE_NOISE_SCHEDULE=[0.0001, 0.001, 0.01, 0.05, 0.2, 0.35], N_FFT=400, HOP_SAMPLES=100)
        m = S.DiffuSE(10, 100, 201, sched_tr, 64, 30).to(dev).eval()
        torch.nn.init.normal_(m.output_projection.weight, std=0.05)
        x32 = (0.1 * torch.randn(32, 32000, generator=torch.Generator().manual_seed(3))).numpy()
        sched = S.inference_schedule(cfg5, fast_sampling=False)
        S.predict_diffuse(m, cfg5, x32[:2], *sched)          # warm-up (LDS attributes, plans)
        torch.cuda.synchronize()
        t0 = time.time()
        S.predict_diffuse(m, cfg5, x32, *sched, streams=2)
        torch.cuda.synchronize()
        dt = time.time() - t0
        res['config5_cdiffuse_sampler'] = {'workload': 'CDiffuSE (30 layers, 64 channels) 50-step supportive reverse diffusion, batch 32 x 2 s clips, conditioner '
                                                       'projections computed once per batch', 'utterances_per_sec': round(32 / dt, 2),
                                           'seconds_per_batch': round(dt, 3), 'ms_per_reverse_step': round(dt / 50 * 1e3, 2)}
        del m
    except Exception as e:      # noqa: BLE001
        res['config5_cdiffuse_sampler'] = {'error': repr(e)[:300]}
    try:        # the front-end at a size where its launches are not latency: batch 256 (168 MB of algorithmic traffic per transform)
        from speech_enhancement_amd import frontend as FE
        Bs = 256
        xs = 0.1 * torch.randn(Bs, 32000, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
        pl, _ = FE.stft_planes(xs, 400, 100, 'pow', padded=False)

        def ev_time(fn, n=10):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(n))[n // 2] * 1e-3
        with torch.no_grad():
            t_st = ev_time(lambda: FE.stft_planes(xs, 400, 100, 'pow', padded=False))
            t_is = ev_time(lambda: FE.istft_planes(pl, 400, 100, 'pow'))
        alg = 0.644e6 * Bs                                  # 0.128 MB in + 0.516 MB out (complex64) per utterance and transform
        moved_st = 4.0 * Bs * (32000 + 321 * 201 * 4)       # what the kernel moves: the plane format writes 16 B per bin (|z|, Re, Im, 0)
        res['frontend_at_batch256'] = {
            'workload': 'se_stft_fused / se_istft_fused (n_fft 400, hop 100, pow compression) on 256 clips of 2 s: one launch each, HIP-event median of 10',
            'stft_ms': round(t_st * 1e3, 4), 'istft_ms': round(t_is * 1e3, 4),
            'stft_fused.frac_of_hbm_peak_at_B256': round(alg / t_st / 1e9 / PEAK_HBM_GBS, 4),
            'istft_fused.frac_of_hbm_peak_at_B256': round(alg / t_is / 1e9 / PEAK_HBM_GBS, 4),
            'stft_gbs_algorithmic': round(alg / t_st / 1e9, 1), 'istft_gbs_algorithmic': round(alg / t_is / 1e9, 1),
            'stft_gbs_moved (16-byte plane pixels)': round(moved_st / t_st / 1e9, 1), 'istft_gbs_moved': round(moved_st / t_is / 1e9, 1),
            'stft_tflops_fp32_mfma': round(2.0 * Bs * 321 * 400 * 402 / t_st / 1e12, 2),
            'note': 'algorithmic bytes = SURVEY 8(d) (0.644 MB per utterance and transform) against the 8 TB/s spec; the transform is a '
                    '[400 x 402] fp32-MFMA DFT per frame (0.10 GFLOP per utterance): at this size the fp32 matrix pipe, not HBM, bounds it'}
        del xs, pl
    except Exception as e:      # noqa: BLE001
        res['frontend_at_batch256'] = {'error': repr(e)[:300]}
    res['seconds_total'] = round(time.time() - t_all, 1)
    return res


def dump_outputs(path, out, models, optimizers):
    """what the caller of the train step holds after its last call, as <path>/<name>.npy: every loss term (float64 scalar), the
    parameters after the optimizer updates (the optimizers' flat fp32 buffers) and the floating-point buffers of each model
    (BatchNorm running statistics, spectral-norm vectors); 8 MB in all at the default size"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for k, v in out.items():
        if hasattr(v, 'item') or isinstance(v, float):
            np.save(os.path.join(path, f'{k}.npy'), np.array(float(v), dtype=np.float64))
    for name, m, o in zip(('generator', 'discriminator'), models, optimizers):
        params = torch.cat([g['flat'].reshape(-1) for g in o.param_groups])
        bufs = [b.detach().reshape(-1).float() for b in m.buffers() if b.dtype.is_floating_point]
        np.save(os.path.join(path, f'{name}_params.npy'), params.float().cpu().numpy())
        if bufs:
            np.save(os.path.join(path, f'{name}_buffers.npy'), torch.cat(bufs).cpu().numpy())


def launch_ranks(n, argv):
    """`bench.py --gpus N` without a launcher: start N ranks with torch.distributed.run as a CHILD process -- decided
    before anything in this process touches the GPU -- and hand its exit code back.  Rank 0 of the children prints the
    JSON line on the inherited stdout."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16, help='utterances per GPU per step')
    ap.add_argument('--arch', default='cmgan')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--full', action='store_true',
                    help='also measure the CPU baseline, clocks, per-kernel roofline and secondary configurations (extra runs)')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write the losses and the updated parameters of the last timed step as DIR/<name>.npy')
    a = ap.parse_args()

    if 'WORLD_SIZE' not in os.environ and a.gpus > 1:
        avail = torch.cuda.device_count()              # does not initialise the GPU
        if avail < a.gpus:
            sys.exit(f'bench.py: --gpus {a.gpus} requested but only {avail} GPU(s) are visible')
        sys.exit(launch_ranks(a.gpus, sys.argv[1:]))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != a.gpus:
        sys.exit(f'bench.py: --gpus {a.gpus} does not match WORLD_SIZE={world} set by the launcher')
    # The CPU-baseline leg needs no GPU: it runs FIRST (rank 0, N = 1 only), bounded to ~30-40 s, so that the GPU section of the
    # command is contiguous and not a sliver at the start of a CPU-dominated run.
    cpu_res = cpu_baseline() if (a.full and world == 1 and not a.no_cpu_baseline) else None
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    force_dp = os.environ.get('SE_FORCE_DP') == '1'       # exercise the RCCL hooks on a single rank (self-test)
    if world > 1 or force_dp:
        dist.init_process_group('nccl', device_id=dev)

    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    if world > 1:
        dist.barrier()
    import speech_enhancement_amd as S
    from speech_enhancement_amd import _lib, optim, train as TR

    torch.manual_seed(0)
    G, D = S.TSCNet(64, 201), S.Discriminator(16)
    G.apply(S.kaiming_init)
    D.apply(S.kaiming_init)
    G.to(dev).train()
    D.to(dev).train()
    hooks = TR.attach_data_parallel(G, D) if (world > 1 or force_dp) else None
    if hooks is not None and force_dp:
        hooks.world = 2          # take the multi-rank code paths (SyncBN exchange, grad averaging); 1 rank => x0.5 grads
    oargs = types.SimpleNamespace(optimizer='adamw', lr=5e-4, weight_decay=0.01, momentum=0.9, max_norm=0.0)
    og, od = optim.build_optimizer(oargs, G), optim.build_optimizer(oargs, D)
    weights = (0.1, 0.9, 0.2, 0.05) if a.arch in ('cmgan', 'cp') else (0.3, 0.7, 0.2, 0.05)
    B, L = a.batch, 32000
    clean, noisy, q = synth_batch(B, L, 1 + rank, dev)
    labels = {'est': q, 'clean': torch.full_like(q, 0.97), 'noisy': q * 0.5}

    def step():
        return TR.gan_step(G, D, og, od, clean, noisy, a.arch, weights, labels=labels, hooks=hooks)

    for _ in range(a.warmup):
        step()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.time()                     # the HEADLINE loop: no per-launch instrumentation (TIMER off), no host thread, exactly K steps
    for _ in range(a.steps):
        out = step()
    fence()
    dt = time.time() - t0
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)
    # the results of the last timed step are read here, before any further step (--full) changes the models
    if rank == 0:
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, out, (G, D), (og, od))
        bad = [k for k, v in out.items() if hasattr(v, 'item') and not torch.isfinite(v).all()]
        if bad:
            sys.exit(f'bench.py: non-finite loss terms after the timed steps: {bad}')
    res = {
        'metric': 'utterances/sec (2 s @16 kHz) CMGAN train step', 'value': round(world * B * a.steps / dt, 3),
        'unit': 'utterances/sec', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
        'ms_per_step': round(dt / a.steps * 1e3, 2), 'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': 'f32 (f16x3 split)', 'data': 'synthetic',
        'config': {'workload': f'{a.arch} generator+discriminator train step (main_gan.py train_gan loop body), '
                               f'batch {B}/GPU, 2 s @ 16 kHz, n_fft=400 hop=100, AdamW lr 5e-4, PESQ labels supplied, '
                               f'kaiming-init weights; fp32 results throughout: conv and token GEMMs as scaled fp16 hi/lo splits '
                               f'(3 MFMAs per product, 2^-24 relative, fp32 accumulate), attention on the same scaled fp16 splits (scales from measured operand maxima), '
                               f'everything else fp32 MFMA / fp32 VALU',
                   'global_batch': world * B, 'parallelism': f'dp{world}',
                   'effective_tflops': round(world * B * a.steps * GFLOP_PER_UTT_STEP / dt / 1e3, 2),
                   'dropout': 'generator ff/attn dropout p=0.2 on (counter-based masks in the GEMM pro/epilogues); '
                              'discriminator Dropout(0.3) on'},
        'losses': {k: round(float(v), 5) for k, v in out.items() if hasattr(v, 'item') or isinstance(v, float)},
    }
    res['dtype_note'] = ('results and accumulators fp32; MFMA-bound products evaluated as 3 fp16 MFMAs on scaled (hi, lo) fp16 operand '
                         'splits (fp32-equivalent: measured against fp64 at or below the fp32-MFMA kernels\' error, tests/test_f16x3_gpu.py)')
    # self-validation of the data-parallel run (every rank; the first N > 1 run on hardware must prove itself): after W + K steps all
    # ranks must hold bit-identical parameters and BatchNorm running statistics -- identical initial broadcast, identical averaged
    # gradients, deterministic kernels.  A mismatch fails the run instead of printing a throughput for diverged replicas.
    dp_check = None
    if world > 1 or force_dp:
        cs = state_checksums(G, D, og, od)
        ids = torch.tensor([rank, local, torch.cuda.current_device()], device=dev, dtype=torch.int64)
        if world > 1:
            allcs = [torch.empty_like(cs) for _ in range(world)]
            allid = [torch.empty_like(ids) for _ in range(world)]
            dist.all_gather(allcs, cs)
            dist.all_gather(allid, ids)
        else:
            allcs, allid = [cs], [ids]
        same = all(bool((c == allcs[0]).all()) for c in allcs)
        dp_check = {'ranks_seen': dist.get_world_size(), 'backend': dist.get_backend(),
                    'ranks': [{'rank': int(i[0]), 'local_rank': int(i[1]), 'device': int(i[2])} for i in allid],
                    'state_checksum_equal_across_ranks': same, 'checksum_words': int(cs.numel()),
                    'checksum_rank0': [int(v) for v in allcs[0][:4]],
                    'note': 'wrapping 64-bit sums (plain + position-weighted) over the bit patterns of every flat parameter buffer of both '
                            'models and the BatchNorm running statistics, all-gathered after the timed loop'}
        if not same:
            bad_ranks = [int(allid[i][0]) for i, c in enumerate(allcs) if not bool((c == allcs[0]).all())]
            sys.exit(f'bench.py: data-parallel replicas DIVERGED after {a.warmup + a.steps} steps: ranks {bad_ranks} differ from rank 0 '
                     f'(state checksums) -- the throughput of diverged replicas is not a result')
        res['data_parallel_check'] = dp_check
    if not a.full:
        if rank == 0:
            print(json.dumps(res))
        if world > 1 or force_dp:
            dist.destroy_process_group()
        return
    # shader clock / board power under the same load: a SEPARATE untimed pass of the same steps right after the timed region (the
    # sampler's sysfs reads issue SMU queries and take the GIL on rank 0 only: they do not belong inside a max-over-ranks timing)
    clock_res = None
    if rank == 0:
        clocks = ClockSampler(local)
        clocks.start()
    for _ in range(min(a.steps, 10)):
        step()
    fence()
    if rank == 0:
        clock_res = clocks.stop()
    # attribution pass 1 (all ranks: the step contains collectives): 2 more steps in the SAME concurrent stream order with two HIP
    # events around every keyed launch and, for N > 1, around the data-parallel exchanges (`comm`)
    conc_steps = 2
    if hooks is not None:
        hooks.comm_events = []
    _lib.TIMER.start()
    for _ in range(conc_steps):
        step()
    fence()
    _lib.TIMER.stop()
    comm = None
    if hooks is not None:
        evs, hooks.comm_events = hooks.comm_events, None
        per = {}
        for kind, e0, e1 in evs:
            d_ = per.setdefault(kind, [0, 0.0])
            d_[0] += 1
            d_[1] += e0.elapsed_time(e1)
        comm = {k: {'calls_per_step': v[0] // conc_steps, 'ms_per_step': round(v[1] / conc_steps, 3)} for k, v in per.items()}
        comm['note'] = ('HIP events on the stream each exchange is issued on, rank 0: generator / discriminator flat-gradient '
                        'all-reduce (issue .. completion seen by the consumer stream: overlapped with the discriminator step), '
                        'SyncBatchNorm statistic exchanges, scp gradient triple')
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    conc = _lib.TIMER.summary()          # concurrent-order pass: weight-gradient and discriminator streams on -> launches overlap
    # Per-kernel attribution: with the streams on a launch's elapsed time is not the kernel's own (kernels of three streams share
    # the machine).  The roofline object is therefore measured on 2 extra steps in SERIAL stream order right after the timed
    # region (same process, same buffers, HIP events per launch); `value` / `ms_per_step` above are the timed region's.
    from speech_enhancement_amd import gemm as _GM
    _saved = (_GM._LeafStream.enabled, TR._D_OVERLAP, _GM.branch_stream.enabled)
    a_steps = a.steps
    serial_steps = 2 if (world == 1 and not force_dp) else 0      # N > 1: the other ranks have left; attribution from the timed region
    if not any(_saved):
        serial_steps = 0                                           # SE_NO_*_STREAM / SE_NO_D_OVERLAP: the timed region is serial already
    a = argparse.Namespace(**{**vars(a), 'steps': conc_steps})          # per-step figures below: per attribution pass
    if serial_steps:
        try:
            _GM._LeafStream.enabled, TR._D_OVERLAP, _GM.branch_stream.enabled = False, False, False
            step()
            torch.cuda.synchronize()
            _lib.TIMER.start()
            for _ in range(serial_steps):
                step()
            torch.cuda.synchronize()
            _lib.TIMER.stop()
        finally:
            _GM._LeafStream.enabled, TR._D_OVERLAP, _GM.branch_stream.enabled = _saved
        summ = _lib.TIMER.summary()
        a = argparse.Namespace(**{**vars(a), 'steps': serial_steps})  # per-step figures of the roofline object: serial pass
    else:
        summ = conc
    dom = max(summ.items(), key=lambda kv: kv[1]['ms']) if summ else None
    roof = None
    if dom is not None:
        k, v = dom
        traffic = mfma_busy = traffic_source = None
        pmc = {}
        tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'pmc_traffic.json')
        if os.path.exists(tpath):      # PMC passes are separate rocprofv3 runs (tools/profile_round.sh); per launch
            pj = json.load(open(tpath))
            pmc = pj.get('kernels', {})
            ent = pmc.get(k, {})
            traffic, mfma_busy = ent.get('traffic_bytes_per_launch'), ent.get('mfma_busy_pct')
            # NOT measured in this run: read from the committed profile of the builder's profiling box (rocprofv3 --pmc cannot
            # run inside this process)
            traffic_source = 'profiles/pmc_traffic.json <- ' + str(pj.get('source', 'profiles/ (separate rocprofv3 --pmc passes)'))
        if k.startswith('gemm_k64_panel') or k.startswith('dwconv'):
            ach = v['bytes'] / (v['ms'] * 1e-3) / 1e9
            roof = {'bound': 'hbm', 'kernel': k, 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s',
                    'frac': round(ach / 8000.0, 4), 'traffic': traffic, 'traffic_source': traffic_source,
                    'note': 'algorithmic bytes (operands read once + result written once) / launch time; peak = HBM3E spec'}
        else:
            ach = v['flops'] / (v['ms'] * 1e-3) / 1e12
            if k.startswith('attn_'):
                # attention: algorithmic fp32 FLOPs of QK^T, q.E, AV (+ backward) against the fp32-MFMA peak, the bar
                # BASELINE.json's north_star names for this path (the kernels execute each 16-deep product as three 16x16x32
                # bf16 MFMAs on an exact three-way operand split: 6x the algorithmic FLOPs on the bf16 pipe)
                peak = PEAK_F32_MFMA_TFLOPS
                xparts, xkind = (3, 'three 16x16x16 fp16 MFMAs per 16-deep product on scaled (hi, lo) fp16 operands') if 'f16x3' in k else \
                                (6, 'three 16x16x32 bf16 MFMAs per 16-deep product on an exact three-way operand split')
                note = ('algorithmic fp32 FLOPs of the attention contractions (forward: QK^T, q.E, AV; backward: their nine '
                        'products) / family launch time (incl. the delta / table / dE-reduce helpers); peak = dense fp32 MFMA '
                        f'(north_star bar); executed as {xkind}: {round(ach * xparts, 1)} TFLOP/s on the 2.5 PFLOP/s 16-bit pipe')
            elif 'bf16x6' in k or 'bf16x3' in k or 'f16x3' in k:
                parts = 6 if 'bf16x6' in k else 3
                kind = 'scaled fp16 hi/lo' if 'f16x3' in k and 'bf16' not in k else 'bf16 hi/mid/lo'
                peak = PEAK_BF16_MFMA_TFLOPS / parts
                note = (f'algorithmic (fp32-equivalent) FLOPs; the kernel evaluates every product as {parts} 16-bit MFMAs '
                        f'({kind} operand split, fp32 accumulate), so its peak is the dense 16-bit MFMA peak / '
                        f'{parts} = {round(peak, 1)} TFLOP/s; executed MFMA rate = {round(ach * parts, 1)} TFLOP/s.  '
                        f'The peak is quoted at the spec clock: under this load on random operands the chip holds a lower one '
                        f'(the same launch runs 25 % faster on all-zero activations, DESIGN.md appendix)')
            else:
                peak = PEAK_F32_MFMA_TFLOPS
                note = 'algorithmic fp32 FLOPs; peak = dense fp32 MFMA (v_mfma_f32_*)'
            roof = {'bound': 'mfma', 'kernel': k, 'achieved': round(ach, 2), 'peak': round(peak, 1), 'unit': 'TFLOP/s',
                    'frac': round(ach / peak, 4), 'traffic': traffic, 'mfma_busy_pct_pmc': mfma_busy,
                    'traffic_source': traffic_source, 'note': note}
            if _pipe16_parts(k):
                roof['frac_of_16bit_pipe'] = round(ach * _pipe16_parts(k) / PEAK_BF16_MFMA_TFLOPS, 4)
        cv = conc.get(k)
        # the two bars BASELINE.json's north_star names: attention vs the fp32-MFMA peak, depthwise conv vs the HBM peak
        secondary = []
        for kk, vv in sorted(summ.items(), key=lambda kv: -kv[1]['ms']):
            if kk.startswith('attn_') and vv['flops'] > 0:
                ach2 = vv['flops'] / (vv['ms'] * 1e-3) / 1e12
                secondary.append({'bound': 'mfma', 'kernel': kk, 'achieved': round(ach2, 2), 'peak': PEAK_F32_MFMA_TFLOPS,
                                  'unit': 'TFLOP/s', 'frac': round(ach2 / PEAK_F32_MFMA_TFLOPS, 4),
                                  'launches_per_step': vv['launches'] // a.steps,
                                  'avg_launch_ms': round(vv['ms'] / vv['launches'], 4),
                                  'traffic': pmc.get(kk, {}).get('traffic_bytes_per_launch'), 'traffic_source': traffic_source,
                                  'frac_of_16bit_pipe': round(ach2 * _pipe16_parts(kk) / PEAK_BF16_MFMA_TFLOPS, 4) if _pipe16_parts(kk) else None,
                                  'mfma_busy_pct_pmc': pmc.get(kk, {}).get('mfma_busy_pct'),
                                  'note': 'algorithmic fp32 FLOPs of QK^T, q.E, AV (+ their backward) / family launch time; '
                                          'peak = dense fp32 MFMA (the bar north_star names); frac_of_16bit_pipe = the same work priced '
                                          'like conv3: executed 16-bit MFMAs (3 per product) / 2.5 PFLOP/s'})
            elif kk.startswith('conv3_') and vv['flops'] > 0:
                parts2 = 6 if 'bf16x6' in kk else 3
                ach2 = vv['flops'] / (vv['ms'] * 1e-3) / 1e12
                secondary.append({'bound': 'mfma', 'kernel': kk, 'achieved': round(ach2, 2), 'peak': round(PEAK_BF16_MFMA_TFLOPS / parts2, 1),
                                  'unit': 'TFLOP/s', 'frac': round(ach2 * parts2 / PEAK_BF16_MFMA_TFLOPS, 4),
                                  'frac_of_16bit_pipe': round(ach2 * parts2 / PEAK_BF16_MFMA_TFLOPS, 4),
                                  'launches_per_step': vv['launches'] // a.steps, 'avg_launch_ms': round(vv['ms'] / vv['launches'], 4),
                                  'traffic': pmc.get(kk, {}).get('traffic_bytes_per_launch'), 'traffic_source': traffic_source,
                                  'mfma_busy_pct_pmc': pmc.get(kk, {}).get('mfma_busy_pct'),
                                  'note': f'triple-tap convolutions (dominant kernel of rounds 1 - 2): fp32-equivalent FLOPs, {parts2} 16-bit '
                                          f'MFMAs per product; peak = 2500 / {parts2} TFLOP/s'})
            elif kk.startswith('dwconv31') and vv['bytes'] > 0:
                ach2 = vv['bytes'] / (vv['ms'] * 1e-3) / 1e9
                secondary.append({'bound': 'hbm', 'kernel': kk, 'achieved': round(ach2, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                                  'frac': round(ach2 / PEAK_HBM_GBS, 4), 'launches_per_step': vv['launches'] // a.steps,
                                  'avg_launch_ms': round(vv['ms'] / vv['launches'], 4),
                                  'traffic': pmc.get(kk, {}).get('traffic_bytes_per_launch'), 'traffic_source': traffic_source,
                                  'note': 'algorithmic bytes (input read once + output written once) / launch time; peak = HBM3E spec'})
        roof['secondary'] = secondary
        roof.update({'launches_per_step': v['launches'] // a.steps, 'avg_launch_ms': round(v['ms'] / v['launches'], 4),
                     'avg_launch_ms_concurrent_order': round(cv['ms'] / cv['launches'], 4) if cv else None,
                     'measured_on': (f'{serial_steps} extra steps in serial stream order after the timed region and after a {conc_steps}-step '
                                     f'instrumented pass in concurrent order (the headline loop itself runs un-instrumented; in '
                                     f'concurrent order the discriminator and weight-gradient streams overlap with this kernel: '
                                     f'elapsed time per launch is then not the kernel\'s own)') if serial_steps else
                                    (f'{conc_steps} instrumented steps after the timed region (serial stream order)' if not any(_saved) else
                                     f'{conc_steps} instrumented steps after the timed region (launches of the three streams overlap: '
                                     f'elapsed time per launch is not the kernel\'s own)'),
                     'share_of_step_time': round(v['ms'] / a.steps / (dt / a_steps * 1e3), 3),
                     'families': {kk: _family_entry(kk, vv, a.steps, pmc) for kk, vv in sorted(summ.items(), key=lambda kv: -kv[1]['ms'])}})
        # step-level figures of the committed profile (separate rocprofv3 passes in serial stream order; NOT measured in this run)
        if os.path.exists(tpath) and pj.get('step'):
            roof['step_profile'] = dict(pj['step'], source=traffic_source,
                                        note='time-weighted MFMA-busy over every kernel of a step and HBM-side bytes per step '
                                             '(2 FETCH_SIZE + WRITE_SIZE over all launches), from the committed PMC passes')
        roof['peak_note'] = ('peak = the 2.4 GHz dense figure of MI355X_MICROARCH.md; with the matrix pipe kept full this part sustains 1.13 - 1.18 GHz '
                             '(vector-only streams 1.52 GHz): profiles/r06_clock_density.txt, tools/micro/clock_density.hip')
    res['roofline'] = roof
    res['clocks'] = clock_res
    if comm is not None:
        res['comm'] = comm
    if world == 1 and not force_dp and os.environ.get('SE_BENCH_NO_SECONDARY') != '1' and a.arch == 'cmgan' and a.batch == 16:
        res['secondary'] = secondary_configs(G, D, og, od, dev)
    if cpu_res is not None:
        res['cpu_baseline'] = cpu_res
    print(json.dumps(res))
    if world > 1 or force_dp:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
