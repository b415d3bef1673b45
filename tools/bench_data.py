"""Times the dataset layer (speech-enhancement_amd/data.py) on the GPU: building a DeviceDataset from a generated directory of
48 kHz wavs (decode + upload + resample), the resampling kernel alone, and one DeviceLoader batch -- plain, and with every row
remixed (data.Remix(1.0): the two launches of se_crop_gather_mix instead of the one of se_crop_gather) or mixed from a resident noise
bank (data.BankMix(bank, 1.0): se_crop_gather_bank).

    python tools/bench_data.py [--out profiles/data_loader.json] [--files 64] [--seconds 3.0] [--reps 50]

Host clock around work that ends in a device synchronise, after warm-up; median and spread over --reps calls.  One JSON line on
stdout, the same record in --out.  The *_device keys are HIP-event times of 20 back-to-back gathers divided by 20: the launches
without the host's share (row table upload, statistics download, synchronise)."""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def device_timed(fn, reps, burst=20):
    """fn enqueues one gather; events around `burst` of them, so that the event overhead is shared"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / burst)
    ts = np.array(ts)
    return {'median_ms': float(np.median(ts)), 'min_ms': float(ts.min()), 'p90_ms': float(np.percentile(ts, 90)), 'reps': reps,
            'burst': burst}


def write_corpus(root, files, seconds, sr, seed):
    rs = np.random.RandomState(seed)
    cdir, ndir = os.path.join(root, 'clean'), os.path.join(root, 'noisy')
    os.makedirs(cdir)
    os.makedirs(ndir)
    total = 0
    for k in range(files):
        n = int(sr * seconds * (0.6 + 0.8 * rs.rand()))
        t = np.arange(n) / sr
        c = 0.3 * np.sin(2 * np.pi * (120 + 10 * k) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2 * t)) + 0.01 * rs.randn(n)
        v = c + 0.05 * rs.randn(n)
        for d, x in ((cdir, c), (ndir, v)):
            with wave.open(os.path.join(d, f'p{k:04d}.wav'), 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())
        total += n
    return cdir, ndir, total


class Resident:
    """what DeviceLoader needs of a DeviceDataset, filled with noise on the device"""

    def __init__(self, files, samples):
        self.lengths = [samples] * files
        self.offsets = [samples * i for i in range(files)]
        self.clean = 0.1 * torch.randn(samples * files, device='cuda')
        self.noisy = self.clean + 0.05 * torch.randn_like(self.clean)

    def __len__(self):
        return len(self.lengths)


class ResidentBank:
    """what DeviceLoader needs of a NoiseBank, filled with noise on the device"""

    def __init__(self, files, samples):
        self.lengths = [samples] * files
        self.offsets = [samples * i for i in range(files)]
        self.total = samples * files
        self.arena = 0.05 * torch.randn(self.total, device='cuda')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'data_loader.json'))
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_data needs a GPU: timings taken anywhere else say nothing')
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import data
    res = {'device': torch.cuda.get_device_name(0), 'files': args.files, 'rate_in': 48000}
    with tempfile.TemporaryDirectory() as root:
        cdir, ndir, total = write_corpus(root, args.files, args.seconds, 48000, 0)
        data.DeviceDataset(cdir, ndir, device='cuda:0')              # warm-up: library load, taps, allocator, page cache
        builds = []
        for _ in range(3):
            t0 = time.perf_counter()
            ds = data.DeviceDataset(cdir, ndir, device='cuda:0')
            builds.append(time.perf_counter() - t0)
        res['dataset_build'] = {'seconds_median': float(np.median(builds)), 'seconds_min': float(min(builds)),
                                'input_samples_per_side': total, 'resident_bytes': ds.nbytes, 'repeats': 3}
    # the kernel alone: one ragged batch already on the device, int16 and fp32 input, 48 kHz -> 16 kHz and 44.1 kHz -> 16 kHz
    rs = np.random.RandomState(1)
    for name, sr in (('48000_to_16000', 48000), ('44100_to_16000', 44100)):
        lens = [int(sr * (1.5 + 3 * rs.rand())) for _ in range(256)]
        pcm = [torch.from_numpy(rs.randint(-20000, 20000, size=n).astype(np.int16)).cuda() for n in lens]
        for kind, xs in (('int16', pcm), ('float32', [p.float() / 32768.0 for p in pcm])):
            arena = torch.cat(xs)
            up, down = data.ratio(sr, 16000)
            y = torch.empty(sum(data.out_length(n, up, down) for n in lens), dtype=torch.float32, device='cuda')
            r = timed(lambda: data._resample_into(arena, lens, up, down, y), args.reps)
            r['input_samples'] = int(sum(lens))
            r['input_samples_per_s'] = r['input_samples'] / (r['median_ms'] * 1e-3)
            res[f'resample_{name}_{kind}'] = r
    # one batch of crops, B = 16, L = 32 000, from a resident corpus of 10 s utterances (host plan + one launch + statistics)
    ds = Resident(64, 160000)
    ld = data.DeviceLoader(ds, 16, 32000, shuffle=True)
    epoch = [0]

    def one_epoch():
        epoch[0] += 1
        ld.set_epoch(epoch[0])
        for _ in ld:
            pass
    r = timed(one_epoch, args.reps)
    res['loader_batch_B16_L32000'] = {'ms_per_batch_median': r['median_ms'] / len(ld), 'ms_per_batch_min': r['min_ms'] / len(ld),
                                      'batches_per_epoch': len(ld), 'reps': args.reps}
    files, starts = list(range(16)), [1000 * i for i in range(16)]
    res['crop_gather_launch_B16_L32000'] = timed(lambda: ld._gather(files, starts).stats(), args.reps)
    # the same point with every row remixed: noise of the next utterance at 10 dB
    mix = [((f + 1) % 64, 500 * i, 10.0) for i, f in enumerate(files)]
    lm = data.DeviceLoader(ds, 16, 32000, shuffle=True, remix=data.Remix(1.0, (0.0, 20.0)))
    res['crop_gather_mix_launch_B16_L32000'] = timed(lambda: lm._gather_mix(files, starts, mix).stats(), args.reps)

    def one_epoch_mix():
        epoch[0] += 1
        lm.set_epoch(epoch[0])
        for _ in lm:
            pass
    r = timed(one_epoch_mix, args.reps)
    res['loader_batch_remix_B16_L32000'] = {'ms_per_batch_median': r['median_ms'] / len(lm), 'ms_per_batch_min': r['min_ms'] / len(lm),
                                            'batches_per_epoch': len(lm), 'reps': args.reps}
    rows = np.array([[ds.offsets[f], ds.lengths[f], s, ds.offsets[m[0]], ds.lengths[m[0]], m[1]]
                     for f, s, m in zip(files, starts, mix)], dtype=np.int64)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).cuda()
    oc, on, st = torch.empty(16, 32000, device='cuda'), torch.empty(16, 32000, device='cuda'), torch.empty(16, 3, device='cuda')
    from speech_enhancement_amd import _lib
    import ctypes as C
    res['crop_gather_B16_L32000_device'] = device_timed(
        lambda: _lib.call('se_crop_gather', _lib.ptr(ds.clean), _lib.ptr(ds.noisy), C.c_longlong(ds.clean.numel()), _lib.ptr(rows_d),
                          C.c_int(16), C.c_int(32000), _lib.ptr(oc), _lib.ptr(on), _lib.ptr(st), _lib.stream()), args.reps)
    n = data.mix_chunks(32000)
    table = torch.from_numpy(rows.reshape(-1)).cuda()
    gain = torch.full((16,), 10.0 ** -0.5, dtype=torch.float64, device='cuda')
    buf = torch.empty(16 * n * 5 + 8, dtype=torch.float64, device='cuda')
    res['crop_gather_mix_B16_L32000_device'] = device_timed(
        lambda: _lib.call('se_crop_gather_mix', _lib.ptr(ds.clean), _lib.ptr(ds.noisy), ds.clean.numel(), _lib.ptr(table),
                          _lib.ptr(gain), 16, 32000, _lib.ptr(oc), _lib.ptr(on), _lib.ptr(buf[32 * n:]), _lib.ptr(buf[80 * n:]),
                          _lib.ptr(buf), 16 * n * 16, _lib.stream()), args.reps)
    # the same rows with the noise taken from a bank of 64 x 10 s: file f + 1 from the same starts, which never wrap here
    bank = ResidentBank(64, 160000)
    res['crop_gather_bank_B16_L32000_device'] = device_timed(
        lambda: _lib.call('se_crop_gather_bank', _lib.ptr(ds.clean), _lib.ptr(ds.noisy), ds.clean.numel(), _lib.ptr(bank.arena),
                          bank.total, _lib.ptr(table), _lib.ptr(gain), 16, 32000, _lib.ptr(oc), _lib.ptr(on), _lib.ptr(buf[32 * n:]),
                          _lib.ptr(buf[80 * n:]), _lib.ptr(buf), 16 * n * 16, _lib.stream()), args.reps)
    lb = data.DeviceLoader(ds, 16, 32000, shuffle=True, bank=data.BankMix(bank, 1.0, (0.0, 20.0)))

    def one_epoch_bank():
        epoch[0] += 1
        lb.set_epoch(epoch[0])
        for _ in lb:
            pass
    r = timed(one_epoch_bank, args.reps)
    res['loader_batch_bank_B16_L32000'] = {'ms_per_batch_median': r['median_ms'] / len(lb), 'ms_per_batch_min': r['min_ms'] / len(lb),
                                           'batches_per_epoch': len(lb), 'reps': args.reps}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
