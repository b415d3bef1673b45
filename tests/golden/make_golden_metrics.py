"""Golden vectors of the objective metrics: runs the reference's utils/compute_metrics.py (numpy / scipy, CPU) on seeded
synthetic (clean, enhanced) pairs and stores per-frame WSS / LLR / segmental SNR, STOI's d_interm, the final six-tuple (the
third-party PESQ replaced by a stub that returns 2.5) and the host constants as the reference and scipy produce them.

    python tests/golden/make_golden_metrics.py /path/to/reference     ->  tests/golden/golden_metrics.npz

The tolerance of the per-frame GPU tests is not taken from the code under test: the reference's own formulas are evaluated a
second time with every FFT replaced by a direct DFT and every sum taken in reversed order (the module's `np`, `fft`, `signal`
and `norm` names are swapped for proxies, its program text is used as it is), and the largest deviation per measure is stored as
reorder_dev_*; the tests allow 100 x that for the device's reduction trees.  The generator asserts that the fixture exercises
what it is meant to (clamps, the 1e-10 floor, silent-frame removal), so the tests cannot pass vacuously."""
import importlib.util
import os
import sys
import time
import types

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
FS = 16000
PESQ_STUB = 2.5
# (clean length, enhanced length, enhanced gain, SNR of the added noise in dB, gap position in s); none a multiple of 120 / 128
PAIRS = [(33331, 33331, 0.9, 12.0, 0.9), (28007, 28007, 1.05, 4.0, 0.5), (30500, 30011, 0.8, 20.0, 1.2)]


def load_reference(root):
    sys.modules['pesq'] = types.SimpleNamespace(pesq=lambda fs, ref, deg, mode: PESQ_STUB)
    spec = importlib.util.spec_from_file_location('ref_compute_metrics', os.path.join(root, 'utils', 'compute_metrics.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synth(rs, n, gap_at):
    """voiced 'speech': harmonics of a gliding pitch under a syllabic envelope, one low-level gap, a noise floor everywhere"""
    t = np.arange(n) / FS
    f0 = 130 + 40 * np.sin(2 * np.pi * 0.7 * t + rs.uniform(0, 6)) + 15 * np.sin(2 * np.pi * 2.3 * t)
    phase = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(n)
    for k in range(1, 24):
        form = np.exp(-0.5 * ((k * 150 - 600) / 500) ** 2) + 0.5 * np.exp(-0.5 * ((k * 150 - 2200) / 600) ** 2) + 0.05
        x += form / np.sqrt(k) * np.sin(k * phase + rs.uniform(0, 6))
    env = 0.25 + 0.75 * (0.5 * (1 + np.sin(2 * np.pi * 3.1 * t + rs.uniform(0, 6)))) ** 1.5
    gap = np.ones(n)
    a, b = int(gap_at * FS), int((gap_at + 0.45) * FS)
    gap[a:b] = 0.002
    x = 0.12 * x / np.abs(x).max() * 2.5 * env * gap
    return x + 1e-4 * rs.randn(n)


def make_pair(rs, nc, ne, gain, snr_db, gap_at):
    clean = synth(rs, max(nc, ne), gap_at)
    w = rs.randn(clean.size + 64)
    noise = np.convolve(w, 0.8 ** np.arange(24), mode='same')[32:32 + clean.size]           # coloured (low-pass) noise
    noise *= np.sqrt(np.mean(clean ** 2) / np.mean(noise ** 2)) * 10 ** (-snr_db / 20)
    enh = gain * clean + noise
    return clean[:nc].astype(np.float32), enh[:ne].astype(np.float32)


class _ReorderedNumpy:
    """numpy with the reductions the reference uses taken in reversed order"""

    def __init__(self):
        self.__dict__['_np'] = np

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def sum(a, axis=None, **kw):
        a = np.asarray(a)
        return np.sum(a[::-1] if axis is None and a.ndim == 1 else np.flip(a, axis), axis=axis, **kw)

    @staticmethod
    def mean(a, axis=None, **kw):
        a = np.asarray(a)
        return np.mean(np.flip(a, axis), axis=axis, **kw)

    @staticmethod
    def dot(a, b):
        return np.dot(np.asarray(a)[::-1], np.asarray(b)[::-1])

    @staticmethod
    def matmul(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return np.matmul(a[..., ::-1], b[::-1])


def _dft_matrix(n_fft, n_in):
    k = (np.arange(n_fft)[:, None] * np.arange(n_in)[None, :]) % n_fft
    return np.exp(-2j * np.pi * k / n_fft)


_DFT = {}


def direct_fft(x, n):
    x = np.asarray(x, dtype=np.float64)
    key = (n, x.size)
    if key not in _DFT:
        _DFT[key] = _dft_matrix(n, x.size)
    return _DFT[key][:, ::-1] @ x[::-1]


class _ReorderedSignal:
    windows = scipy.signal.windows

    @staticmethod
    def resample_poly(x, up, down):
        """scipy's polyphase filter (same taps, same dtype as the input), every output as a sum over descending input index"""
        assert (up, down) == (10000, 16000)
        h = scipy.signal.firwin(161, 1 / 8, window=('kaiser', 5.0)).astype(x.dtype)
        h *= 5
        n_out = -(-x.size * 5 // 8)
        top = 8 * np.arange(n_out) + 80
        acc = np.zeros(n_out, dtype=x.dtype)
        for i_rel in range(32, -33, -1):                      # input index = top // 5 + i_rel, descending
            i = top // 5 + i_rel
            t = top - 5 * i
            ok = (i >= 0) & (i < x.size) & (t >= 0) & (t <= 160)
            acc = acc + np.where(ok, x[np.clip(i, 0, x.size - 1)] * h[np.clip(t, 0, 160)], 0).astype(x.dtype)
        return acc

    @staticmethod
    def stft(x, window, nperseg, noverlap, nfft, return_onesided, boundary):
        hop = nperseg - int(noverlap)
        nseg = (x.size - nperseg) // hop + 1
        fr = np.stack([x[s * hop:s * hop + nperseg] * window for s in range(nseg)], 1)
        E = _dft_matrix(nfft, nperseg)
        return None, None, (E[:, ::-1] @ fr[::-1]) / window.sum()


def run_all(mod, clean, enh):
    """the reference's per-frame vectors, d_interm and final tuple for one pair"""
    got = {}
    orig_corr = mod.taa_corr
    dvals = []

    def spy(x, y):
        r = orig_corr(x, y)
        dvals.append(r / 15)
        return r
    mod.taa_corr = spy
    try:
        t0 = time.perf_counter()
        final = mod.compute_metrics(clean, enh, FS, 0)
        got['seconds'] = time.perf_counter() - t0
        got['dinterm'] = np.array(dvals)
        n = min(clean.size, enh.size)
        c, e = clean, enh
        if clean.size != enh.size:
            c, e = clean[:n] + np.spacing(1), enh[:n] + np.spacing(1)
        got['wss'] = mod.wss(c, e, FS)
        got['llr'] = mod.llr(c, e, FS)
        got['snr'] = mod.snr(c, e, FS)[1]
        got['final'] = np.array(final, dtype=np.float64)
    finally:
        mod.taa_corr = orig_corr
    return got


def main():
    if len(sys.argv) < 2:
        raise SystemExit('usage: make_golden_metrics.py /path/to/reference')
    root = sys.argv[1]
    mod = load_reference(root)
    rs = np.random.RandomState(20240607)
    out = {'n_pairs': np.array(len(PAIRS)), 'pesq_stub': np.array(PESQ_STUB)}
    pairs = [make_pair(rs, *p) for p in PAIRS]
    ref = [run_all(mod, c, e) for c, e in pairs]
    # the same formulas with reversed sums and direct DFTs
    saved = (mod.np, mod.fft, mod.signal, mod.norm)
    mod.np, mod.fft, mod.signal = _ReorderedNumpy(), direct_fft, _ReorderedSignal
    mod.norm = lambda a, axis=None, keepdims=False: np.sqrt(np.sum(np.flip(np.square(a), -1), axis=axis, keepdims=keepdims))
    try:
        alt = [run_all(mod, c, e) for c, e in pairs]
    finally:
        mod.np, mod.fft, mod.signal, mod.norm = saved
    dev = {k: 0.0 for k in ('wss', 'llr', 'snr', 'dinterm')}
    for r, a in zip(ref, alt):
        for k in dev:
            assert r[k].shape == a[k].shape, k
            dev[k] = max(dev[k], float(np.max(np.abs(r[k] - a[k]))))
    for k, v in dev.items():
        assert 0 < v < 1e-3, (k, v)
        out['reorder_dev_' + k] = np.array(v)
    # conditions on the fixture
    drop_ok = floor_ok = False
    for i, ((c, e), r) in enumerate(zip(pairs, ref)):
        for k in ('wss', 'llr', 'snr', 'dinterm', 'final'):
            assert np.isfinite(r[k]).all(), (i, k)
        n = min(c.size, e.size)
        assert n % 120 and n % 128 and c.size % 120 and e.size % 128
        nsf = len(np.arange(0, -(-n * 5 // 8) - 256, 128))
        kept = r['dinterm'].size + 30                         # frames_size = kept - 1, d_interm = frames_size - 29
        assert r['dinterm'].size >= 1 and kept >= 30, (i, kept)
        drop_ok |= 0.10 <= 1 - kept / nsf <= 0.60
        s = r['snr']
        lo, inside = np.sum(s == -10), np.sum((s > -10) & (s < 35))
        assert lo > 0 and inside > 0 and np.sum((s == -10) | (s == 35)) <= 0.5 * s.size, (i, lo, inside, s.size)
        # the 1e-10 floor: band energies of the reference's formulas for every frame of the clean signal
        win = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, 481) / 481))
        filt = None
        for f in range(r['wss'].size):
            fr = (c[:n][f * 120:f * 120 + 480] / 32768) * win
            spec = np.abs(np.fft.fft(fr, 1024))[:512] ** 2
            if filt is None:
                filt = crit_filter_of(mod)
            floor_ok |= bool(np.any(filt @ spec < 1e-10))
        out[f'clean_{i}'], out[f'enh_{i}'] = c, e
        for k in ('wss', 'llr', 'snr', 'dinterm', 'final'):
            out[f'{k}_{i}'] = r[k]
        out[f'ref_cpu_seconds_{i}'] = np.array(r['seconds'])
        print(i, c.size, e.size, 'frames', s.size, 'clamped', int(lo), 'stoi frames', nsf, 'kept', kept, 'final', np.round(r['final'], 4),
              f"{r['seconds']:.3f} s")
    assert drop_ok, 'silent-frame removal must drop 10-60 % of the frames in at least one pair'
    assert floor_ok, 'the 1e-10 floor must be hit in at least one WSS frame'
    # host constants as the reference and scipy produce them
    out['crit_filter'] = crit_filter_of(mod)
    out['thirdoct'] = mod.thirdoct(10000, 512, 15, 150)[0]
    imp64, imp32 = [], []
    for pos in range(20, 25):
        x = np.zeros(100)
        x[pos] = 1.0
        imp64.append(scipy.signal.resample_poly(x, 10000, 16000))
        imp32.append(scipy.signal.resample_poly(x.astype(np.float32), 10000, 16000))
    out['resample_impulse'] = np.stack(imp64)
    out['resample_impulse_f32'] = np.stack(imp32)
    assert out['resample_impulse_f32'].dtype == np.float32
    out['hann'] = scipy.signal.windows.hann(258)[1:257]
    print('reorder deviations', dev)
    path = os.path.join(HERE, 'golden_metrics.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000


def crit_filter_of(mod):
    """the reference builds its critical-band filter inside wss(): recover it as the response to unit spectra"""
    captured = {}
    real = np.matmul

    class Spy(_ReorderedNumpy):
        @staticmethod
        def matmul(a, b):
            captured.setdefault('f', np.array(a))
            return real(a, b)
    saved = mod.np
    mod.np = Spy()
    try:
        mod.wss(np.ones(600), np.ones(600), FS)
    finally:
        mod.np = saved
    return captured['f']


if __name__ == '__main__':
    main()
