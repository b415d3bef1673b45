"""utils/compute_metrics.py on the device: WSS, LLR, segmental SNR and STOI as fp64 HIP kernels (csrc/se_metrics.hip), the
composite measures CSIG / CBAK / COVL, and the evaluation loop of inference_gan.py:102-127 with the enhanced audio kept on
the GPU between the generator and the metric launches.

    pesq, csig, cbak, covl, ssnr, stoi = compute_metrics(clean, enhanced, 16000, 0)

Fixed-function limits (README.md): 16 kHz signals passed as arrays / tensors -- `Fs != 16000` and `path == 1` (wav file names)
raise.  PESQ is third-party CPU arithmetic that this package does not contain: it comes from the `pesq` argument, from
`train.set_pesq_score_provider`, or from the PyPI package `pesq` when installed; without any of them `pesq` and the three
composites are nan (one warning), `ssnr` and `stoi` are still computed.  There is no CPU fallback for the measures themselves."""
import ctypes as C
import math
import warnings

import numpy as np
import torch

from . import _lib as L

META = 9                       # SE_METRIC_META (include/se_hip.h)
WIN, SKIP, NFFT, NCRIT = 480, 120, 1024, 25
ST_N, ST_HOP, ST_K, ST_J, ST_SEG = 256, 128, 512, 15, 30
ALPHA = 0.95

_CENT = [50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72,
         1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63]
_BW = [70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823,
       168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136]


def critical_band_filter(fs=16000):
    """[25, 512] Gaussian critical-band filters over the bins of the 1024-point spectrum (compute_metrics.py:98-123): centre at
    floor(f0), equal weight sums, everything below the -30 dB point zeroed"""
    half = NFFT // 2
    max_freq = fs // 2
    cent, bw = np.array(_CENT), np.array(_BW)
    floor = math.exp(-30.0 / (2.0 * 2.303))
    j = np.arange(half)
    out = np.empty((NCRIT, half))
    for i in range(NCRIT):
        f0 = (cent[i] / max_freq) * half
        b = (bw[i] / max_freq) * half
        row = np.exp(-11 * np.square((j - np.floor(f0)) / b) + (np.log(bw[0]) - np.log(bw[i])))
        out[i] = np.where(row > floor, row, 0)
    return out


def third_octave_matrix(fs=10000, n_fft=ST_K, bands=ST_J, first=150):
    """[15, 257] 0/1 matrix of the one-third octave bands (compute_metrics.py:374-414)"""
    f = np.linspace(0, fs, n_fft + 1)[:n_fft // 2 + 1]
    k = np.arange(bands)
    cf = np.power(2, k / 3) * first
    lo = np.sqrt(cf * (np.power(2, (k - 1) / 3) * first))
    hi = np.sqrt(cf * (np.power(2, (k + 1) / 3) * first))
    A = np.zeros((bands, f.size))
    for i in range(bands):
        A[i, np.argmin((f - lo[i]) ** 2):np.argmin((f - hi[i]) ** 2)] = 1
    rnk = A.sum(1)
    keep = [i for i in range(bands - 1) if rnk[i + 1] >= rnk[i] and rnk[i + 1] != 0][-1] + 2
    return A[:keep]


def resample_fir(dtype=np.float64, up=5, down=8):
    """the taps scipy.signal.resample_poly uses for 16 kHz -> 10 kHz: firwin(2 * 10 * 8 + 1, 1 / 8, window=('kaiser', 5.0)) cast to
    the dtype of the signal, then * 5 in that dtype -- in numpy (scipy is not a dependency of the package)"""
    half = 10 * max(up, down)
    m = np.arange(2 * half + 1) - half
    cutoff = 1.0 / max(up, down)
    h = cutoff * np.sinc(cutoff * m)
    h = h * (np.i0(5.0 * np.sqrt(1 - (m / half) ** 2.0)) / np.i0(5.0))
    h = (h / np.sum(h)).astype(dtype)
    h *= up
    return h


def resample_impulse(h, pos, n_in):
    """response of the resampler to a unit impulse at sample `pos` of an n_in-sample signal: out[j] = h[8 j + 80 - 5 pos]"""
    n_out = (5 * n_in + 7) // 8
    idx = 8 * np.arange(n_out) + 80 - 5 * pos
    ok = (idx >= 0) & (idx < h.size)
    return np.where(ok, h[np.clip(idx, 0, h.size - 1)], 0.0)


_HOST = None


def host_constants():
    """the constant tables of the kernels, fp64, computed once with numpy"""
    global _HOST
    if _HOST is None:
        k = np.arange(NFFT // 2)
        _HOST = {
            'window': 0.5 * (1 - np.cos(2 * math.pi * np.arange(1, WIN + 1) / (WIN + 1))),
            'twiddle': np.stack([np.cos(2 * math.pi * k / NFFT), -np.sin(2 * math.pi * k / NFFT)], -1),
            'crit_filter': critical_band_filter(),
            'thirdoct': third_octave_matrix(),
            # row 0: the taps for float32 input (exactly representable in fp64), row 1: for a pair promoted to fp64
            'fir': np.stack([resample_fir(np.float32).astype(np.float64), resample_fir(np.float64)]),
            'hann': (0.5 - 0.5 * np.cos(2 * math.pi * np.arange(ST_N + 2) / (ST_N + 1)))[1:ST_N + 1],
        }
    return _HOST


_DEV = {}


def _tables(device):
    key = (device.type, device.index)
    if key not in _DEV:
        _DEV[key] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host_constants().items()}
    return _DEV[key]


def frame_count(length):
    """int(L / 120 - 4) frames of 480 samples, skip 120"""
    return (length - WIN) // SKIP if length >= WIN else 0


def stoi_sizes(length):
    """(resampled length ceil(5 L / 8), number of frame starts arange(0, n - 256, 128))"""
    n = (5 * length + 7) // 8
    return n, max(0, (n - ST_N + ST_HOP - 1) // ST_HOP)


class _Batch:
    """B (clean, enhanced) pairs packed for the kernels"""

    def __init__(self, clean, enh, truncate):
        self.single = not isinstance(clean, (list, tuple))
        cl = [clean] if self.single else list(clean)
        en = [enh] if not isinstance(enh, (list, tuple)) else list(enh)
        if len(cl) != len(en) or not cl:
            raise ValueError('clean and enhanced must be the same number of signals')
        for t in cl + en:
            if not torch.is_tensor(t):
                raise L.SeHipError('the metric kernels take CUDA tensors: there is no CPU fallback')
        L.check_cuda(*cl, *en)
        rows, cs, es = [], [], []
        off = foff = roff = soff = 0
        for c, e in zip(cl, en):
            c, e = c.reshape(-1), e.reshape(-1)
            promote = 0
            if c.numel() != e.numel():
                if not truncate:
                    raise ValueError('Both speech signals must have the same length')
                n = min(c.numel(), e.numel())             # compute_metrics.py:39-42: both cut to the shorter one, + spacing(1)
                c, e, promote = c[:n], e[:n], 1
            n = c.numel()
            nfr = frame_count(n)
            nr, nsf = stoi_sizes(n)
            rows.append([off, n, foff, nfr, roff, nr, soff, nsf, promote])
            cs.append(c.to(torch.float32))
            es.append(e.to(torch.float32))
            off, foff, roff, soff = off + n, foff + nfr, roff + nr, soff + nsf
        self.rows = rows
        self.B = len(rows)
        self.device = cs[0].device
        self.clean = torch.cat(cs).contiguous() if self.B > 1 else cs[0].contiguous()
        self.enh = torch.cat(es).contiguous() if self.B > 1 else es[0].contiguous()
        self.meta = torch.tensor(rows, dtype=torch.int64).to(self.device, non_blocking=True)
        self.frames, self.resampled, self.sframes = foff, roff, soff
        self.tab = _tables(self.device)

    def split(self, flat, col_off, col_n):
        out = [flat[r[col_off]:r[col_off] + r[col_n]] for r in self.rows]
        return out[0] if self.single else out


def _frames(b):
    wss, llr, snr = (torch.empty(max(b.frames, 1), dtype=torch.float64, device=b.device) for _ in range(3))
    t = b.tab
    L.call('se_metric_frames', L.ptr(b.clean), L.ptr(b.enh), L.ptr(b.meta), C.c_int(b.B), C.c_int(max(r[3] for r in b.rows)),
           L.ptr(t['window']), L.ptr(t['twiddle']), L.ptr(t['crit_filter']), L.ptr(wss), L.ptr(llr), L.ptr(snr), L.stream())
    return wss, llr, snr


def _trimmed(b, wss, llr, snr):
    out = torch.empty(b.B, 3, dtype=torch.float64, device=b.device)
    L.call('se_metric_trimmed_means', L.ptr(wss), L.ptr(llr), L.ptr(snr), L.ptr(b.meta), C.c_int(b.B), L.ptr(out), L.stream())
    return out


def _stoi(b):
    """(stoi [B], d_interm [sum of frame starts], kept-frame counts [B]) on the device"""
    lib = L.lib()
    need = lib.se_metric_stoi_workspace_bytes(C.c_long(b.resampled), C.c_long(b.sframes), C.c_int(b.B))
    ws = torch.empty(need, dtype=torch.uint8, device=b.device)
    d = torch.zeros(max(b.sframes, 1), dtype=torch.float64, device=b.device)
    cnt = torch.empty(b.B, dtype=torch.int32, device=b.device)
    out = torch.empty(b.B, dtype=torch.float64, device=b.device)
    t = b.tab
    L.call('se_metric_stoi', L.ptr(b.clean), L.ptr(b.enh), L.ptr(b.meta), C.c_int(b.B), C.c_long(b.resampled), C.c_long(b.sframes),
           C.c_int(max(r[5] for r in b.rows)), C.c_int(max(r[7] for r in b.rows)), L.ptr(t['fir']), L.ptr(t['hann']),
           L.ptr(t['twiddle']), L.ptr(t['thirdoct']), L.ptr(ws), C.c_size_t(need), L.ptr(d), L.ptr(cnt), L.ptr(out), L.stream())
    return out, d, cnt


def wss(clean, enh):
    """per-frame weighted spectral slope distances (fp64, device); a list of signals gives a list of vectors"""
    b = _Batch(clean, enh, False)
    return b.split(_frames(b)[0], 2, 3)


def llr(clean, enh):
    """per-frame log-likelihood ratios of the order-16 LPC models"""
    b = _Batch(clean, enh, False)
    return b.split(_frames(b)[1], 2, 3)


def snr(clean, enh):
    """(overall SNR, per-frame segmental SNR clamped to [-10, 35]) like the reference's `snr`"""
    b = _Batch(clean, enh, False)
    seg = b.split(_frames(b)[2], 2, 3)
    overall = []
    for r in b.rows:
        c, e = b.clean[r[0]:r[0] + r[1]].double(), b.enh[r[0]:r[0] + r[1]].double()
        overall.append(10 * torch.log10(torch.sum(c * c) / torch.sum((c - e) ** 2)))
    return (overall[0], seg) if b.single else (overall, seg)


def stoi(clean, enh):
    """short-time objective intelligibility (fp64 scalar on the device; nan when fewer than 30 frames survive the silent-frame
    removal, as in the reference); a list of signals gives a tensor [B]"""
    b = _Batch(clean, enh, False)
    out = _stoi(b)[0]
    return out[0] if b.single else out


def stoi_frames(clean, enh):
    """the reference's d_interm vector(s): one value per 30-frame segment.  Reads the kept-frame counts back (one synchronisation):
    a diagnostic, not part of the evaluation loop"""
    b = _Batch(clean, enh, False)
    _, d, cnt = _stoi(b)
    out = [d[r[6]:r[6] + max(int(n) - ST_SEG, 0)] for r, n in zip(b.rows, cnt.tolist())]
    return out[0] if b.single else out


def composites(pesq, wss_dist, llr_mean, seg_snr):
    """(CSIG, CBAK, COVL) of compute_metrics.py:63-72, limited to [1, 5]; tensors of any (equal) shape"""
    csig = (3.093 - 1.029 * llr_mean + 0.603 * pesq - 0.009 * wss_dist).clamp(1, 5)
    cbak = (1.634 + 0.478 * pesq - 0.007 * wss_dist + 0.063 * seg_snr).clamp(1, 5)
    covl = (1.594 + 0.805 * pesq - 0.512 * llr_mean - 0.007 * wss_dist).clamp(1, 5)
    return csig, cbak, covl


def measures(clean, enh):
    """[B, 4] on the device: (trimmed-mean WSS, trimmed-mean LLR, mean segmental SNR, STOI) per pair; pairs of unequal lengths are
    cut to the shorter one like compute_metrics does.  No synchronisation."""
    b = _Batch(clean, enh, True)
    return torch.cat([_trimmed(b, *_frames(b)), _stoi(b)[0][:, None]], 1)


_WARNED = False


def _pesq_scores(pesq, get_pairs):
    """raw PESQ per pair as a list of floats, or None when there is no source; get_pairs() -> [(clean, enhanced) numpy arrays]"""
    global _WARNED
    if pesq is not None:
        if callable(pesq):
            return [float(pesq(c, e)) for c, e in get_pairs()]
        return [float(v) for v in np.atleast_1d(np.asarray(pesq, dtype=np.float64))]
    from . import train
    if train.have_pesq_scores():
        pairs = get_pairs()
        return [float(v) for v in train.pesq_scores([c for c, _ in pairs], [e for _, e in pairs])] if pairs else []
    if not _WARNED:
        _WARNED = True
        warnings.warn('no PESQ source (pass pesq=, call train.set_pesq_score_provider(fn) or install `pesq`): '
                      'pesq, csig, cbak and covl are nan; ssnr and stoi are computed')
    return None


def six(meas, q):
    """[N, 6] (pesq, csig, cbak, covl, ssnr, stoi) from measures() rows and raw PESQ scores [N] (nan = unknown)"""
    return torch.stack([q, *composites(q, meas[:, 0], meas[:, 1], meas[:, 2]), meas[:, 2], meas[:, 3]], 1)


def _check_fixed(Fs, path):
    if path == 1:
        raise ValueError('compute_metrics: path == 1 (wav file names) is not supported: load the signals and pass arrays or tensors')
    if Fs != 16000:
        raise ValueError(f'compute_metrics: the metric kernels are built for 16 kHz signals (got Fs = {Fs})')


def compute_metrics(clean, enh, Fs=16000, path=0, pesq=None):
    """the reference's (pesq, csig, cbak, covl, ssnr, stoi) for one pair of CUDA tensors, as Python floats"""
    _check_fixed(Fs, path)
    if not (torch.is_tensor(clean) and torch.is_tensor(enh)):
        raise L.SeHipError('the metric kernels take CUDA tensors: there is no CPU fallback')
    meas = measures(clean, enh)
    n = min(clean.numel(), enh.numel())
    q = _pesq_scores(pesq, lambda: [(clean.reshape(-1)[:n].cpu().numpy(), enh.reshape(-1)[:n].cpu().numpy())])
    qt = torch.tensor(q if q is not None else [float('nan')], dtype=torch.float64, device=meas.device)
    return tuple(six(meas, qt)[0].tolist())


@torch.no_grad()
def evaluate(model, config, pairs, pesq=None, on_enhanced=None, enhancer=None):
    """inference_gan.py:102-127: enhance every noisy signal with a GraphedEnhancer, score it against its clean signal, return
    the six sums (numpy [6]: pesq, csig, cbak, covl, ssnr, stoi).

    pairs: iterable of (noisy, clean) float arrays at 16 kHz.  The enhanced audio stays on the device: the metric launches follow
    the graph replay on the same stream, and one [6] vector crosses to the host at the end.  PESQ needs host audio: with a
    source (`pesq` callable(clean, enhanced) -> score, or a provider / the `pesq` package) each enhanced signal is copied out once
    and scored by a worker thread while the GPU goes on with the next utterance.  on_enhanced(index, device tensor): hook for
    saving; the tensor is valid until the next utterance is enhanced."""
    from concurrent.futures import ThreadPoolExecutor
    from . import train
    from .inference import GraphedEnhancer
    _check_fixed(getattr(config, 'SAMPLE_RATE', 16000), 0)
    device = next(model.parameters()).device
    enhancer = enhancer or GraphedEnhancer(model, config, device=device)
    have_pesq = callable(pesq) or (pesq is None and train.have_pesq_scores())
    rows, futures = [], []
    pool = ThreadPoolExecutor(max_workers=1) if have_pesq else None
    try:
        for i, (noisy, clean) in enumerate(pairs):
            est = enhancer.enhance_device(noisy)
            cl = torch.as_tensor(np.asarray(clean, dtype=np.float32).reshape(-1)).to(device, non_blocking=True)
            rows.append(measures(cl, est))
            if on_enhanced is not None:
                on_enhanced(i, est)
            if pool is not None:
                c_np, e_np = np.asarray(clean, dtype=np.float32).reshape(-1), est.cpu().numpy()
                n = min(c_np.size, e_np.size)
                futures.append(pool.submit(lambda c=c_np[:n], e=e_np[:n]: _pesq_scores(pesq, lambda: [(c, e)])[0]))
        if not rows:
            return np.zeros(6)
        if pool is not None:
            q = [f.result() for f in futures]
        elif pesq is not None:
            q = np.broadcast_to(np.asarray(pesq, dtype=np.float64), (len(rows),)).tolist()
        else:
            _pesq_scores(None, list)                              # the one warning
            q = [float('nan')] * len(rows)
    finally:
        if pool is not None:
            pool.shutdown()
    meas = torch.cat(rows)
    return six(meas, torch.tensor(q, dtype=torch.float64, device=meas.device)).sum(0).cpu().numpy()
