"""Training data on the device: the VoicebankDataset + Collator of datasets/voicebank_dataset.py without a loader.

    train_set = DeviceDataset(clean_dir, noisy_dir, device='cuda:0')        # decode once, resample on the GPU, keep resident
    loader = DeviceLoader(train_set, batch_size=16, crop_samples=32000, shuffle=True)
    for epoch in ...:
        loader.set_epoch(epoch)
        for batch in loader:                # {'audio': [b, L], 'noisy': [b, L], 'keys': [(file_index, start), ...]} on the device

Every wav is read once (`read_wav`), resampled to 16 kHz by a HIP kernel (`resample`, csrc/se_data.hip) and kept in two fp32
arenas; a batch of crops is one launch (`se_crop_gather`) that also returns each row's energy, which is what the loader rejects
silent crops on.  `DeviceLoader(..., remix=Remix(prob, (lo, hi)))` pairs a row's speech crop with the noise (noisy - clean) of another
utterance at a drawn SNR, in the same two-launch gather (`se_crop_gather_mix`); `bank=BankMix(NoiseBank(noise_dir), prob, (lo, hi))`
takes the noise from a separate folder of recordings instead (`se_crop_gather_bank`), which is also how a corpus of clean speech
alone, `DeviceDataset(clean_dir, None)`, is trained from.  The resampling filter is scipy.signal.resample_poly's default (Kaiser beta = 5, metrics.resample_fir), NOT
librosa's soxr_hq: the 16 kHz signals differ slightly from the ones the reference trained on.  There is no CPU fallback."""
import bisect
import ctypes as C
import glob
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib as L
from .metrics import resample_fir

MAX_RATIO = 441                 # 44.1 kHz <-> 16 kHz = 160:441 is the largest tap table the kernel stages (8 821 taps)
READ_THREADS = 8
CHUNK_SAMPLES = 1 << 25         # input samples uploaded and resampled at a time (64 MB of PCM16)
MAX_ATTEMPTS = 10               # the collator's "ten more chances"
MIX_CHUNK = 4096                # SE_MIX_CHUNK of include/se_hip.h
MAX_NOISE_SAMPLES = 2 ** 31 - 1 # the longest file of a NoiseBank: se_crop_gather_bank wraps a 32-bit index


def _scale_pcm(x):
    if x.dtype == np.int16:
        return x.astype(np.float32) / 32768.0
    if x.dtype == np.int32:
        return (x.astype(np.float64) / 2147483648.0).astype(np.float32)
    if x.dtype == np.uint8:
        return (x.astype(np.float32) - 128.0) / 128.0
    return x.astype(np.float32)


def _read_any(path):
    """(sample rate, int16 or float32 array [n] or [n, channels]) -- stdlib `wave` for 16-bit PCM, scipy.io.wavfile otherwise"""
    import wave
    try:
        with wave.open(path, 'rb') as w:
            if w.getsampwidth() == 2 and w.getcomptype() == 'NONE':
                sr, ch, n = w.getframerate(), w.getnchannels(), w.getnframes()
                x = np.frombuffer(w.readframes(n), dtype='<i2')
                return sr, (x.reshape(-1, ch) if ch > 1 else x)
    except wave.Error:
        pass                        # not plain PCM (float, extensible, ...): scipy's reader knows more formats
    try:
        from scipy.io import wavfile
    except ImportError as e:
        raise RuntimeError(f'{path}: not 16-bit PCM, and reading other wav formats needs scipy (scipy.io.wavfile)') from e
    sr, x = wavfile.read(path)
    return sr, (x if x.dtype == np.int16 else _scale_pcm(x))


def _mono(x):
    """int16 mono stays int16 (the resampler scales it on the device); anything else becomes float32, channels averaged like
    librosa.load(mono=True)"""
    if x.ndim == 1:
        return x if x.dtype == np.int16 else _scale_pcm(x)
    return _scale_pcm(x).mean(axis=1, dtype=np.float32)


def read_wav(path):
    """(sample rate, float32 signal in [-1, 1)); multi-channel files become the channel mean"""
    sr, x = _read_any(path)
    return sr, _scale_pcm(_mono(x))


def _wav_info(path):
    """(sample rate, frames) from the header where the stdlib can parse it, else from a full read"""
    import wave
    try:
        with wave.open(path, 'rb') as w:
            return w.getframerate(), w.getnframes()
    except wave.Error:
        sr, x = _read_any(path)
        return sr, x.shape[0]


def ratio(sr_in, sr_out):
    """(up, down) reduced by the gcd"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f'sample rates must be positive (got {sr_in} -> {sr_out})')
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError(f'resampling {sr_in} -> {sr_out} Hz is the ratio {up}:{down}; the kernel supports up to {MAX_RATIO}')
    return up, down


def out_length(n, up, down):
    return (n * up + down - 1) // down


_TAPS = {}


def _taps(up, down, device):
    key = (up, down, device.type, device.index)
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(resample_fir(np.float32, up, down)).to(device)
    return _TAPS[key]


def resample_tables(lengths, up, down, tile, in_offsets=None, out_offsets=None):
    """host tables of se_resample_poly: utt int64 [U][3] = (in offset, length, out offset) and tiles int32 [T][2] = (utterance,
    first output); offsets default to dense packing in list order"""
    n = np.asarray(lengths, dtype=np.int64)
    n_out = (n * up + down - 1) // down
    ino = np.concatenate([[0], np.cumsum(n)[:-1]]) if in_offsets is None else np.asarray(in_offsets, dtype=np.int64)
    outo = np.concatenate([[0], np.cumsum(n_out)[:-1]]) if out_offsets is None else np.asarray(out_offsets, dtype=np.int64)
    utt = np.stack([ino, n, outo], 1).astype(np.int64)
    per = (n_out + tile - 1) // tile
    which = np.repeat(np.arange(len(n), dtype=np.int64), per)
    first = (np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * tile
    return utt, np.stack([which, first], 1).astype(np.int32), n_out


def _resample_into(x_arena, lengths, up, down, y_arena, in_offsets=None, out_offsets=None):
    """launch the resampler for utterances packed in x_arena (int16 or fp32, device) writing into y_arena (fp32, device)"""
    L.check_cuda(x_arena, y_arena)
    if x_arena.dtype not in (torch.int16, torch.float32) or y_arena.dtype != torch.float32:
        raise L.SeHipError(f'the resampler takes int16 or float32 and writes float32 (got {x_arena.dtype} -> {y_arena.dtype})')
    if not (x_arena.is_contiguous() and y_arena.is_contiguous()):
        raise L.SeHipError('the resampler takes contiguous arenas')
    taps = _taps(up, down, x_arena.device)
    tile = L.lib().se_resample_poly_tile(C.c_int(up), C.c_int(down), C.c_int(taps.numel()))
    if tile <= 0:
        raise L.SeHipError(f'se_resample_poly has no tile size for the ratio {up}:{down}')
    utt, tiles, n_out = resample_tables(lengths, up, down, tile, in_offsets, out_offsets)
    if len(utt) == 0 or (utt[:, 1] <= 0).any():
        raise ValueError('resample: empty signal')
    if (utt[:, 0] < 0).any() or (utt[:, 0] + utt[:, 1]).max() > x_arena.numel() or (utt[:, 2] < 0).any() \
            or (utt[:, 2] + n_out).max() > y_arena.numel():
        raise L.SeHipError('resample: an utterance does not fit its arena')
    dev = x_arena.device
    utt_d = torch.from_numpy(utt).to(dev, non_blocking=True)
    tiles_d = torch.from_numpy(tiles).to(dev, non_blocking=True)
    L.call('se_resample_poly', L.ptr(x_arena), C.c_int(int(x_arena.dtype == torch.int16)), L.ptr(utt_d), C.c_int(len(utt)),
           L.ptr(tiles_d), C.c_int(len(tiles)), C.c_int(tile), L.ptr(taps), C.c_int(taps.numel()), C.c_int(up), C.c_int(down),
           L.ptr(y_arena), C.c_longlong(x_arena.numel()), C.c_longlong(y_arena.numel()), L.stream())
    return n_out


def resample(x, sr_in, sr_out):
    """x: a 1-D device tensor (int16 PCM or float32) or a list of them, resampled from sr_in to sr_out in one launch -> float32
    tensor(s).  Equal rates return the input."""
    if int(sr_in) == int(sr_out):
        return x
    up, down = ratio(sr_in, sr_out)
    single = torch.is_tensor(x)
    xs = [x] if single else list(x)
    if not xs or not all(torch.is_tensor(t) for t in xs):
        raise L.SeHipError('resample takes CUDA tensors: there is no CPU fallback')
    L.check_cuda(*xs)
    xs = [t.reshape(-1) for t in xs]
    if len({t.dtype for t in xs}) > 1 or xs[0].dtype not in (torch.int16, torch.float32):
        xs = [(t.to(torch.float32) / 32768.0 if t.dtype == torch.int16 else t.to(torch.float32)) for t in xs]
    lengths = [t.numel() for t in xs]
    arena = xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)
    n_out = [out_length(n, up, down) for n in lengths]
    y = torch.empty(sum(n_out), dtype=torch.float32, device=arena.device)
    _resample_into(arena, lengths, up, down, y)
    out = list(torch.split(y, n_out))
    return out[0] if single else out


def _load_files(layout, idx, read, paths, arena):
    """one chunk of files into `arena`: files at the target rate are copied, the others grouped by (rate, sample type) and
    resampled straight into their places.  layout: the object (DeviceDataset, NoiseBank) whose rates / raw_lengths / offsets /
    sample_rate / device say what the headers promised and where file i lives"""
    groups = {}
    for i, (sr, x) in zip(idx, read):
        x = _mono(x)
        if sr != layout.rates[i] or x.shape[0] != layout.raw_lengths[i]:
            raise ValueError(f'{paths[i]}: {x.shape[0]} samples at {sr} Hz, its header says {layout.raw_lengths[i]} at {layout.rates[i]}')
        if sr == layout.sample_rate:
            x = _scale_pcm(x)
        groups.setdefault((sr, x.dtype.str), []).append((i, x))
    for (sr, _), items in groups.items():
        host = torch.from_numpy(np.ascontiguousarray(np.concatenate([x for _, x in items])))
        if sr == layout.sample_rate:
            o = 0
            for i, x in items:
                arena[layout.offsets[i]:layout.offsets[i] + x.shape[0]].copy_(host[o:o + x.shape[0]])
                o += x.shape[0]
            continue
        up, down = ratio(sr, layout.sample_rate)
        _resample_into(host.to(layout.device), [x.shape[0] for _, x in items], up, down, arena,
                       out_offsets=[layout.offsets[i] for i, _ in items])


def _lay_out(layout, info, sides, max_bytes, what):
    """rates / raw_lengths / lengths / offsets / total / nbytes of `layout` from the headers `info` = [(rate, frames)], for `sides`
    arenas; MemoryError before anything is allocated"""
    layout.rates = [a[0] for a in info]
    layout.raw_lengths = [a[1] for a in info]
    layout.lengths = [n if sr == layout.sample_rate else out_length(n, *ratio(sr, layout.sample_rate))
                      for sr, n in zip(layout.rates, layout.raw_lengths)]
    layout.offsets = [0] + list(np.cumsum(layout.lengths)[:-1].tolist())
    layout.total = int(sum(layout.lengths))
    layout.nbytes = sides * 4 * layout.total
    # + the staging of one chunk of one side (fp32 at worst): at most CHUNK_SAMPLES / 2 samples, or one file if it is longer
    need = layout.nbytes + 4 * min(sum(layout.raw_lengths), CHUNK_SAMPLES // 2 + max(layout.raw_lengths))
    if max_bytes is not None and need > max_bytes:
        raise MemoryError(f'the {what} needs {need} bytes on the device, max_bytes allows {max_bytes}')
    free = torch.cuda.mem_get_info(layout.device)[0]
    if need > free:
        raise MemoryError(f'the {what} needs {need} bytes on the device, {free} are free')


def _fill(layout, sides):
    """decode and upload in chunks of at most CHUNK_SAMPLES / 2 input samples; sides = [(paths, arena)], loaded in that order
    chunk by chunk"""
    n_files = len(layout.raw_lengths)
    with torch.cuda.device(layout.device), ThreadPoolExecutor(max_workers=READ_THREADS) as pool:
        i = 0
        while i < n_files:
            j, acc = i, 0
            while j < n_files and (j == i or acc + layout.raw_lengths[j] <= CHUNK_SAMPLES // 2):
                acc += layout.raw_lengths[j]
                j += 1
            for paths, arena in sides:
                _load_files(layout, list(range(i, j)), list(pool.map(_read_any, paths[i:j])), paths, arena)
            i = j
    torch.cuda.synchronize(layout.device)


class DeviceDataset:
    """Every (clean, noisy) pair of a VoiceBank-style directory pair, at `sample_rate`, resident on `device`.

    files[i] = sorted(glob(noisy_dir/*.wav))[i]; its clean twin is the same path with noisy_dir replaced by clean_dir
    (datasets/voicebank_dataset.py:28,39).  clean / noisy: fp32 arenas; offsets / lengths: where utterance i lives.

    noisy_dir None or '': a corpus of clean speech alone.  files = sorted(glob(clean_dir/*.wav)), `paired` is False and `noisy` IS
    `clean` (one arena); a loader over it takes all its noise from a NoiseBank (BankMix with prob 1)."""

    def __init__(self, clean_dir, noisy_dir, sample_rate=16000, device=None, max_bytes=None):
        self.paired = noisy_dir is not None and noisy_dir != ''
        self.clean_dir, self.noisy_dir, self.sample_rate = clean_dir, noisy_dir if self.paired else None, int(sample_rate)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != 'cuda':
            raise L.SeHipError('DeviceDataset lives on the GPU: there is no CPU fallback')
        self.files = sorted(glob.glob(f'{noisy_dir if self.paired else clean_dir}/*.wav'))
        if not self.files:
            raise FileNotFoundError(f'no wav files under {noisy_dir if self.paired else clean_dir}')
        self.clean_files = [p.replace(noisy_dir, clean_dir) for p in self.files] if self.paired else list(self.files)
        with ThreadPoolExecutor(max_workers=READ_THREADS) as pool:
            info_n = list(pool.map(_wav_info, self.files))
            info_c = list(pool.map(_wav_info, self.clean_files)) if self.paired else info_n
        for p, a, b in zip(self.files, info_n, info_c):
            if a != b:
                raise ValueError(f'{p}: the noisy file has {a[1]} samples at {a[0]} Hz, its clean file {b[1]} at {b[0]} Hz')
            if a[1] <= 0:
                raise ValueError(f'{p}: empty file')
        _lay_out(self, info_n, 2 if self.paired else 1, max_bytes, 'dataset')
        self.clean = torch.empty(self.total, dtype=torch.float32, device=self.device)
        self.noisy = torch.empty(self.total, dtype=torch.float32, device=self.device) if self.paired else self.clean
        _fill(self, [(self.files, self.noisy), (self.clean_files, self.clean)] if self.paired else [(self.clean_files, self.clean)])

    def _load(self, idx, read, paths, arena):
        _load_files(self, idx, read, paths, arena)

    def __len__(self):
        return len(self.files)

    def signal(self, i):
        """(clean, noisy) views of utterance i"""
        o, n = self.offsets[i], self.lengths[i]
        return self.clean[o:o + n], self.noisy[o:o + n]


class NoiseBank:
    """Every wav under `noise_dir` (one folder or a list of folders, each searched recursively, its files in sorted order), mono, at
    `sample_rate`, resident on `device` in one fp32 arena: the noise a loader with `bank=BankMix(...)` adds to its speech crops.
    Decoding, resampling and layout are those of DeviceDataset.  arena[offsets[i]:offsets[i] + lengths[i]] is file i; a noise crop
    may start anywhere in a file and wraps around its end, so a file may be shorter than a crop."""

    def __init__(self, noise_dir, sample_rate=16000, device=None, max_bytes=None):
        dirs = [noise_dir] if isinstance(noise_dir, (str, os.PathLike)) else list(noise_dir)
        self.noise_dir, self.sample_rate = [str(d) for d in dirs], int(sample_rate)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != 'cuda':
            raise L.SeHipError('NoiseBank lives on the GPU: there is no CPU fallback')
        self.files = [p for d in self.noise_dir for p in sorted(glob.glob(os.path.join(d, '**', '*.wav'), recursive=True))]
        if not self.files:
            raise FileNotFoundError(f'no wav files under {", ".join(self.noise_dir)}')
        with ThreadPoolExecutor(max_workers=READ_THREADS) as pool:
            info = list(pool.map(_wav_info, self.files))
        for p, a in zip(self.files, info):
            if a[1] <= 0:
                raise ValueError(f'{p}: empty file')
        _lay_out(self, info, 1, max_bytes, 'noise bank')
        for p, n in zip(self.files, self.lengths):
            if n > MAX_NOISE_SAMPLES:
                raise ValueError(f'{p}: {n} samples at {self.sample_rate} Hz; a file of the noise bank holds at most {MAX_NOISE_SAMPLES}')
        self.arena = torch.empty(self.total, dtype=torch.float32, device=self.device)
        _fill(self, [(self.files, self.arena)])

    def __len__(self):
        return len(self.files)

    def signal(self, i):
        """view of file i"""
        o, n = self.offsets[i], self.lengths[i]
        return self.arena[o:o + n]


def zero_energy(stats):
    """the default rejection rule on stats [b, 3] = (sum clean^2, sum noisy^2, max |clean|): a signal without energy, where
    normalize_batch divides by zero"""
    return (stats[:, 0] == 0) | (stats[:, 1] == 0)


def crop_rng(seed, epoch, rank):
    """the private stream of crop starts of one (seed, epoch, rank)"""
    return random.Random(f'se-crop-{int(seed)}-{int(epoch)}-{int(rank)}')


def mix_rng(seed, epoch, rank):
    """the private stream of noise draws of one (seed, epoch, rank): its own, so the crop starts of a loader do not move when
    remixing is switched on"""
    return random.Random(f'se-mix-{int(seed)}-{int(epoch)}-{int(rank)}')


class Remix:
    """Dynamic mixing: with probability `prob` a row's noise is replaced by the noise of a uniformly drawn utterance (its own
    included), scaled so that the crop's SNR is uniform in snr_db = (lo, hi) dB.  Gain augmentation is not part of it:
    normalize_batch rescales every pair by the noisy energy."""

    def __init__(self, prob, snr_db=(0.0, 20.0)):
        prob = float(prob)
        lo, hi = (float(v) for v in snr_db)
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f'remix probability {prob} is outside [0, 1]')
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f'remix SNR bounds ({lo}, {hi}) are not finite')
        if lo > hi:
            raise ValueError(f'remix SNR bounds ({lo}, {hi}): the lower one is the larger')
        self.prob, self.snr_db = prob, (lo, hi)

    def __repr__(self):
        return f'Remix({self.prob}, snr_db={self.snr_db})'


def draw_mix(files, lengths, crop_samples, rng, remix):
    """the noise of every row of `files`, in order: (noise file, noise start, snr dB) or None for a row that keeps its own noise.
    Every row consumes the same draws whether it is mixed or not -- u = random(), j = randrange(N), the start
    randint(0, len_j - L) (none when len_j < L: the noise is tiled, start -1), snr = uniform(lo, hi) -- and is mixed iff u < prob."""
    out = []
    lo, hi = remix.snr_db
    for _ in files:
        u = rng.random()
        j = rng.randrange(len(lengths))
        start = rng.randint(0, lengths[j] - crop_samples) if lengths[j] >= crop_samples else -1
        snr = rng.uniform(lo, hi)
        out.append((j, start, snr) if u < remix.prob else None)
    return out


def mix_chunks(samples):
    """workgroups (chunks of SE_MIX_CHUNK samples) a row of se_crop_gather_mix is spread over"""
    return -(-int(samples) // MIX_CHUNK)


def _launch_mix(dataset, rows, snr_db, samples, bank=None):
    """one se_crop_gather_mix -- with `bank` (a NoiseBank or its stand-in) one se_crop_gather_bank -- for rows int64 [b, 6]
    (include/se_hip.h) and the SNR of every row -> clean [b, L], noisy [b, L] and the
    launch's doubles: tail = buf[2 b nchunk:] holds the statistics [b][nchunk][3] followed by the scales (b floats)"""
    b, n = len(rows), mix_chunks(samples)
    dev = dataset.clean.device
    host = np.empty(7 * b, dtype=np.int64)              # the row table and the gains in one upload
    host[:6 * b] = np.asarray(rows, dtype=np.int64).reshape(-1)
    host[6 * b:].view(np.float64)[:] = [10.0 ** (-float(v) / 20.0) for v in snr_db]
    clean = torch.empty(b, samples, dtype=torch.float32, device=dev)
    noisy = torch.empty(b, samples, dtype=torch.float32, device=dev)
    buf = torch.empty(5 * b * n + (b + 1) // 2, dtype=torch.float64, device=dev)
    table = torch.from_numpy(host).to(dev, non_blocking=True)
    need = L.lib().se_crop_gather_mix_workspace_bytes(b, samples)
    if need != 16 * b * n:
        raise L.SeHipError(f'se_crop_gather_mix wants {need} workspace bytes for B {b}, L {samples}: {16 * b * n} were laid out')
    at, base = table.data_ptr(), buf.data_ptr()           # addresses inside the two buffers: a tensor view each costs microseconds
    with torch.cuda.device(dev):
        if bank is None:
            L.call('se_crop_gather_mix', L.ptr(dataset.clean), L.ptr(dataset.noisy), dataset.clean.numel(), C.c_void_p(at),
                   C.c_void_p(at + 48 * b), b, samples, L.ptr(clean), L.ptr(noisy), C.c_void_p(base + 16 * b * n),
                   C.c_void_p(base + 40 * b * n), C.c_void_p(base), need, L.stream())
        else:
            if bank.arena.device != dev or bank.arena.dtype != torch.float32 or not bank.arena.is_contiguous() \
                    or bank.arena.numel() < bank.total:
                raise L.SeHipError('the noise bank is one contiguous fp32 arena of `total` samples on the device of the dataset')
            L.call('se_crop_gather_bank', L.ptr(dataset.clean), L.ptr(dataset.noisy), dataset.clean.numel(), L.ptr(bank.arena),
                   int(bank.total), C.c_void_p(at), C.c_void_p(at + 48 * b), b, samples, L.ptr(clean), L.ptr(noisy),
                   C.c_void_p(base + 16 * b * n), C.c_void_p(base + 40 * b * n), C.c_void_p(base), need, L.stream())
    return clean, noisy, buf[2 * b * n:]


def _sum_chunks(tail, b, n):
    """host copy of a launch's tail -> (stats [b, 3] float64: the chunk partials added in index order, scale [b] float32)"""
    part = tail[:3 * b * n].reshape(b, n, 3)
    stats = np.empty((b, 3), dtype=np.float64)
    stats[:, :2] = np.cumsum(part[:, :, :2], axis=1)[:, -1]        # a running sum: chunk 0, + chunk 1, ... (np.sum may add pairwise)
    stats[:, 2] = part[:, :, 2].max(axis=1)
    return stats, tail[3 * b * n:].view(np.float32)[:b].copy()


def mix_at_snr(dataset, i, j, snr_db, noise_start=0):
    """(clean, noisy) device tensors of the whole utterance i with the noise of utterance j at snr_db: noise samples
    noise_start ... when j is at least as long as i, else j's noise tiled.  Silent noise or speech returns the pair as stored."""
    n, m = dataset.lengths[i], dataset.lengths[j]
    if m >= n and not 0 <= noise_start <= m - n:
        raise ValueError(f'noise start {noise_start} leaves utterance {j} of {m} samples ({n} are needed)')
    rows = [[dataset.offsets[i], n, 0, dataset.offsets[j], m, noise_start if m >= n else 0]]
    clean, noisy, _ = _launch_mix(dataset, rows, [snr_db], n)
    return clean[0], noisy[0]


class BankMix:
    """Noise from outside the corpus: with probability `prob` a row's noise is a crop of `bank` (a NoiseBank), the file drawn in
    proportion to its duration, the start anywhere in it (the crop wraps around the file's end), scaled so that the crop's SNR is
    uniform in snr_db = (lo, hi) dB.  A row that is not drawn keeps the noise of its own pair."""

    def __init__(self, bank, prob, snr_db=(0.0, 20.0)):
        prob = float(prob)
        lo, hi = (float(v) for v in snr_db)
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f'noise bank probability {prob} is outside [0, 1]')
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f'noise bank SNR bounds ({lo}, {hi}) are not finite')
        if lo > hi:
            raise ValueError(f'noise bank SNR bounds ({lo}, {hi}): the lower one is the larger')
        if not all(hasattr(bank, a) for a in ('lengths', 'offsets', 'total', 'arena')):
            raise TypeError(f'BankMix takes a NoiseBank (lengths, offsets, total, arena), got {type(bank).__name__}')
        if len(bank.lengths) < 1 or len(bank.lengths) != len(bank.offsets) or int(bank.total) < 1:
            raise ValueError('BankMix: the noise bank is empty')
        self.bank, self.prob, self.snr_db = bank, prob, (lo, hi)

    def __repr__(self):
        return f'BankMix({len(self.bank.lengths)} files, {self.prob}, snr_db={self.snr_db})'


def bank_rng(seed, epoch, rank):
    """the private stream of noise-bank draws of one (seed, epoch, rank): its own, so order and crop starts of a loader do not move
    when the bank is switched on"""
    return random.Random(f'se-bank-{int(seed)}-{int(epoch)}-{int(rank)}')


def draw_bank(n_rows, offsets, total, rng, mix):
    """the bank noise of n_rows rows, in order: (bank file, start in it, snr dB) or None for a row that keeps its own noise.  Every
    row consumes the same three draws whether it is mixed or not -- u = random(), p = randrange(total), snr = uniform(lo, hi) -- and
    is mixed iff u < prob.  p is a sample of the arena: the file it lies in and its place there are file and start, so files are
    weighted by duration, and since the noise wraps every start is legal."""
    out = []
    lo, hi = mix.snr_db
    for _ in range(n_rows):
        u = rng.random()
        p = rng.randrange(total)
        snr = rng.uniform(lo, hi)
        j = bisect.bisect_right(offsets, p) - 1
        out.append((j, p - offsets[j], snr) if u < mix.prob else None)
    return out


def mix_bank_at_snr(dataset, bank, i, j, snr_db, noise_start=0):
    """(clean, noisy) device tensors of the whole utterance i with file j of `bank` at snr_db: noise samples noise_start ..., wrapped
    around the end of the file.  Silent noise or speech returns the pair as stored."""
    n, m = dataset.lengths[i], bank.lengths[j]
    if not 0 <= noise_start < m:
        raise ValueError(f'noise start {noise_start} is outside file {j} of {m} samples')
    rows = [[dataset.offsets[i], n, 0, bank.offsets[j], m, noise_start]]
    clean, noisy, _ = _launch_mix(dataset, rows, [snr_db], n, bank)
    return clean[0], noisy[0]


def sampler_order(n, world=1, rank=0, shuffle=True, seed=0, epoch=0):
    """the indices one rank visits in one epoch: torch.utils.data.DistributedSampler(range(n), world, rank, shuffle, seed) after
    set_epoch(epoch) for world > 1 (padded by wrapping so every rank gets ceil(n / world)); for world == 1 randperm(n) from a
    generator seeded seed + epoch, or range(n)"""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    if world == 1:
        return order
    total = -(-n // world) * world
    pad = total - n
    order += order[:pad] if pad <= n else (order * -(-pad // n))[:pad]
    return order[rank:total:world]


class _Gathered:
    """one se_crop_gather launch in flight: the device tensors and the statistics on their way to pinned memory"""
    __slots__ = ('clean', 'noisy', 'host', 'full', 'event', 'pool')

    def stats(self):
        """[b, 3] numpy (waits for the copy only); the pinned buffer goes back to the loader"""
        self.event.synchronize()
        out = self.host.numpy().copy()
        self.pool.append(self.full)
        self.host = self.full = None
        return out


class _GatheredMix(_Gathered):
    """one se_crop_gather_mix in flight; `scale` [b] (0 = the row kept its own noise) is there once stats() has returned"""
    __slots__ = ('chunks', 'scale')

    def stats(self):
        self.event.synchronize()
        out, self.scale = _sum_chunks(self.host.numpy(), self.clean.shape[0], self.chunks)
        self.pool.append(self.full)
        self.host = self.full = None
        return out


class DeviceLoader:
    """Batches of random crops of a DeviceDataset: the DataLoader + DistributedSampler + Collator of the reference's main_gan.py.

    Order: `sampler_order`.  Crops: a row with length >= L draws start = randint(0, length - L) from `crop_rng(seed, epoch, rank)`,
    a shorter row is tiled to L samples and draws nothing.  A row whose statistics `reject` flags (default `zero_energy`; the
    reference rejects where PESQ throws) is redrawn, all rejected rows of the batch in one pass, up to 10 attempts in all, then
    dropped -- the batch gets smaller, as in the reference; a tiled row is dropped at once; a batch that loses every row is
    skipped.  The gather of batch i + 1 is launched before the statistics of batch i are waited for, so the draws of a redraw
    pass of batch i come after the first draws of batch i + 1 in the stream.

    remix: a `Remix`, or None for the corpus' own pairs.  The noise of every row is drawn by `draw_mix` from `mix_rng(seed, epoch,
    rank)` -- order and crop starts are those of the same loader without remix -- and every gather, redraw passes (which draw a fresh
    noise tuple) included, is one se_crop_gather_mix.  The key of a mixed row is (file, start, noise file, noise start, snr dB); a
    row the kernel did not mix (silent noise or speech) keeps the plain (file, start), as do the rows that were not drawn.

    bank: a `BankMix`, or None; not together with remix.  The same plan with the noise of a NoiseBank: `draw_bank` from
    `bank_rng(seed, epoch, rank)`, every gather one se_crop_gather_bank, the key of a mixed row (file, start, 'bank', bank file,
    start in it, snr dB).  Over a dataset of clean speech alone (`paired` False) the bank is required, with prob 1, and a row the
    kernel did not mix (scale 0: it would be delivered with noisy == clean) counts as rejected: redrawn with a fresh start and fresh
    noise -- a tiled row, which has no start to draw, with fresh noise alone -- and dropped after the last attempt."""

    def __init__(self, dataset, batch_size, crop_samples, shuffle, seed=0, rank=0, world=1, reject=None, remix=None, bank=None):
        if batch_size < 1 or crop_samples < 1 or not 0 <= rank < world:
            raise ValueError(f'bad loader geometry: batch {batch_size}, crop {crop_samples}, rank {rank} of {world}')
        self.dataset, self.batch_size, self.crop_samples, self.shuffle = dataset, int(batch_size), int(crop_samples), bool(shuffle)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.reject = reject if reject is not None else zero_energy
        if remix is not None and not isinstance(remix, Remix):
            raise TypeError(f'remix takes a Remix or None (got {type(remix).__name__})')
        if bank is not None and not isinstance(bank, BankMix):
            raise TypeError(f'bank takes a BankMix or None (got {type(bank).__name__})')
        if remix is not None and bank is not None:
            raise ValueError('a loader mixes either the noise of its corpus (remix) or that of a noise bank (bank), not both')
        self.unpaired = not getattr(dataset, 'paired', True)
        if self.unpaired and (bank is None or bank.prob != 1.0):
            raise ValueError('a dataset of clean speech alone has no noise of its own: its loader needs bank=BankMix(bank, 1.0)')
        self.remix, self.bank = remix, bank
        self._pinned, self._pinned_mix = [], []

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        return sampler_order(len(self.dataset), self.world, self.rank, self.shuffle, self.seed, self.epoch)

    def __len__(self):
        return -(-len(self.indices()) // self.batch_size)

    def _draw(self, files, rng):
        Lc, lengths = self.crop_samples, self.dataset.lengths
        return [rng.randint(0, lengths[f] - Lc) if lengths[f] >= Lc else -1 for f in files]

    def _gather(self, files, starts):
        """launch one se_crop_gather for rows (file, start) -> _Gathered"""
        ds, b, Lc = self.dataset, len(files), self.crop_samples
        rows = np.empty((b, 3), dtype=np.int64)
        for r, (f, s) in enumerate(zip(files, starts)):
            n = ds.lengths[f]
            if not (0 <= f < len(ds.lengths)) or (n >= Lc and not 0 <= s <= n - Lc):
                raise L.SeHipError(f'crop ({f}, {s}) is outside utterance {f} of {n} samples')
            rows[r] = (ds.offsets[f], n, max(s, 0))
        dev = ds.clean.device
        g = _Gathered()
        g.clean = torch.empty(b, Lc, dtype=torch.float32, device=dev)
        g.noisy = torch.empty(b, Lc, dtype=torch.float32, device=dev)
        stats = torch.empty(b, 3, dtype=torch.float32, device=dev)
        rows_d = torch.from_numpy(rows).to(dev, non_blocking=True)
        with torch.cuda.device(dev):
            L.call('se_crop_gather', L.ptr(ds.clean), L.ptr(ds.noisy), C.c_longlong(ds.clean.numel()), L.ptr(rows_d), C.c_int(b),
                   C.c_int(Lc), L.ptr(g.clean), L.ptr(g.noisy), L.ptr(stats), L.stream())
            full = self._pinned.pop() if self._pinned else torch.empty(self.batch_size, 3, dtype=torch.float32, pin_memory=True)
            g.full, g.host = full, full[:b]
            g.host.copy_(stats, non_blocking=True)
            g.event = torch.cuda.Event()
            g.event.record()
        g.pool = self._pinned
        return g

    def _gather_mix(self, files, starts, mix):
        """launch one se_crop_gather_mix for rows (file, start) with the noise `mix` of draw_mix -> _GatheredMix"""
        ds, b, Lc = self.dataset, len(files), self.crop_samples
        rows = np.empty((b, 6), dtype=np.int64)
        for r, (f, s, m) in enumerate(zip(files, starts, mix)):
            n = ds.lengths[f]
            if not (0 <= f < len(ds.lengths)) or (n >= Lc and not 0 <= s <= n - Lc):
                raise L.SeHipError(f'crop ({f}, {s}) is outside utterance {f} of {n} samples')
            if m is None:
                rows[r] = (ds.offsets[f], n, max(s, 0), -1, 0, 0)
                continue
            j, sj, _ = m
            nj = ds.lengths[j]
            if not (0 <= j < len(ds.lengths)) or (nj >= Lc and not 0 <= sj <= nj - Lc):
                raise L.SeHipError(f'noise crop ({j}, {sj}) is outside utterance {j} of {nj} samples')
            rows[r] = (ds.offsets[f], n, max(s, 0), ds.offsets[j], nj, max(sj, 0))
        g = _GatheredMix()
        g.chunks = mix_chunks(Lc)
        g.clean, g.noisy, tail = _launch_mix(ds, rows, [m[2] if m is not None else 0.0 for m in mix], Lc)
        self._download(g, tail)
        return g

    def _gather_bank(self, files, starts, mix):
        """launch one se_crop_gather_bank for rows (file, start) with the noise `mix` of draw_bank -> _GatheredMix"""
        ds, nb, b, Lc = self.dataset, self.bank.bank, len(files), self.crop_samples
        rows = np.empty((b, 6), dtype=np.int64)
        for r, (f, s, m) in enumerate(zip(files, starts, mix)):
            n = ds.lengths[f]
            if not (0 <= f < len(ds.lengths)) or (n >= Lc and not 0 <= s <= n - Lc):
                raise L.SeHipError(f'crop ({f}, {s}) is outside utterance {f} of {n} samples')
            if m is None:
                rows[r] = (ds.offsets[f], n, max(s, 0), -1, 0, 0)
                continue
            j, sj, _ = m
            if not (0 <= j < len(nb.lengths)) or not 0 <= sj < nb.lengths[j]:
                raise L.SeHipError(f'noise start ({j}, {sj}) is outside the noise bank')
            rows[r] = (ds.offsets[f], n, max(s, 0), nb.offsets[j], nb.lengths[j], sj)
        g = _GatheredMix()
        g.chunks = mix_chunks(Lc)
        g.clean, g.noisy, tail = _launch_mix(ds, rows, [m[2] if m is not None else 0.0 for m in mix], Lc, nb)
        self._download(g, tail)
        return g

    def _download(self, g, tail):
        """the doubles of a mixed launch on their way to pinned memory"""
        per = 3 * g.chunks
        with torch.cuda.device(g.clean.device):
            full = self._pinned_mix.pop() if self._pinned_mix else \
                torch.empty(self.batch_size * per + (self.batch_size + 1) // 2, dtype=torch.float64, pin_memory=True)
            g.full, g.host = full, full[:tail.numel()]
            g.host.copy_(tail, non_blocking=True)
            g.event = torch.cuda.Event()
            g.event.record()
        g.pool = self._pinned_mix

    def _draw_noise(self, files, mrng):
        """one noise tuple per row from the loader's noise stream"""
        if self.bank is not None:
            return draw_bank(len(files), self.bank.bank.offsets, self.bank.bank.total, mrng, self.bank)
        return draw_mix(files, self.dataset.lengths, self.crop_samples, mrng, self.remix)

    def _gather_noise(self, files, starts, mix):
        return self._gather_bank(files, starts, mix) if self.bank is not None else self._gather_mix(files, starts, mix)

    def _place(self, g, rows, sub):
        """rows `rows` of batch g <- the redrawn crops `sub`"""
        at = torch.as_tensor(rows, device=g.clean.device)
        g.clean.index_copy_(0, at, sub.clean)
        g.noisy.index_copy_(0, at, sub.noisy)

    def _select(self, g, keep):
        at = torch.as_tensor(keep, device=g.clean.device)
        return g.clean.index_select(0, at), g.noisy.index_select(0, at)

    def _finish(self, files, starts, g, rng, mix=None, mrng=None):
        """wait for the statistics of a gathered batch, redraw / drop what they reject -> the item, or None"""
        starts = list(starts)
        rejected = np.asarray(self.reject(g.stats()), dtype=bool)
        if mix is not None:
            mix, scale = list(mix), g.scale
        attempt = 1
        Lc, lengths = self.crop_samples, self.dataset.lengths
        # a tiled row has no other crop to offer: what `reject` flags of them is dropped at once
        dropped = [r for r in np.flatnonzero(rejected).tolist() if lengths[files[r]] < Lc]
        if self.unpaired:               # no noise of its own: an unmixed row is redrawn too (a tiled one with fresh noise alone)
            rejected = rejected | (np.asarray(scale) == 0)
        bad = [r for r in np.flatnonzero(rejected).tolist() if r not in dropped]
        while bad and attempt < MAX_ATTEMPTS:
            sub_files = [files[r] for r in bad]
            sub_starts = self._draw(sub_files, rng)
            if mix is None:
                sub = self._gather(sub_files, sub_starts)
            else:
                sub_mix = self._draw_noise(sub_files, mrng)
                sub = self._gather_noise(sub_files, sub_starts, sub_mix)
            self._place(g, bad, sub)
            for r, s in zip(bad, sub_starts):
                starts[r] = s
            still = np.asarray(self.reject(sub.stats()), dtype=bool)
            if mix is not None:
                for k, r in enumerate(bad):
                    mix[r], scale[r] = sub_mix[k], sub.scale[k]
            if self.unpaired:
                dropped += [r for r, x in zip(bad, still) if x and lengths[files[r]] < Lc]
                still = still | (np.asarray(sub.scale) == 0)
            bad = [r for r, x in zip(bad, still) if x and r not in dropped]
            attempt += 1
        dropped = set(dropped + bad)
        keep = [r for r in range(len(files)) if r not in dropped]
        if not keep:
            return None
        clean, noisy = (g.clean, g.noisy) if not dropped else self._select(g, keep)
        keys = [(int(files[r]), int(starts[r])) for r in keep]
        if mix is not None:
            tag = ('bank',) if self.bank is not None else ()
            keys = [k + tag + (int(mix[r][0]), int(mix[r][1]), float(mix[r][2])) if mix[r] is not None and scale[r] != 0 else k
                    for k, r in zip(keys, keep)]
        return {'audio': clean, 'noisy': noisy, 'keys': keys}

    def __iter__(self):
        rng = crop_rng(self.seed, self.epoch, self.rank)
        mrng = None
        if self.remix is not None:
            mrng = mix_rng(self.seed, self.epoch, self.rank)
        elif self.bank is not None:
            mrng = bank_rng(self.seed, self.epoch, self.rank)
        order = self.indices()
        pending = None
        for i in range(0, len(order), self.batch_size):
            files = order[i:i + self.batch_size]
            starts = self._draw(files, rng)
            if mrng is None:
                cur = (files, starts, self._gather(files, starts), rng)
            else:
                mix = self._draw_noise(files, mrng)
                cur = (files, starts, self._gather_noise(files, starts, mix), rng, mix, mrng)
            if pending is not None:
                item = self._finish(*pending)
                if item is not None:
                    yield item
            pending = cur
        if pending is not None:
            item = self._finish(*pending)
            if item is not None:
                yield item
