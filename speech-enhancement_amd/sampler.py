"""The reverse process of the TSC-diffusion hybrid (inference_diffuse.py:231-269) without the host in the loop.

`predict_tsc` runs the generator once per reverse step with ~1500 launches each, does the [B, L] sampler arithmetic as PyTorch ops,
calls torch.randn_like and uploads the step value every step.  Here the step index, the utterance counter and the seed live in
device memory (csrc/se_sampler.hip): `se_sampler_update` is the whole update of a step in one launch with the Gaussian noise drawn
in the kernel (Philox4x32-10 + Box-Muller), `se_sampler_advance` moves the step index and fetches the next step's projected
embedding from a table computed once, so ONE reverse step is captured as a HIP graph and replayed `steps` times per utterance.

The noise is the sampler's own: outputs differ draw-for-draw from a torch.randn_like run and are reproducible per seed.  With
`noises` supplied the sampler computes what predict_tsc computes with the same `noises`."""
import numpy as np
import torch

from . import _lib as L
from . import frontend as FE
from . import ops as O
from .diffuse import inference_schedule
from .inference import LRU, Enhancer, capture, hop_frames, spectral_forward
from .tsc_diffusion import step_embedding

GAMMA = 0.2                     # inference_diffuse.py:248
_M64 = (1 << 64) - 1


def pack_coef(c1, c2, c3, delta_bar):
    """the kernel's table [steps, 4] float32 = (c1, c2, c3, sigma = sqrt(delta_bar)) of inference_schedule's lists"""
    return np.stack([np.asarray(c1, np.float64), np.asarray(c2, np.float64), np.asarray(c3, np.float64),
                     np.sqrt(np.asarray(delta_bar, np.float64))], 1).astype(np.float32)


def _check(t, dtype, what):
    if t is None:
        return
    L.check_cuda(t)
    if t.dtype != dtype or not t.is_contiguous():
        raise L.SeHipError(f'sampler: {what} must be a contiguous {dtype} tensor')


def sampler_update(audio, noisy, eps, coef, n, noise=None, seed=None, run=None, c_inv=None, gamma=GAMMA, clamp=False):
    """se_sampler_update (include/se_hip.h): one reverse step on audio [B, L] in place.  coef [steps, 4] float32, n int32 [1],
    noise [steps - 1, B, L] or None (then seed int64 [1] and run int32 [1] drive the in-kernel generator), c_inv = the clip scales
    c [B] whose reciprocal multiplies the result of step 0.  Everything lives on the device; nothing is read back."""
    for t, what in ((audio, 'audio'), (noisy, 'noisy'), (eps, 'eps'), (coef, 'coef'), (noise, 'noise'), (c_inv, 'c_inv')):
        _check(t, torch.float32, what)
    _check(n, torch.int32, 'n')
    _check(run, torch.int32, 'run')
    _check(seed, torch.int64, 'seed')
    B, Ls = audio.shape
    steps = coef.shape[0]
    if noisy.shape != audio.shape or eps.shape != audio.shape or coef.shape != (steps, 4) or n.numel() != 1:
        raise L.SeHipError(f'sampler_update: shapes {tuple(audio.shape)} {tuple(noisy.shape)} {tuple(eps.shape)} {tuple(coef.shape)}')
    if noise is not None and noise.numel() != max(steps - 1, 0) * B * Ls:
        raise L.SeHipError(f'sampler_update: noise must hold [{steps - 1}, {B}, {Ls}] values (got {tuple(noise.shape)})')
    if noise is None and (seed is None or run is None or seed.numel() != 1 or run.numel() != 1):
        raise L.SeHipError('sampler_update: without a noise buffer the kernel draws: pass seed (int64 [1]) and run (int32 [1])')
    if c_inv is not None and c_inv.numel() != B:
        raise L.SeHipError(f'sampler_update: c_inv must have {B} entries')
    L.call('se_sampler_update', L.ptr(audio), L.ptr(noisy), L.ptr(eps), L.ptr(coef), L.ptr(n), steps, L.ptr(noise), L.ptr(seed),
           L.ptr(run), L.ptr(c_inv), float(gamma), int(bool(clamp)), B, Ls, L.stream())
    return audio


def sampler_advance(n, run, emb, d):
    """se_sampler_advance: n <- n - 1 (from 0: steps - 1, and run <- run + 1); d [1, 64] <- row n of emb [steps, 64]"""
    _check(n, torch.int32, 'n')
    _check(run, torch.int32, 'run')
    _check(emb, torch.float32, 'emb')
    _check(d, torch.float32, 'd')
    if emb.dim() != 2 or emb.shape[1] != 64 or d.numel() != 64 or n.numel() != 1 or run.numel() != 1:
        raise L.SeHipError(f'sampler_advance: emb must be [steps, 64] and d [1, 64] (got {tuple(emb.shape)}, {tuple(d.shape)})')
    L.call('se_sampler_advance', L.ptr(n), L.ptr(run), emb.shape[0], L.ptr(emb), L.ptr(d), L.stream())


def sampler_begin(x, c, audio, noisy):
    """se_sampler_begin: audio = noisy = wrap_pad(x) * c; x [B, length], c [B], audio / noisy [B, padded]"""
    for t, what in ((x, 'x'), (c, 'c'), (audio, 'audio'), (noisy, 'noisy')):
        _check(t, torch.float32, what)
    B, length = x.shape
    if audio.shape != noisy.shape or audio.shape[0] != B or c.numel() != B:
        raise L.SeHipError(f'sampler_begin: shapes {tuple(x.shape)} {tuple(c.shape)} {tuple(audio.shape)} {tuple(noisy.shape)}')
    L.call('se_sampler_begin', L.ptr(x), L.ptr(c), L.ptr(audio), L.ptr(noisy), B, length, audio.shape[1], L.stream())


def philox_normal(seed, c2, c3, first_group, n_groups, words=False, normals=True, device=torch.device('cuda')):
    """se_philox_normal: the sampler's generator for groups first_group .. first_group + n_groups - 1 with counter words (c2, c3) =
    (n, run).  Returns (words, normals): int32 [4 n_groups] holding the raw 32-bit words (view them as uint32 on the host) and
    float32 [4 n_groups]; the one that was not asked for is None."""
    w = torch.empty(4 * n_groups, device=device, dtype=torch.int32) if words else None
    z = torch.empty(4 * n_groups, device=device, dtype=torch.float32) if normals else None
    with torch.cuda.device(device):
        L.call('se_philox_normal', int(seed) & _M64, int(c2) & 0xFFFFFFFF, int(c3) & 0xFFFFFFFF, int(first_group) & _M64,
               int(n_groups), L.ptr(w), L.ptr(z), L.stream())
    return w, z


class GraphedTSCSampler(Enhancer):
    """predict_tsc with ONE reverse step (STFT of the current audio, the hybrid generator, iSTFT, se_sampler_update,
    se_sampler_advance) captured into a HIP graph (inference.capture) per LENGTH BUCKET = number of STFT frames, replayed `steps`
    times per utterance; the same graph serves any schedule length.  Per utterance the host copies the signal in, launches the clip scale, the wrap-pad
    and the STFT of the conditioning spectrum eagerly, then only replays.

    State shared by all buckets (device): n = index of the next reverse step (steps - 1 between utterances), run = utterances
    finished since the seed was set, the seed, d = the projected embedding of step n.  The step-embedding table and the coefficient
    table are computed once: call refresh() after the weights change.
    `noises` ([steps - 1, 1, padded length]) selects the supplied-noise variant of a bucket (its own graph: the kernel's noise source
    is a launch argument); without it the kernel draws.  `max_graphs` bounds the cache (least recently used is dropped)."""

    def __init__(self, model, args, config, fast=False, device=torch.device('cuda'), max_graphs=4, seed=0):
        self.model, self.config, self.fast, self.max_graphs = model, config, bool(fast), max_graphs
        self.device = torch.device(device)
        self.comp = getattr(args, 'comp_type', 'pow')
        self.buckets = LRU()                  # (frames, supplied noise) -> dict(graph, audio, noisy, orig_planes, c, noise)
        dev = self.device
        self.n = torch.zeros(1, device=dev, dtype=torch.int32)
        self.run = torch.zeros(1, device=dev, dtype=torch.int32)
        self.seed = torch.zeros(1, device=dev, dtype=torch.int64)
        self.d = torch.zeros(1, 64, device=dev, dtype=torch.float32)
        self.refresh()
        self.set_seed(seed)

    @torch.no_grad()
    def refresh(self):
        """recompute the schedule tables and the step-embedding table (after the weights or the config changed)"""
        sched = inference_schedule(self.config, fast_sampling=self.fast)
        T, c1, c2, c3, delta_bar = sched[4], sched[5], sched[6], sched[7], sched[9]
        self.steps = len(c1)
        if len(T) != self.steps:
            raise L.SeHipError(f'sampler: the inference schedule aligns {len(T)} of its {self.steps} steps with the training schedule')
        coef = torch.from_numpy(pack_coef(c1, c2, c3, delta_bar)).to(self.device)
        emb = step_embedding(self.model, torch.as_tensor(np.asarray(T, np.float32), device=self.device)).float().contiguous()
        if getattr(self, 'coef', None) is not None and self.coef.shape == coef.shape:
            self.coef.copy_(coef)                    # in place: the captured graphs hold these addresses
            self.emb.copy_(emb)
        else:
            self.coef, self.emb = coef, emb
            self.buckets.clear()
        self._rewind()

    def _rewind(self):
        self.n.fill_(self.steps - 1)
        self.d.copy_(self.emb[self.steps - 1:self.steps])

    def set_seed(self, seed):
        """key of the generator; the utterance counter restarts, so a seed names one reproducible sequence of utterances"""
        s = int(seed) & _M64
        self.seed.fill_(s - (1 << 64) if s >> 63 else s)
        self.run.zero_()

    def _step(self, b):
        eps = spectral_forward(self.model, self.config, b['audio'], b['orig_planes'], None, comp=self.comp, d=self.d)
        sampler_update(b['audio'], b['noisy'], eps, self.coef, self.n, noise=b['noise'], seed=self.seed, run=self.run, c_inv=b['c'],
                       gamma=GAMMA, clamp=False)
        sampler_advance(self.n, self.run, self.emb, self.d)

    def _conditioner(self, b):
        cfg = self.config
        planes, _ = FE.stft_planes(b['noisy'], cfg.N_FFT, cfg.HOP_SAMPLES, self.comp, padded=False)
        return planes

    def _build(self, frames, supplied):
        hop, dev = self.config.HOP_SAMPLES, self.device
        Lp = frames * hop
        b = {'audio': torch.zeros(1, Lp, device=dev, dtype=torch.float32), 'noisy': torch.zeros(1, Lp, device=dev, dtype=torch.float32),
             'c': torch.ones(1, device=dev, dtype=torch.float32),
             'noise': torch.zeros(self.steps - 1, 1, Lp, device=dev, dtype=torch.float32) if supplied else None}
        b['noisy'].normal_(0.0, 0.1)                 # warm-up on non-degenerate data
        b['audio'].copy_(b['noisy'])
        with torch.no_grad():
            b['orig_planes'] = self._conditioner(b).clone()
            n0, run0 = self.n.clone(), self.run.clone()

        def restore():                               # the warm-up leaves the step index, its embedding and the counter as they were
            self.n.copy_(n0)
            self.run.copy_(run0)
            self.d.copy_(self.emb[self.steps - 1:self.steps])
        b['graph'], _ = capture(lambda: self._step(b), dev, restore)
        return b

    def _bucket(self, frames, supplied):
        return self.buckets.lookup((frames, bool(supplied)), lambda: self._build(frames, bool(supplied)), self.max_graphs)

    @torch.no_grad()
    def enhance_device(self, noisy_signal, noises=None):
        """the enhanced signal as a device tensor [length], complete on the current stream: a view of the bucket's audio buffer,
        valid until the same bucket is used again (metrics.evaluate scores it in place)"""
        x = np.ascontiguousarray(np.asarray(noisy_signal, dtype=np.float32).reshape(1, -1))
        length, hop = x.shape[1], self.config.HOP_SAMPLES
        frames, pad = hop_frames(length, hop)
        if pad > length:
            raise L.SeHipError(f'sampler: a signal of {length} samples is shorter than its padding to the hop ({hop})')
        with torch.cuda.device(self.device):
            b = self._bucket(frames, noises is not None)
            self._rewind()                           # (an utterance that ended in an exception may have left n anywhere)
            xd = torch.from_numpy(x).to(self.device, non_blocking=True)
            b['c'].copy_(O.clip_scale(xd))           # c = sqrt(L / sum x^2) over the UNPADDED signal: one eager launch
            sampler_begin(xd, b['c'], b['audio'], b['noisy'])
            b['orig_planes'].copy_(self._conditioner(b))
            if noises is not None:
                nz = (noises if torch.is_tensor(noises) else torch.from_numpy(np.asarray(noises))).to(torch.float32).reshape(-1)
                if nz.numel() != b['noise'].numel():
                    raise L.SeHipError(f'sampler: noises must hold [{self.steps - 1}, 1, {frames * hop}] values (got {nz.numel()})')
                b['noise'].copy_(nz.view_as(b['noise']), non_blocking=True)
            for _ in range(self.steps):
                b['graph'].replay()
        return torch.flatten(b['audio'])[:length]
