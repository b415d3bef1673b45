"""TSC-diffusion hybrid: the reference's `models/tsc_diffusion.py` TSCNet -- the CMGAN generator with a second
DenseEncoder for the noisy conditioner and a `MergeBlock` (diffusion-step embedding + gated 1x1 convolutions) in front of every TSCB
-- and `inference_diffuse.predict_tsc` (:231-269), on the HIP kernels of the generator.  This file holds the module tree and the
steps around the network; the network itself is the generator's walk with a conditioner (`layers.tscnet_fwd(cond=(nin, d))` /
`tscnet_bwd`, MergeBlock: `layers.merge_fwd` / `merge_bwd`) behind the generator's autograd node.  Training step of the hybrid
(`core/function.py:25-44` add_noise, `:453-532` train_tsc_diffusion): `tsc_diffusion_step` = add_noise -> two compressed
STFTs -> the generator in train mode (hand-written backward: both encoders, the four MergeBlock applications, TSCBs, decoders) ->
iSTFT -> L1 against the combined noise -> optimizer step.  fp32 arithmetic (the reference wraps this loop in fp16 autocast +
GradScaler: a precision policy of its CUDA run, not part of the function being computed).  With `seed=` the prologue of the step --
the clip scaling, the draw of the diffusion steps and of the noise, add_noise -- runs on the device from the sampler's Philox generator
(`draw_steps`, `diffusion_noise`: csrc/se_sampler.hip), reproducible from (seed, counter) alone; the epoch loops (train_diffuse.py) use it.

state_dict names are the reference's (`dense_encoder_noisy.*`, `merge_block.diffusion_embedding.projection1.weight`,
`merge_block.merge_diffusion.weight [128, 64, 1, 1]`, ...), so its checkpoints load with `load_state_dict`.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import frontend as FE
from . import losses as LS
from . import ops as O
from .diffuse import _DiffusionEmbedding
from .generator import TSCNet, _TSCNetFn, _dilated_dense


class TSCNetDiffusion(TSCNet):
    """models/tsc_diffusion.py:43-90.  forward(x complex [B, F, T], noisy_spec complex [B, F, T], diffusion_step [1] or [B])
    -> (real, imag) [B, 1, T, F]."""

    def __init__(self, num_channel=64, num_features=201, noise_schedule=None):
        super().__init__(num_channel, num_features)
        ch = num_channel
        enc = nn.Module()
        enc.conv_1 = nn.Sequential(nn.Conv2d(3, ch, (1, 1)), nn.InstanceNorm2d(ch, affine=True), nn.PReLU(ch))
        enc.dilated_dense = _dilated_dense(ch)
        enc.conv_2 = nn.Sequential(nn.Conv2d(ch, ch, (1, 3), (1, 2), padding=(0, 1)), nn.InstanceNorm2d(ch, affine=True), nn.PReLU(ch))
        self.dense_encoder_noisy = enc
        mb = nn.Module()
        mb.diffusion_embedding = _DiffusionEmbedding(len(noise_schedule))
        mb.diffusion_projection = nn.Linear(512, ch)
        mb.merge_diffusion = nn.Conv2d(ch, ch * 2, 1)
        mb.conditioner_projection = nn.Conv2d(ch, ch * 2, 1)
        mb.output_residual = nn.Conv2d(ch, ch, 1)
        self.merge_block = mb
        self._pnames = [k for k, _ in self.named_parameters()]

    def forward_planes(self, xin, nin, diffusion_step, d=None):
        """xin / nin: planes [B, T, F, 4] of the current and of the conditioning spectrum -> est planes [B, T, F, 4]: the generator's
        walk (layers.tscnet_fwd) with the conditioner.  Train mode records the hand-written backward; eval mode records nothing.
        d (optional): the projected step embedding [1, 64] on the device, used instead of the embedding MLP of diffusion_step"""
        if d is not None and (tuple(d.shape) != (1, 64) or d.device != xin.device or d.dtype != torch.float32):
            raise L.SeHipError('TSCNetDiffusion: d must be a float32 [1, 64] tensor on the device of the planes')
        with torch.set_grad_enabled(self.training and torch.is_grad_enabled()):
            if d is None:
                d = step_embedding(self, torch.as_tensor(diffusion_step, device=xin.device))     # [N, 64], host-sized plumbing
            return _TSCNetFn.apply(self, xin, nin, d, *[p for _, p in self.named_parameters()])

    def forward(self, x, noisy_spec, diffusion_step=None):
        est = self.forward_planes(FE.spec_to_planes(x), FE.spec_to_planes(noisy_spec), diffusion_step)
        return est[..., 1].unsqueeze(1), est[..., 2].unsqueeze(1)


def step_embedding(model, t):
    """MergeBlock's projected diffusion-step embedding d [N, 64] (tsc_diffusion.py:28-29): plain torch (autograd) on [N, 512]"""
    mb = model.merge_block
    return mb.diffusion_projection(mb.diffusion_embedding(t))


def add_noise(audio, noisy, noise_schedule, t=None, noise=None):
    """core/function.py:25-44: (noisy_audio, combine_noise, t) of the supportive forward process; t / noise may be supplied
    (reproducible parity runs), otherwise drawn like the reference ([N] uniform steps, standard normal noise)."""
    N, _ = audio.shape
    beta = np.array(noise_schedule)
    noise_level = torch.tensor(np.cumprod(1 - beta).astype(np.float32), device=audio.device)
    if t is None:
        t = torch.randint(0, len(noise_schedule), [N], device=audio.device)
    noise_scale = noise_level[t].unsqueeze(1)
    noise_scale_sqrt = noise_scale ** 0.5
    m = (((1 - noise_level[t]) / noise_level[t] ** 0.5) ** 0.5).unsqueeze(1)
    if noise is None:
        noise = torch.randn_like(audio)
    noisy_audio = (1 - m) * noise_scale_sqrt * audio + m * noise_scale_sqrt * noisy + (1.0 - (1 + m ** 2) * noise_scale) ** 0.5 * noise
    combine_noise = (m * noise_scale_sqrt * (noisy - audio) + (1.0 - (1 + m ** 2) * noise_scale) ** 0.5 * noise) / (1 - noise_scale) ** 0.5
    return noisy_audio, combine_noise, t


_M64 = (1 << 64) - 1
STEP_STREAM = 1 << 30               # counter word 3 of the step draw = word 3 of the noise draw with this bit set
KIND_TRAIN, KIND_VALID = 0, 2       # `kind` of the noise stream; the step stream of either is kind + 1


def pack_counter(kind, rank=0):
    """counter word 3 of a draw: (kind << 30) | rank with kind 0 = training noise, 1 = training steps, 2 = validation noise,
    3 = validation steps, so no two of the four streams of any two ranks share a counter"""
    if not 0 <= kind < 4 or not 0 <= rank < STEP_STREAM:
        raise L.SeHipError(f'pack_counter: kind {kind} / rank {rank} outside [0, 4) / [0, 2^30)')
    return (kind << 30) | rank


def step_index(epoch, idx, iters_per_epoch):
    """counter word 2 of training iteration idx of an epoch: the number of iterations before it mod 2^32, so a run resumed at an
    epoch boundary continues the sequence of draws of the uninterrupted run"""
    return (epoch * iters_per_epoch + idx) & 0xFFFFFFFF


def noise_coefficients(noise_schedule):
    """the kernel's table [steps, 5] float32 = (A, Bn, S, G, H) of add_noise per diffusion step: noisy_audio = A audio + Bn noisy +
    S noise, combine_noise = G (noisy - audio) + H noise.  From the reference's starting values (cumprod(1 - beta) in float32),
    evaluated in float64 and rounded once"""
    a = np.cumprod(1 - np.asarray(noise_schedule, np.float64)).astype(np.float32).astype(np.float64)
    m = np.sqrt((1 - a) / np.sqrt(a))
    A, Bn, S = (1 - m) * np.sqrt(a), m * np.sqrt(a), np.sqrt(1 - (1 + m * m) * a)
    return np.stack([A, Bn, S, Bn / np.sqrt(1 - a), S / np.sqrt(1 - a)], 1).astype(np.float32)


_COEF_TABLES = {}


def _coef_table(noise_schedule, device):
    key = (str(device), tuple(noise_schedule))
    if key not in _COEF_TABLES:
        _COEF_TABLES[key] = torch.from_numpy(noise_coefficients(noise_schedule)).to(device)
    return _COEF_TABLES[key]


def draw_steps(seed, c2, c3, B, steps, device=torch.device('cuda')):
    """se_diffuse_draw_steps (include/se_hip.h): t int64 [B] on the device, t[b] = (word 0 of Philox(seed; b, 0, c2, c3) * steps) >> 32"""
    device = torch.device(device)
    if device.type != 'cuda':
        raise L.SeHipError('draw_steps: the draw happens on the GPU (no CPU fallback)')
    if B <= 0 or steps <= 0:
        raise L.SeHipError(f'draw_steps: bad sizes (B {B}, steps {steps})')
    t = torch.empty(B, device=device, dtype=torch.int64)
    with torch.cuda.device(device):
        L.call('se_diffuse_draw_steps', int(seed) & _M64, int(c2) & 0xFFFFFFFF, int(c3) & 0xFFFFFFFF, int(B), int(steps), L.ptr(t),
               L.stream())
    return t


def diffusion_noise(clean, noisy, c, coef, t, noise=None, seed=None, c2=0, c3=0):
    """se_diffuse_noise (include/se_hip.h): normalize_batch + add_noise of a batch in one launch.  clean, noisy [B, L] float32,
    c [B] (ops.clip_scale), coef [steps, 5] float32 (noise_coefficients), t int64 [B]; the noise is either supplied (noise [B, L])
    or drawn in the kernel (seed, with counter words c2, c3).  Returns (noisy_n, x_t, combine), each [B, L]."""
    L.check_cuda(clean, noisy, c, coef, t, noise)
    if (noise is None) == (seed is None):
        raise L.SeHipError('diffusion_noise: pass exactly one of noise (supplied) and seed (drawn in the kernel)')
    if clean.dim() != 2 or clean.numel() == 0:
        raise L.SeHipError(f'diffusion_noise: clean must be a non-empty [B, L] tensor (got {tuple(clean.shape)})')
    B, Ls = clean.shape
    if noisy.shape != clean.shape or tuple(c.shape) != (B,) or tuple(t.shape) != (B,) or coef.dim() != 2 or coef.shape[1] != 5 \
            or coef.shape[0] == 0 or (noise is not None and noise.shape != clean.shape):
        raise L.SeHipError(f'diffusion_noise: shapes clean {tuple(clean.shape)} noisy {tuple(noisy.shape)} c {tuple(c.shape)} '
                           f'coef {tuple(coef.shape)} t {tuple(t.shape)} noise {None if noise is None else tuple(noise.shape)}')
    for x, dtype, what in ((clean, torch.float32, 'clean'), (noisy, torch.float32, 'noisy'), (c, torch.float32, 'c'),
                           (coef, torch.float32, 'coef'), (t, torch.int64, 't'), (noise, torch.float32, 'noise')):
        if x is not None and (x.dtype != dtype or not x.is_contiguous() or x.device != clean.device):
            raise L.SeHipError(f'diffusion_noise: {what} must be a contiguous {dtype} tensor on the device of clean')
    noisy_n, x_t, combine = torch.empty_like(clean), torch.empty_like(clean), torch.empty_like(clean)
    with torch.cuda.device(clean.device):
        L.call('se_diffuse_noise', L.ptr(clean), L.ptr(noisy), L.ptr(c), L.ptr(coef), L.ptr(t), L.ptr(noise),
               0 if seed is None else int(seed) & _M64, int(c2) & 0xFFFFFFFF, int(c3) & 0xFFFFFFFF, B, Ls, coef.shape[0],
               L.ptr(noisy_n), L.ptr(x_t), L.ptr(combine), L.stream())
    return noisy_n, x_t, combine


def _noised_planes(clean, noisy, noise_schedule, n_fft, hop, comp_type, t, noise, seed=None, counter=None):
    """the prologue of the train and the validation step: normalize_batch, add_noise, compressed STFTs of the noised clip and of the
    noisy clip (conditioner).  Returns (noised planes, conditioner planes, combine_noise, t).
    seed (with t and noise None): the draws come from the sampler's generator on the device -- clip_scale, draw_steps, diffusion_noise
    -- with counter = (c2, c3) for the noise and (c2, c3 | STEP_STREAM) for the steps; they depend on (seed, counter) only."""
    if seed is not None:
        if t is not None or noise is not None:
            raise L.SeHipError('tsc_diffusion: seed draws t and the noise on the device; supply t / noise or a seed, not both')
        c2, c3 = (0, 0) if counter is None else counter
        if int(c3) & STEP_STREAM:
            raise L.SeHipError('tsc_diffusion: counter word 3 names the noise stream (bit 30 clear); its step stream sets bit 30')
        clean, noisy = clean.contiguous(), noisy.contiguous()
        c = O.clip_scale(noisy)
        t = draw_steps(seed, c2, int(c3) | STEP_STREAM, clean.shape[0], len(noise_schedule), clean.device)
        noisy_n, noisy_audio, combine_noise = diffusion_noise(clean, noisy, c, _coef_table(noise_schedule, clean.device), t,
                                                              seed=seed, c2=c2, c3=c3)
        orig_pl, _ = FE.stft_planes(noisy_n, n_fft, hop, comp_type, padded=False)
        nz_pl, _ = FE.stft_planes(noisy_audio, n_fft, hop, comp_type, padded=False)
        return nz_pl, orig_pl, combine_noise, t
    if counter is not None:
        raise L.SeHipError('tsc_diffusion: counter names a draw of the seeded generator; pass seed with it')
    c = O.clip_scale(noisy.contiguous())
    clean, noisy = clean * c[:, None], noisy * c[:, None]
    noisy_audio, combine_noise, t = add_noise(clean, noisy, noise_schedule, t, noise)
    orig_pl, _ = FE.stft_planes(noisy.contiguous(), n_fft, hop, comp_type, padded=False)
    nz_pl, _ = FE.stft_planes(noisy_audio.contiguous(), n_fft, hop, comp_type, padded=False)
    return nz_pl, orig_pl, combine_noise, t


def tsc_diffusion_step(model, optimizer, clean, noisy, noise_schedule, n_fft=400, hop=100, comp_type='pow', max_norm=0.0,
                       t=None, noise=None, step=True, seed=None, counter=None):
    """One iteration of train_tsc_diffusion (core/function.py:472-525): normalize_batch, add_noise, compressed STFT of the noisy
    clip (conditioner) and of the noised clip, the hybrid generator, iSTFT, loss = mean |predicted - combine_noise|, backward,
    optional global-norm clipping, optimizer step.  Returns the loss (0-d tensor).
    seed / counter = (c2, c3): t and the noise are drawn on the device from (seed, counter) alone (_noised_planes) instead of from
    torch's global generator."""
    from . import train as TR
    nz_pl, orig_pl, combine_noise, t = _noised_planes(clean, noisy, noise_schedule, n_fft, hop, comp_type, t, noise, seed, counter)
    params = [p for _, p in model.named_parameters()]
    O.ARENA.begin(clean.device)
    try:
        est = model.forward_planes(nz_pl, orig_pl, t)
        predicted = FE.istft_planes(est, n_fft, hop, comp_type)
        loss = LS.l1_time_loss(predicted, combine_noise.contiguous())
        optimizer.zero_grad()
        loss.backward()
        if max_norm != 0.0:
            TR.clip_grad_norm(optimizer, params, max_norm)
        if step:
            optimizer.step()
    finally:
        O.ARENA.end()
    return loss.detach()


@torch.no_grad()
def tsc_diffusion_validation_loss(model, clean, noisy, noise_schedule, n_fft=400, hop=100, comp_type='pow', t=None, noise=None,
                                  seed=None, counter=None):
    """One iteration of validate_tsc_diffusion (core/function.py:566-597): the same pipeline as the training step in eval mode
    (BatchNorm running statistics, no dropout), no backward.  Returns the loss (0-d tensor).  seed / counter: as in the step."""
    if model.training:
        raise L.SeHipError('tsc_diffusion_validation_loss: call model.eval() first (the reference validates in eval mode)')
    nz_pl, orig_pl, combine_noise, t = _noised_planes(clean, noisy, noise_schedule, n_fft, hop, comp_type, t, noise, seed, counter)
    est = model.forward_planes(nz_pl, orig_pl, t)
    predicted = FE.istft_planes(est, n_fft, hop, comp_type)
    return LS.l1_time_loss(predicted, combine_noise.contiguous()).detach()


@torch.no_grad()
def predict_tsc(model, args, config, noisy_signal, alpha, beta, alpha_cum, sigmas, T, c1, c2, c3, delta, delta_bar,
                device=torch.device('cuda'), noises=None):
    """inference_diffuse.py:231-269: the supportive reverse process in the compressed-STFT domain -- every step re-analyses the
    current audio, runs the hybrid generator conditioned on the noisy spectrum and the step, re-synthesises the predicted noise.
    `noises` (optional, [steps - 1, 1, padded length]) replaces torch.randn_like for reproducible parity runs."""
    noisy = torch.as_tensor(np.asarray(noisy_signal), dtype=torch.float32, device=device).unsqueeze(0)
    hop, n_fft = config.HOP_SAMPLES, config.N_FFT
    comp = getattr(args, 'comp_type', 'pow')
    c = O.clip_scale(noisy.contiguous())
    length = noisy.size(-1)
    padding_len = int(np.ceil(length / hop)) * hop - length
    noisy = noisy * c[:, None]
    noisy = torch.cat([noisy, noisy[:, :padding_len]], dim=-1).contiguous()
    audio = noisy_audio = noisy
    orig_planes, _ = FE.stft_planes(noisy, n_fft, hop, comp, padded=False)
    if noises is not None:
        noises = torch.as_tensor(np.asarray(noises), dtype=torch.float32, device=device)
    gamma = [0.2]
    k = 0
    for n in range(len(alpha) - 1, -1, -1):
        planes, _ = FE.stft_planes(audio.contiguous(), n_fft, hop, comp, padded=False)
        est = model.forward_planes(planes, orig_planes, torch.tensor([float(T[n])], device=device))
        predicted_noise = FE.istft_planes(est, n_fft, hop, comp)
        if n > 0:
            audio = float(c1[n]) * audio + float(c2[n]) * noisy_audio - float(c3[n]) * predicted_noise
            noise = torch.randn_like(audio) if noises is None else noises[k]
            k += 1
            audio = audio + float(delta_bar[n]) ** 0.5 * noise
        else:
            audio = float(c1[n]) * audio - float(c3[n]) * predicted_noise
            audio = (1 - gamma[n]) * audio + gamma[n] * noisy_audio
    audio = audio / c[:, None]
    return torch.flatten(audio)[:length].cpu().numpy()
