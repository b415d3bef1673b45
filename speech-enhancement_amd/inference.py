"""inference_gan.py's model loading and per-utterance enhancement (inference_gan.py:60-100) on the HIP path.

Whole-utterance batch-1 forward exactly like the reference (InstanceNorm and attention span the utterance).  The
objective-metric loop over the enhanced audio is metrics.evaluate."""
from collections import OrderedDict

import numpy as np
import torch

from . import frontend as FE
from . import ops as O
from .generator import TSCNet


def load_model(model_path, config, device=torch.device('cuda')):
    """inference_gan.py:60-72: TSCNet(64, N_FFT//2+1), checkpoint['gen_state_dict'], eval().  The reference strips
    7 characters from every key because its checkpoints always come from DDP ('module.' prefix, main_gan.py:142);
    here the prefix is stripped only where present, so single-GPU checkpoints of this package load as well."""
    model = TSCNet(num_channel=64, num_features=config.N_FFT // 2 + 1).to(device)
    checkpoint = torch.load(model_path, map_location=device)
    sd = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in checkpoint['gen_state_dict'].items())
    model.load_state_dict(sd)
    model.eval()
    return model


@torch.no_grad()
def predict(model, config, noisy_signal, device=torch.device('cuda')):
    """inference_gan.py:75-100: normalise by c, wrap-pad the head of the signal to a multiple of the hop, STFT ->
    generator -> iSTFT, de-normalise, truncate."""
    noisy = torch.as_tensor(np.asarray(noisy_signal), dtype=torch.float32, device=device).unsqueeze(0)
    hop, n_fft = config.HOP_SAMPLES, config.N_FFT
    c = O.clip_scale(noisy.contiguous())
    length = noisy.size(-1)
    frame_num = int(np.ceil(length / hop))
    padding_len = frame_num * hop - length
    noisy = torch.cat([noisy, noisy[:, :padding_len]], dim=-1)
    planes, _ = FE.stft_planes(noisy, n_fft, hop, 'pow', scale=c, padded=False)
    est = model.forward_planes(planes)
    est_audio = FE.istft_planes(est, n_fft, hop, 'pow') / c[:, None]
    est_audio = torch.flatten(est_audio)[:length].cpu().numpy()
    assert len(est_audio) == length, "Estimated audio and the origin audio must have the same length"
    return est_audio


class GraphedEnhancer:
    """predict() with the whole device-side pipeline (STFT, generator, iSTFT, de-normalisation) captured into HIP graphs,
    one graph per LENGTH BUCKET = number of STFT frames (all lengths that pad to the same multiple of the hop share a
    graph; the reference's wrap-padding to the hop multiple (inference_gan.py:84-87) is done on the host copy, the
    clip scale c of the UNPADDED signal by one eager launch in front of the replay, so results equal predict() exactly).

    Batch-1 inference is launch-bound: ~1500 kernel launches cost ~20 ms of host time for ~10 ms of GPU work, a replayed
    graph removes the host side.  All kernels are launched on torch's current stream, which is the capture stream
    inside `torch.cuda.graph`; the dynamic-LDS attributes are raised by the eager warm-up run before the capture.
    `max_graphs` bounds the cache (least recently used bucket is dropped)."""

    def __init__(self, model, config, length=None, device=torch.device('cuda'), max_graphs=8):
        self.model, self.config, self.device, self.max_graphs = model, config, device, max_graphs
        self.buckets = OrderedDict()          # frames -> dict(graph, static_in, c, out)
        if length is not None:
            self._bucket(int(np.ceil(int(length) / config.HOP_SAMPLES)))

    def _pipeline(self, b):
        cfg = self.config
        planes, _ = FE.stft_planes(b['static_in'], cfg.N_FFT, cfg.HOP_SAMPLES, 'pow', scale=b['c'], padded=False)
        est = self.model.forward_planes(planes)
        return FE.istft_planes(est, cfg.N_FFT, cfg.HOP_SAMPLES, 'pow') / b['c'][:, None]

    def _bucket(self, frames):
        b = self.buckets.get(frames)
        if b is not None:
            self.buckets.move_to_end(frames)
            return b
        hop = self.config.HOP_SAMPLES
        b = {'static_in': torch.zeros(1, frames * hop, device=self.device, dtype=torch.float32),
             'c': torch.ones(1, device=self.device, dtype=torch.float32)}
        b['static_in'].normal_(0.0, 0.1)             # warm-up on non-degenerate data
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._pipeline(b)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            b['graph'] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(b['graph']):
                b['out'] = self._pipeline(b)
        torch.cuda.synchronize()
        self.buckets[frames] = b
        while len(self.buckets) > self.max_graphs:
            self.buckets.popitem(last=False)
        return b

    @torch.no_grad()
    def enhance_device(self, noisy_signal):
        """the enhanced signal as a device tensor [length], complete on the current stream: a view of the bucket's output buffer,
        valid until the next utterance of the same bucket is enhanced (metrics.evaluate scores it in place)"""
        x = np.asarray(noisy_signal, dtype=np.float32).reshape(-1)
        length, hop = x.shape[0], self.config.HOP_SAMPLES
        frames = int(np.ceil(length / hop))
        b = self._bucket(frames)
        pad = frames * hop - length
        xp = np.concatenate([x, x[:pad]]) if pad else x        # the reference's wrap-pad (head of the signal)
        b['static_in'].copy_(torch.from_numpy(xp).reshape(1, -1), non_blocking=True)
        # c = sqrt(L / sum x^2) over the UNPADDED signal: one eager launch writing the scalar the graph reads
        b['c'].copy_(O.clip_scale(b['static_in'][:, :length].contiguous() if pad else b['static_in']))
        b['graph'].replay()
        return torch.flatten(b['out'])[:length]

    def __call__(self, noisy_signal):
        return self.enhance_device(noisy_signal).cpu().numpy()


def check_chunking(chunk, overlap, hop=100):
    """the chunk length S and the crossfade length V (samples) a chunk plan accepts"""
    S, V, hop = int(chunk), int(overlap), int(hop)
    if hop < 1 or S % hop != 0 or S <= 2 * hop:
        raise ValueError(f'chunk length {S} must be a multiple of the hop ({hop}) and longer than two hops: the STFT reflect-pads by 2 hops')
    if V < 1 or 3 * V > S:
        raise ValueError(f'chunk overlap {V} must lie in [1, chunk / 3 = {S // 3}]: a fade-in has to end before the next chunk starts')
    return S, V


def chunk_plan(length, chunk, overlap, hop=100):
    """start samples of the chunks of a recording of `length` samples: K chunks of `chunk` = S samples, all of them full of real audio
    (nothing is padded), the first at 0, the last ending at `length`, spread evenly, neighbours overlapping by at least `overlap` = V:
        K = max(2, ceil((L - V) / (S - V))),   s_k = (k (L - S)) // (K - 1)
    so every stride is <= S - V, and for K >= 3 it is >= V (needs 3 V <= S): the fade-in of a chunk over its first V samples is over
    before the next chunk starts, and every sample belongs to at most two chunks.  length <= S gives [0]: one whole-utterance forward."""
    S, V = check_chunking(chunk, overlap, hop)
    L = int(length)
    if L < 1:
        raise ValueError(f'chunk_plan: empty recording (length {L})')
    if L <= S:
        return [0]
    K = max(2, -(-(L - V) // (S - V)))
    return [(k * (L - S)) // (K - 1) for k in range(K)]


class LongEnhancer:
    """Enhances recordings of any length: the recording is cut into overlapping chunks (chunk_plan), each chunk is normalised by its
    own c = sqrt(S / sum x^2) -- the statistics of the crops the generator was trained on, not of the whole recording --, the chunks
    run through the generator `batch` at a time (the batched eval forward validate_gan uses), and the enhanced chunks are
    de-normalised and joined with a linear crossfade over the first `overlap_seconds` of every chunk.  The weights of the fade are
    amplitude-complementary (they sum to one): both sides estimate the same signal.  Chunks of exact zeros are not forwarded and
    come out as exact zeros.  A recording no longer than one chunk takes predict()'s whole-utterance arithmetic.

    Everything runs eagerly on the current stream: one copy of the recording to the device, one gather launch (ops.chunk_gather),
    one copy of the K silence flags back (the only synchronisation), ceil(non-silent K / batch) forwards, one assemble launch
    (ops.chunk_assemble).  Memory is that of one forward of `batch` chunks plus the recording, its chunks [K, S] twice (in and out) and the result.  Same contract as
    GraphedEnhancer: enhance_device -> device tensor [L], __call__ -> numpy, so metrics.evaluate(..., enhancer=...) takes it."""

    def __init__(self, model, config, chunk_seconds=4.0, overlap_seconds=0.5, batch=8, device=torch.device('cuda')):
        rate = getattr(config, 'SAMPLE_RATE', 16000)
        self.S, self.V = check_chunking(round(chunk_seconds * rate), round(overlap_seconds * rate), config.HOP_SAMPLES)
        if int(batch) < 1:
            raise ValueError(f'LongEnhancer: batch must be at least 1, got {batch}')
        self._require_eval(model)
        self.model, self.config, self.batch, self.device = model, config, int(batch), device
        self.forwards = 0               # generator forwards issued so far

    @staticmethod
    def _require_eval(model):
        if model.training:
            raise RuntimeError('LongEnhancer needs model.eval(): BatchNorm must use its running statistics')

    def _whole(self, x):
        """predict() on a device signal [L], result left on the device"""
        hop, n_fft = self.config.HOP_SAMPLES, self.config.N_FFT
        noisy = x.unsqueeze(0)
        c = O.clip_scale(noisy.contiguous())
        length = noisy.size(-1)
        padding_len = int(np.ceil(length / hop)) * hop - length
        noisy = torch.cat([noisy, noisy[:, :padding_len]], dim=-1)
        planes, _ = FE.stft_planes(noisy, n_fft, hop, 'pow', scale=c, padded=False)
        self.forwards += 1
        est = self.model.forward_planes(planes)
        est_audio = FE.istft_planes(est, n_fft, hop, 'pow') / c[:, None]
        return torch.flatten(est_audio)[:length]

    @torch.no_grad()
    def enhance_chunks(self, x):
        """x: device signal [L], L > S -> (y [K, S], c [K], silent [K], starts [K]): the enhanced chunks still scaled by c (rows of
        silent chunks are zeros), as ops.chunk_assemble takes them"""
        self._require_eval(self.model)
        hop, n_fft = self.config.HOP_SAMPLES, self.config.N_FFT
        plan = chunk_plan(x.numel(), self.S, self.V, hop)
        starts = torch.tensor(plan, dtype=torch.int64).to(x.device)
        chunks, c, silent = O.chunk_gather(x, starts, self.S)
        live = torch.nonzero(silent.cpu() == 0).flatten()
        y = torch.zeros_like(chunks)
        live_dev = live.to(x.device)
        for g in range(0, live.numel(), self.batch):
            rows = live_dev[g:g + self.batch]
            planes, _ = FE.stft_planes(chunks.index_select(0, rows), n_fft, hop, 'pow', scale=c.index_select(0, rows), padded=False)
            self.forwards += 1
            est = self.model.forward_planes(planes)
            y.index_copy_(0, rows, FE.istft_planes(est, n_fft, hop, 'pow'))
        return y, c, silent, starts

    @torch.no_grad()
    def enhance_device(self, noisy_signal):
        """the enhanced recording as a device tensor [length], complete on the current stream"""
        self._require_eval(self.model)
        x = torch.as_tensor(np.asarray(noisy_signal, dtype=np.float32).reshape(-1)).to(self.device)
        if x.numel() <= self.S:
            return self._whole(x)
        y, c, silent, starts = self.enhance_chunks(x)
        return O.chunk_assemble(y, c, silent, starts, self.V, x.numel())

    def __call__(self, noisy_signal):
        return self.enhance_device(noisy_signal).cpu().numpy()
