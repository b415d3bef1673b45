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
