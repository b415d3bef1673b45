"""inference_diffuse.py command line (flags :38-88, loop :271-346) for the two diffusion models.  Enhances every wav under
config.DATA.TEST_NOISY_DIR, scores it against the file of the same name under config.DATA.TEST_CLEAN_DIR on the device
(metrics.evaluate) and prints the reference's line `pesq csig cbak covl ssnr stoi`; `--validate-epochs` does so for
checkpoint_{start..end-1} and names the best epoch.  Without clean files it only enhances (and saves with --save).

`-a tsc*`: the graph-replayed sampler (sampler.GraphedTSCSampler), which draws its own Philox noise: reproducible per `--seed`, not
draw-for-draw equal to a torch.randn_like run.  `-a diffuse*`: diffuse.predict as it is (torch's generator, seeded with --seed).
Needs a wav reader (scipy.io.wavfile)."""
import argparse

import numpy as np
import torch

from .config import get_config
from .diffuse import DiffuSE, inference_schedule
from .diffuse import predict as predict_diffuse
from .inference import Enhancer, load_checkpoint_into
from .inference_gan import run_cli
from .sampler import GraphedTSCSampler
from .tsc_diffusion import TSCNetDiffusion


def parse_option(argv=None):
    p = argparse.ArgumentParser(description='runs diffusion speech-enhancement inference')
    p.add_argument('-a', '--arch', metavar='ARCH', default='diffuse',
                   help='model architecture: diffuse* | tsc* (default: diffuse)')
    p.add_argument('--output', '-o', type=str, required=True)
    p.add_argument('--model_path', '-m', type=str, required=True, metavar='FILE')
    p.add_argument('--cfg', type=str, required=True, metavar='FILE')
    p.add_argument('--save', action='store_true')
    p.add_argument('--validate-epochs', action='store_true')
    p.add_argument('--start', default=None, type=int)
    p.add_argument('--end', default=None, type=int)
    p.add_argument('--gpu', default=0, type=int)
    p.add_argument('--comp-type', default='pow', type=str, choices=['norm', 'log', 'pow', 'none'])
    p.add_argument('--opts', default=None, nargs='+')
    p.add_argument('--fast', dest='fast', action='store_true', help='fast sampling procedure')
    p.add_argument('--seed', default=0, type=int, help='seed of the sampling noise')
    args, _ = p.parse_known_args(argv)
    if not args.arch.startswith(('diffuse', 'tsc')):
        p.error(f'-a {args.arch}: expected diffuse* or tsc*')
    config = get_config(args)
    if isinstance(config.NOISE_SCHEDULE, int):          # config/default.py:119: the number of training steps -> the beta list
        config = config.clone()
        config.NOISE_SCHEDULE = np.linspace(1e-4, 0.035, config.NOISE_SCHEDULE).tolist()
        config.freeze()
    return args, config


def load_model(model_path, args, config, device=torch.device('cuda')):
    """inference_diffuse.py:91-114: the model of args.arch, checkpoint['state_dict'], eval().  The reference strips 7 characters
    from every key ('module.' of its DDP checkpoints); here the prefix is stripped only where present."""
    if args.arch.startswith('diffuse'):
        model = DiffuSE(config.DILATION_CYCLE_LENGTH, config.HOP_SAMPLES, config.N_SPECS, config.NOISE_SCHEDULE,
                        config.RESIDUAL_CHANNELS, config.RESIDUAL_LAYERS).to(device)
    else:
        model = TSCNetDiffusion(num_channel=64, num_features=config.N_FFT // 2 + 1, noise_schedule=config.NOISE_SCHEDULE).to(device)
    return load_checkpoint_into(model, model_path, 'state_dict', device)


class _DiffuseEnhancer(Enhancer):
    """diffuse.predict behind the `enhance_device` interface of metrics.evaluate (the result goes back to the device for scoring)"""

    def __init__(self, model, config, fast, device):
        self.model, self.config, self.device = model, config, device
        self.schedule = inference_schedule(config, fast_sampling=fast)

    def enhance_device(self, noisy_signal):
        x = np.asarray(noisy_signal, dtype=np.float32).reshape(-1)
        y = predict_diffuse(self.model, self.config, x, *self.schedule, device=self.device)
        return torch.from_numpy(np.ascontiguousarray(y[:x.shape[0]])).to(self.device)


def build_enhancer(args, config, model_path, device):
    model = load_model(model_path, args, config, device)
    if args.arch.startswith('tsc'):
        return model, GraphedTSCSampler(model, args, config, fast=args.fast, device=device, seed=args.seed)
    torch.manual_seed(args.seed)
    return model, _DiffuseEnhancer(model, config, args.fast, device)


def main(argv=None):
    args, config = parse_option(argv)
    device = torch.device('cuda', args.gpu)
    with torch.cuda.device(device):
        run_cli(args, config, lambda model_path: build_enhancer(args, config, model_path, device),
                lambda model, enhancer, x: enhancer.enhance_device(x))


if __name__ == '__main__':
    main()
