"""main_diffuse.py's command line and worker (flags main_diffuse.py:37-115, worker :153-342) for the TSC-diffusion hybrid.

    python -m speech_enhancement_amd.main_diffuse -a tsc-diffuse --cfg config/baseline.yaml -b 16 --optimizer adamw --lr 5e-4 \\
        --crop-len 2 --seed 1

Each epoch trains (train_diffuse.train_tsc_diffusion), validates and writes `checkpoint_{epoch:04d}.pth.tar` =
{'epoch', 'arch', 'state_dict' (keys prefixed `module.`), 'optimizer', 'scaler', 'best_loss'}: the file `inference_diffuse -a tsc-diffuse`
and the reference's own inference and `--resume` load.  The loss is a time-domain L1, so no PESQ label provider is needed.  The data
come from main_gan's loaders, called as they are: `--synthetic N`, `main_gan.DATASET_FACTORY`, or the four `config.DATA.*_DIR` wav
folders on the device with `--remix-prob/--remix-snr` or `--noise-dir/--noise-prob/--noise-snr`.  `--seed` (0 when unset) also keys
the diffusion steps and the noise, which are drawn on the device (train_diffuse.py).

One process on one GPU (the reference refuses that; here it is the supported form).  `-a diffuse` (CDiffuSE training, DESIGN.md
section 8 (f4)) and more than one rank are declined with an error before any GPU work."""
import argparse
import logging
import os
import random
import warnings

import numpy as np
import torch

from . import main_gan
from .config import get_config
from .optim import build_optimizer
from .train_diffuse import train_tsc_diffusion, validate_tsc_diffusion
from .tsc_diffusion import TSCNetDiffusion
from .utils import kaiming_init, save_checkpoint, strip_module_prefix

model_names = ['diffuse', 'tsc-diffuse']


def parse_option(argv=None):
    p = argparse.ArgumentParser(description='Diffusion speech enhancement training script')
    p.add_argument('-a', '--arch', metavar='ARCH', default='diffuse', choices=model_names)
    p.add_argument('--output', default='output', type=str, metavar='PATH')
    p.add_argument('--tag')
    p.add_argument('--cfg', type=str, required=True, metavar='FILE')
    p.add_argument('--opts', default=None, nargs='+')
    p.add_argument('-j', '--workers', default=32, type=int)
    p.add_argument('--epochs', default=100, type=int)
    p.add_argument('--start-epoch', default=0, type=int)
    p.add_argument('-b', '--batch-size', default=64, type=int)
    p.add_argument('--lr', '--learning-rate', default=0.01, type=float, dest='lr')
    p.add_argument('--momentum', default=0.9, type=float)
    p.add_argument('--wd', '--weight-decay', default=0.01, type=float, dest='weight_decay')
    p.add_argument('--max-norm', default=0.0, type=float)
    p.add_argument('-p', '--print-freq', default=10, type=int)
    p.add_argument('--resume', default='', type=str)
    p.add_argument('--world-size', default=-1, type=int)
    p.add_argument('--rank', default=-1, type=int)
    p.add_argument('--dist_url', default='env://')
    p.add_argument('--dist-backend', default='nccl', type=str)
    p.add_argument('--seed', default=None, type=int)
    p.add_argument('--gpu', default=None, type=int)
    p.add_argument('--multiprocessing-distributed', action='store_true')
    p.add_argument('--debug', action='store_true')
    p.add_argument('--optimizer', default='sgd', type=str, choices=['sgd', 'adamw', 'lars', 'lamb'])
    p.add_argument('--criterion', default='l1', type=str, choices=['mae', 'l1', 'mse', 'l2', 'quantile'])
    p.add_argument('--crop-len', default=1, type=int)
    p.add_argument('--comp-type', default='pow', type=str, choices=['norm', 'log', 'pow', 'none'])
    # main_gan's data flags (their meaning: main_gan.parse_option)
    p.add_argument('--synthetic', default=0, type=int, metavar='N',
                   help='train on N synthetic batches per epoch instead of the wav folders')
    p.add_argument('--remix-prob', default=0.0, type=float, metavar='P')
    p.add_argument('--remix-snr', default=[0.0, 20.0], type=float, nargs=2, metavar=('LO', 'HI'))
    p.add_argument('--noise-dir', default=None, type=str, nargs='+', metavar='DIR')
    p.add_argument('--noise-prob', default=1.0, type=float, metavar='P')
    p.add_argument('--noise-snr', default=[0.0, 20.0], type=float, nargs=2, metavar=('LO', 'HI'))
    args, _ = p.parse_known_args(argv)
    config = get_config(args)
    if isinstance(config.NOISE_SCHEDULE, int):          # config/default.py:119: the number of training steps -> the beta list
        config = config.clone()
        config.NOISE_SCHEDULE = np.linspace(1e-4, 0.035, config.NOISE_SCHEDULE).tolist()
        config.freeze()
    return args, config


def check_supported(args):
    """what this command line declines, before CUDA is touched"""
    if args.arch.startswith('diffuse'):
        raise RuntimeError("-a diffuse: CDiffuSE training is declined (DESIGN.md section 8 (f4)); the model runs for inference only "
                           "(inference_diffuse). Train the hybrid with -a tsc-diffuse")
    world = args.world_size
    if args.dist_url == 'env://' and world == -1:
        world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1 or args.multiprocessing_distributed:
        raise RuntimeError('data-parallel hybrid training is not built: run one process on one GPU (no --world-size > 1, no '
                           '--multiprocessing-distributed)')


def _fresh_scaler_state():
    """the state of an untouched GradScaler: the reference's --resume reads checkpoint['scaler']; training here is fp32 and has none"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return torch.cuda.amp.GradScaler().state_dict()


def main_worker(gpu, args, config):
    args.gpu = 0 if gpu is None else gpu
    args.distributed, args.rank = False, 0
    torch.cuda.set_device(args.gpu)
    model = TSCNetDiffusion(num_channel=64, num_features=config.N_FFT // 2 + 1, noise_schedule=config.NOISE_SCHEDULE)
    model.apply(kaiming_init)
    model.cuda(args.gpu)
    optimizer = build_optimizer(args, model)
    best_loss = 1e8
    if args.resume:
        if os.path.isfile(args.resume):
            ck = torch.load(args.resume, map_location=f'cuda:{args.gpu}')
            args.start_epoch = ck['epoch']
            model.load_state_dict(strip_module_prefix(ck['state_dict']))
            optimizer.load_state_dict(ck['optimizer'])
            best_loss = ck['best_loss']             # (ck['scaler'] belongs to the reference's fp16 loop: ignored)
            print("=> loaded checkpoint '{}' (epoch {})".format(args.resume, ck['epoch']))
        else:
            print("=> no checkpoint found at '{}'".format(args.resume))
    samples = config.CROP_FRAMES * config.HOP_SAMPLES * config.CROP_LEN
    if args.synthetic:
        train_loader = [{k: v.cuda(args.gpu) for k, v in b.items() if torch.is_tensor(v)}
                        for b in main_gan.synthetic_loader(args.synthetic, args.batch_size, samples, 1)]
        valid_loader = train_loader[:1]
    elif main_gan.DATASET_FACTORY is not None:
        train_loader, valid_loader = main_gan.DATASET_FACTORY(args, config)
    elif all(os.path.isdir(d) for d in (config.DATA.TRAIN_CLEAN_DIR, config.DATA.TRAIN_NOISY_DIR or config.DATA.TRAIN_CLEAN_DIR,
                                        config.DATA.TEST_CLEAN_DIR, config.DATA.TEST_NOISY_DIR)):
        train_loader, valid_loader = main_gan.device_loaders(args, config, samples)
    else:
        raise RuntimeError('no training data: pass --synthetic N, set speech_enhancement_amd.main_gan.DATASET_FACTORY, or point '
                           'config.DATA.*_DIR at the four wav folders')
    logger = logging.getLogger(args.arch)
    logging.basicConfig(level=logging.INFO)
    logger.info(f'start_epoch == {args.start_epoch}')
    scaler_state = _fresh_scaler_state()
    for epoch in range(args.start_epoch, args.epochs):
        for loader in (train_loader, valid_loader):
            if hasattr(loader, 'set_epoch'):
                loader.set_epoch(epoch)
        train_loss = train_tsc_diffusion(train_loader, model, None, optimizer, None, logger, epoch, args, config)
        valid_loss = validate_tsc_diffusion(valid_loader, model, None, None, logger, epoch, args, config)
        is_best = valid_loss <= best_loss
        best_loss = min(best_loss, valid_loss)
        # every key carries the DDP prefix: the reference's inference strips seven characters from each without looking
        save_checkpoint({'epoch': epoch + 1, 'arch': args.arch,
                         'state_dict': {'module.' + k: v for k, v in model.state_dict().items()},
                         'optimizer': optimizer.state_dict(), 'scaler': scaler_state, 'best_loss': best_loss},
                        config.OUTPUT, is_best=is_best, filename='checkpoint_{:04d}.pth.tar'.format(epoch))
        logger.info('=> saving checkpoint: checkpoint_{:04d}.pth.tar'.format(epoch))
        logger.info('Train Loss: {:.3f}\t Validation Loss: {:.3f}'.format(train_loss, valid_loss))


def main(argv=None):
    args, config = parse_option(argv)
    check_supported(args)
    if args.remix_prob != 0 and (args.synthetic or main_gan.DATASET_FACTORY is not None):
        raise RuntimeError('--remix-prob mixes the noise of the device-resident wav folders (config.DATA.*_DIR): it cannot be '
                           'combined with --synthetic or a DATASET_FACTORY')
    if args.synthetic or main_gan.DATASET_FACTORY is not None:
        if args.noise_dir:
            raise RuntimeError('--noise-dir mixes into crops of the device-resident wav folders (config.DATA.*_DIR): it cannot be '
                               'combined with --synthetic or a DATASET_FACTORY')
    else:
        main_gan.check_noise_flags(args, config)
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
        warnings.warn('You have chosen to seed training.')
    main_worker(args.gpu, args, config)


if __name__ == '__main__':
    main()
