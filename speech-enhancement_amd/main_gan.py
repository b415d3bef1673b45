"""main_gan.py's command line and worker (flags main_gan.py:35-115, worker :118-315) on the HIP path.

    python -m speech_enhancement_amd.main_gan -a cmgan --cfg config/baseline.yaml -b 16 --optimizer adamw --lr 5e-4 \\
        --crop-len 2 --synthetic 8

One process per GPU: launch N processes with torch.distributed.run (env:// rendezvous); `--multiprocessing-distributed`
spawns them itself like the reference.  With `--synthetic N` the loaders are N synthetic batches per epoch with PESQ labels
supplied (the bench's data recipe); else `speech_enhancement_amd.main_gan.DATASET_FACTORY`, when set, is a callable returning
(train, valid) loaders; else the four `config.DATA.*_DIR` wav folders become device-resident datasets (data.py: decoded once,
resampled to 16 kHz on the GPU, one launch per batch of crops) and the PESQ labels come from the provider (train.py);
`--remix-prob P --remix-snr LO HI` then gives a training crop, with probability P, the noise of another utterance at an SNR
drawn from [LO, HI] dB (data.Remix); `--noise-dir DIR [DIR ...] --noise-prob P --noise-snr LO HI` adds noise from folders of
recordings outside the corpus instead (data.NoiseBank), and with `DATA.TRAIN_NOISY_DIR ''` and P = 1 trains from clean speech alone.
"""
import argparse
import os
import random
import types
import warnings

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .config import get_config
from .discriminator import Discriminator
from .generator import TSCNet
from .optim import build_optimizer
from .train import attach_data_parallel, train_gan, validate_gan
from .utils import kaiming_init, save_checkpoint, strip_module_prefix

model_names = ['cmgan', 'scp', 'cp', 'sc']
DATASET_FACTORY = None


def parse_option(argv=None):
    p = argparse.ArgumentParser(description='Speech enhancement training script')
    p.add_argument('-a', '--arch', metavar='ARCH', default='cmgan', choices=model_names + ['diffuse'])
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
    p.add_argument('--criterion', default='l1', type=str, choices=['mae', 'l1', 'mse', 'l2'])
    p.add_argument('--crop-len', default=1, type=int)
    p.add_argument('--gen-first', action='store_true')
    p.add_argument('--comp-type', default='pow', type=str, choices=['norm', 'log', 'pow', 'none'])
    p.add_argument('--synthetic', default=0, type=int, metavar='N',
                   help='train on N synthetic batches per epoch (labels supplied) instead of VoiceBank-DEMAND')
    p.add_argument('--remix-prob', default=0.0, type=float, metavar='P',
                   help='wav folders only: probability that a training crop gets the noise of another utterance (data.Remix)')
    p.add_argument('--remix-snr', default=[0.0, 20.0], type=float, nargs=2, metavar=('LO', 'HI'),
                   help='SNR range in dB of the remixed training crops')
    p.add_argument('--noise-dir', default=None, type=str, nargs='+', metavar='DIR',
                   help='wav folders only: folders (searched recursively) of noise recordings mixed into the training crops '
                        '(data.NoiseBank); with DATA.TRAIN_NOISY_DIR \'\' the training set is clean speech alone')
    p.add_argument('--noise-prob', default=1.0, type=float, metavar='P',
                   help='probability that a training crop gets its noise from --noise-dir')
    p.add_argument('--noise-snr', default=[0.0, 20.0], type=float, nargs=2, metavar=('LO', 'HI'),
                   help='SNR range in dB of the training crops mixed from --noise-dir')
    args, _ = p.parse_known_args(argv)
    if args.arch == 'diffuse':      # the reference's default is not in its own choices and selects the cmgan branch
        args.arch = 'cmgan'
    return args, get_config(args)


def synthetic_loader(n_batches, batch, samples, seed):
    out = []
    for i in range(n_batches):
        g = torch.Generator().manual_seed(seed + i)
        clean = 0.1 * torch.randn(batch, samples, generator=g)
        noisy = clean + 0.05 * torch.randn(batch, samples, generator=g)
        q = 0.2 + 0.7 * torch.rand(batch, generator=g)
        out.append({'audio': clean, 'noisy': noisy,
                    'labels': {'est': q, 'clean': torch.full_like(q, 0.97), 'noisy': 0.5 * q}})
    return out


def check_noise_flags(args, config):
    """the combinations of --noise-dir that cannot work, and a clean-only training set without its noise"""
    noise_dir = getattr(args, 'noise_dir', None)
    if noise_dir and args.remix_prob != 0:
        raise RuntimeError('--noise-dir takes the noise of the training crops from a noise bank, --remix-prob from the corpus: '
                           'one loader does one of the two')
    if not config.DATA.TRAIN_NOISY_DIR and (not noise_dir or getattr(args, 'noise_prob', 1.0) != 1.0):
        raise RuntimeError("DATA.TRAIN_NOISY_DIR is '': training from clean speech alone takes all its noise from a noise bank, "
                           'pass --noise-dir DIR [DIR ...] and leave --noise-prob at 1')


def device_loaders(args, config, samples):
    """main_gan.py:222-253 on the device (data.py): both corpora resident on this rank's GPU, the per-rank batch size, and the
    reference's sampling -- shuffled when there is no sampler (train) or a DistributedSampler with its defaults (both)"""
    from . import data
    dev = torch.device('cuda', args.gpu)
    rank, world = (args.rank, args.world_size) if args.distributed else (0, 1)
    noise_dir = getattr(args, 'noise_dir', None)
    check_noise_flags(args, config)
    train_set = data.DeviceDataset(config.DATA.TRAIN_CLEAN_DIR, config.DATA.TRAIN_NOISY_DIR or None, config.SAMPLE_RATE, device=dev)
    valid_set = data.DeviceDataset(config.DATA.TEST_CLEAN_DIR, config.DATA.TEST_NOISY_DIR, config.SAMPLE_RATE, device=dev)
    print('Audio signals cropped to {} seconds long'.format(config.CROP_LEN))
    # the training crops only: validation always sees the corpus' own pairs
    remix = {'remix': data.Remix(args.remix_prob, tuple(args.remix_snr))} if args.remix_prob != 0 else {}
    if noise_dir:                   # each rank holds its own bank, as it holds its own corpus
        bank = data.NoiseBank(noise_dir, config.SAMPLE_RATE, device=dev)
        print('Noise bank: {} files, {:.2f} hours, {} bytes resident'.format(len(bank.files), bank.total / config.SAMPLE_RATE / 3600.0,
                                                                             bank.nbytes))
        remix = {'bank': data.BankMix(bank, args.noise_prob, tuple(args.noise_snr))}
    train_loader = data.DeviceLoader(train_set, args.batch_size, samples, shuffle=True, rank=rank, world=world, **remix)
    valid_loader = data.DeviceLoader(valid_set, args.batch_size, samples, shuffle=args.distributed, rank=rank, world=world)
    return train_loader, valid_loader


def main_worker(gpu, ngpus_per_node, args, config):
    args.gpu = gpu
    if args.distributed:
        if args.dist_url == 'env://' and args.rank == -1:
            args.rank = int(os.environ['RANK'])
        if args.multiprocessing_distributed:
            args.rank = args.rank * ngpus_per_node + gpu
        if args.gpu is None:
            args.gpu = int(os.environ.get('LOCAL_RANK', 0))
        torch.cuda.set_device(args.gpu)
        dist.init_process_group(backend=args.dist_backend, init_method=args.dist_url, world_size=args.world_size,
                                rank=args.rank)
        dist.barrier()
    elif args.gpu is None:
        args.gpu = 0
    torch.cuda.set_device(args.gpu)
    model = TSCNet(num_channel=64, num_features=config.N_FFT // 2 + 1)
    discriminator = Discriminator(ndf=16)
    model.apply(kaiming_init)
    discriminator.apply(kaiming_init)
    model.cuda(args.gpu)
    discriminator.cuda(args.gpu)
    if args.distributed:
        args.batch_size = int(args.batch_size / args.world_size)
        attach_data_parallel(model, discriminator)
    criterion = torch.nn.MSELoss()
    optimizer = build_optimizer(args, model)
    optimizer_disc = build_optimizer(args, discriminator, lr=args.lr * 2)
    best_loss = 1e8
    if args.resume and os.path.isfile(args.resume):
        ck = torch.load(args.resume, map_location=f'cuda:{args.gpu}')
        args.start_epoch = ck['epoch']
        model.load_state_dict(strip_module_prefix(ck['gen_state_dict']))
        discriminator.load_state_dict(strip_module_prefix(ck['disc_state_dict']))
        optimizer.load_state_dict(ck['optimizer'])
        optimizer_disc.load_state_dict(ck['optimizer_disc'])
        best_loss = ck['best_loss']
    samples = config.CROP_FRAMES * config.HOP_SAMPLES * config.CROP_LEN
    if args.synthetic:
        rank = args.rank if args.distributed else 0
        train_loader = [{k: (v.cuda(args.gpu) if torch.is_tensor(v) else {a: b.cuda(args.gpu) for a, b in v.items()})
                         for k, v in b.items()} for b in synthetic_loader(args.synthetic, args.batch_size, samples, 1 + 1000 * rank)]
        valid_loader = train_loader[:1]
    elif DATASET_FACTORY is not None:
        train_loader, valid_loader = DATASET_FACTORY(args, config)
    elif all(os.path.isdir(d) for d in (config.DATA.TRAIN_CLEAN_DIR, config.DATA.TRAIN_NOISY_DIR or config.DATA.TRAIN_CLEAN_DIR,
                                        config.DATA.TEST_CLEAN_DIR, config.DATA.TEST_NOISY_DIR)):
        train_loader, valid_loader = device_loaders(args, config, samples)
    else:
        raise RuntimeError('the VoiceBank dataset / collator is outside this package: pass --synthetic N or set '
                           'speech_enhancement_amd.main_gan.DATASET_FACTORY')
    import logging
    logger = logging.getLogger(args.arch)
    if not args.distributed or args.rank == 0:
        logging.basicConfig(level=logging.INFO)
    for epoch in range(args.start_epoch, args.epochs):
        for loader in (train_loader, valid_loader):
            if hasattr(loader, 'set_epoch'):
                loader.set_epoch(epoch)
        tg, td = train_gan(train_loader, model, discriminator, criterion, optimizer, optimizer_disc, logger, epoch, args,
                           config)
        vg, vd = validate_gan(valid_loader, model, discriminator, criterion, logger, epoch, args, config)
        if not args.distributed or args.rank == 0:
            is_best = vd <= best_loss
            best_loss = min(best_loss, vd)
            pre = 'module.' if args.distributed else ''
            save_checkpoint({'epoch': epoch + 1, 'arch': args.arch,
                             'gen_state_dict': {pre + k: v for k, v in model.state_dict().items()},
                             'disc_state_dict': {pre + k: v for k, v in discriminator.state_dict().items()},
                             'optimizer': optimizer.state_dict(), 'optimizer_disc': optimizer_disc.state_dict(),
                             'best_loss': best_loss}, config.OUTPUT, is_best=is_best,
                            filename='checkpoint_{:04d}.pth.tar'.format(epoch))
            logger.info(f'Train Generator Loss: {tg:.3f}\tTrain Discriminator Loss: {td:.3f}\t'
                        f'Validation Generator Loss: {vg:.3f}\tValidation Discriminator Loss: {vd:.3f}')
    if args.distributed:
        dist.destroy_process_group()


def main(argv=None):
    args, config = parse_option(argv)
    if args.remix_prob != 0 and (args.synthetic or DATASET_FACTORY is not None):
        raise RuntimeError('--remix-prob mixes the noise of the device-resident wav folders (config.DATA.*_DIR): it cannot be '
                           'combined with --synthetic or a DATASET_FACTORY')
    if args.synthetic or DATASET_FACTORY is not None:
        if args.noise_dir:
            raise RuntimeError('--noise-dir mixes into crops of the device-resident wav folders (config.DATA.*_DIR): it cannot be '
                               'combined with --synthetic or a DATASET_FACTORY')
    else:
        check_noise_flags(args, config)
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
        warnings.warn('You have chosen to seed training.')
    if args.dist_url == 'env://' and args.world_size == -1:
        args.world_size = int(os.environ.get('WORLD_SIZE', 1))
    args.distributed = args.world_size > 1 or args.multiprocessing_distributed
    ngpus = torch.cuda.device_count()
    if args.multiprocessing_distributed:
        args.world_size = ngpus * args.world_size
        mp.spawn(main_worker, nprocs=ngpus, args=(ngpus, args, config))
    else:
        main_worker(args.gpu, ngpus, args, config)


if __name__ == '__main__':
    main()
