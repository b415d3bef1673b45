"""Epoch loops of the TSC-diffusion hybrid (core/function.py:453-622) around tsc_diffusion.tsc_diffusion_step /
tsc_diffusion_validation_loss, with the reference's signatures.

The diffusion step of every clip and its Gaussian noise are drawn on the device by the sampler's Philox generator
(csrc/se_sampler.hip: se_diffuse_draw_steps, se_diffuse_noise), keyed by `args.seed` (0 when unset) and counted by
    c2 = (epoch * iters_per_epoch + idx) mod 2^32 in training, idx in validation,
    c3 = (kind << 30) | rank, kind 0 = training noise, 1 = training steps, 2 = validation noise, 3 = validation steps,
so a resumed run continues the sequence of draws of the uninterrupted one, ranks draw from disjoint streams, and validation sees the
same (t, z) every epoch: its loss is comparable across epochs (the reference redraws from torch's global generator each time).
`criterion` and `scaler` are accepted and unused: the loss is the time-domain L1 and the arithmetic is fp32 (tsc_diffusion.py)."""
import datetime
import time

import torch

from . import tsc_diffusion as TD
from .train import _to_gpu
from .utils import AverageMeter, adjust_learning_rate


def _seed_rank(args):
    seed = getattr(args, 'seed', None)
    rank = getattr(args, 'rank', 0) if getattr(args, 'distributed', False) else 0
    return (0 if seed is None else int(seed)), max(int(rank), 0)


def train_tsc_diffusion(train_loader, model, criterion, optimizer, scaler, logger, epoch, args, config):
    """core/function.py:453-547: one epoch; returns the average loss"""
    if getattr(args, 'debug', False):
        torch.autograd.set_detect_anomaly(True)
    batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
    model.train()
    seed, rank = _seed_rank(args)
    c3 = TD.pack_counter(TD.KIND_TRAIN, rank)
    start = end = time.time()
    iters = len(train_loader)
    for idx, batch in enumerate(train_loader):
        data_time.update(time.time() - end)
        adjust_learning_rate([optimizer], epoch + idx / iters, config)
        clean, noisy = _to_gpu(batch, args)
        loss = TD.tsc_diffusion_step(model, optimizer, clean, noisy, config.NOISE_SCHEDULE, config.N_FFT, config.HOP_SAMPLES,
                                     getattr(args, 'comp_type', 'pow'), args.max_norm, seed=seed,
                                     counter=(TD.step_index(epoch, idx, iters), c3))
        losses.update(loss.item(), clean.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if idx % args.print_freq == 0 and logger is not None:
            eta = datetime.timedelta(seconds=int(batch_time.avg * (iters - idx)))
            logger.info(f'Train: [{epoch}/{args.epochs}][{idx}/{iters}]\t'
                        f'eta {eta} lr {optimizer.param_groups[0]["lr"]:.6f}\t'
                        f'time {batch_time.val:.4f} ({batch_time.avg:.4f})\t'
                        f'loss {losses.val:.4f} ({losses.avg:.4f})\t'
                        f'mem {torch.cuda.max_memory_allocated() / 2 ** 20:.0f}MB')
    if logger is not None:
        logger.info(f'EPOCH {epoch} training takes {datetime.timedelta(seconds=int(time.time() - start))}')
    return losses.avg


@torch.no_grad()
def validate_tsc_diffusion(valid_loader, model, criterion, scaler, logger, epoch, args, config):
    """core/function.py:549-622: the average loss in eval mode, on draws that do not depend on the epoch"""
    batch_time, losses = AverageMeter(), AverageMeter()
    model.eval()
    seed, rank = _seed_rank(args)
    c3 = TD.pack_counter(TD.KIND_VALID, rank)
    end = time.time()
    iters = len(valid_loader)
    for idx, batch in enumerate(valid_loader):
        clean, noisy = _to_gpu(batch, args)
        loss = TD.tsc_diffusion_validation_loss(model, clean, noisy, config.NOISE_SCHEDULE, config.N_FFT, config.HOP_SAMPLES,
                                                getattr(args, 'comp_type', 'pow'), seed=seed, counter=(idx & 0xFFFFFFFF, c3))
        losses.update(loss.item(), clean.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if idx % getattr(args, 'print_freq', 10) == 0 and logger is not None:
            logger.info(f'Test: [{idx}/{iters}]\t'
                        f'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                        f'Loss {losses.val:.4f} ({losses.avg:.4f})\t'
                        f'Mem {torch.cuda.max_memory_allocated() / 2 ** 20:.0f}MB')
    return losses.avg
