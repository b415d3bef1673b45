"""inference_gan.py command line (flags :29-52, loop :102-162).  Enhances every wav under config.DATA.TEST_NOISY_DIR, scores it
against the file of the same name under config.DATA.TEST_CLEAN_DIR on the device (metrics.evaluate) and prints the reference's
line `pesq csig cbak covl ssnr stoi`; `--validate-epochs` does so for checkpoint_{start..end-1} and names the best epoch.
Without clean files it only enhances (and saves with --save).  Needs a wav reader (scipy.io.wavfile).
--chunk-len SEC > 0 enhances every recording in overlapping chunks of SEC seconds, --chunk-batch of them per forward, crossfaded over
--chunk-overlap seconds (inference.LongEnhancer): for recordings too long for one whole-utterance forward.  The default 0 is the
reference's whole-utterance forward.
--stream-block SEC > 0 enhances every recording as if it had arrived live, SEC seconds at a time, through a window of --stream-window
seconds with --stream-lookahead seconds withheld and a crossfade of --stream-fade seconds (inference.StreamEnhancer): the metrics
then show what streaming costs with the checkpoint at hand.  Not together with --chunk-len."""
import argparse
import glob
import os

import numpy as np
import torch

from . import metrics
from .config import get_config
from .inference import LongEnhancer, StreamEnhancer, check_chunking, check_streaming, load_model, predict


def parse_option(argv=None):
    p = argparse.ArgumentParser(description='runs GAN speech-enhancement inference')
    p.add_argument('--output', '-o', type=str, required=True)
    p.add_argument('--model_path', '-m', type=str, required=True, metavar='FILE')
    p.add_argument('--cfg', type=str, required=True, metavar='FILE')
    p.add_argument('--save', action='store_true')
    p.add_argument('--validate-epochs', action='store_true')
    p.add_argument('--start', default=None, type=int)
    p.add_argument('--end', default=None, type=int)
    p.add_argument('--gpu', default=0, type=int)
    p.add_argument('--opts', default=None, nargs='+')
    p.add_argument('--chunk-len', default=0.0, type=float, metavar='SEC')
    p.add_argument('--chunk-overlap', default=0.5, type=float, metavar='SEC')
    p.add_argument('--chunk-batch', default=8, type=int, metavar='N')
    add_stream_flags(p)
    args, _ = p.parse_known_args(argv)
    config = get_config(args)
    if args.chunk_len < 0:
        raise ValueError(f'--chunk-len must be 0 (whole utterances) or a chunk length in seconds, got {args.chunk_len}')
    if args.chunk_len > 0:
        check_chunking(round(args.chunk_len * config.SAMPLE_RATE), round(args.chunk_overlap * config.SAMPLE_RATE), config.HOP_SAMPLES)
        if args.chunk_batch < 1:
            raise ValueError(f'--chunk-batch must be at least 1, got {args.chunk_batch}')
    check_stream_flags(args, config)
    return args, config


def add_stream_flags(p):
    p.add_argument('--stream-block', default=0.0, type=float, metavar='SEC')
    p.add_argument('--stream-window', default=2.0, type=float, metavar='SEC')
    p.add_argument('--stream-lookahead', default=0.05, type=float, metavar='SEC')
    p.add_argument('--stream-fade', default=0.01, type=float, metavar='SEC')


def check_stream_flags(args, config):
    """refuses what StreamEnhancer would refuse, without touching the GPU; --stream-block 0 = off, the other flags are not looked at"""
    if args.stream_block < 0:
        raise ValueError(f'--stream-block must be 0 (off) or a block length in seconds, got {args.stream_block}')
    if args.stream_block > 0:
        if getattr(args, 'chunk_len', 0) > 0:
            raise ValueError('--stream-block and --chunk-len exclude each other: a recording is streamed or chunked, not both')
        rate = config.SAMPLE_RATE
        check_streaming(round(args.stream_window * rate), round(args.stream_block * rate), round(args.stream_lookahead * rate),
                        round(args.stream_fade * rate), config.HOP_SAMPLES)


def long_enhancer(args, config, model, device):
    """the chunked enhancer the --chunk-* flags ask for, the streaming one the --stream-* flags ask for, or None for the
    whole-utterance default"""
    if getattr(args, 'stream_block', 0) > 0:
        return stream_enhancer(args, config, model, device)
    if args.chunk_len <= 0:
        return None
    return LongEnhancer(model, config, args.chunk_len, args.chunk_overlap, args.chunk_batch, device)


def stream_enhancer(args, config, model, device):
    return StreamEnhancer(model, config, args.stream_window, args.stream_block, args.stream_lookahead, args.stream_fade, 1, device)


def _read(path, config):
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sr != config.SAMPLE_RATE:         # on the current device, with scipy's polyphase default filter (data.py), not librosa's soxr_hq
        from . import data
        _, x = data.read_wav(path)
        return data.resample(torch.from_numpy(x).cuda(), sr, config.SAMPLE_RATE).cpu().numpy()
    return x.astype(np.float32) / (32768.0 if x.dtype == np.int16 else 1.0)


def _save(args, config, path, y):
    from scipy.io import wavfile
    y = y.cpu() if torch.is_tensor(y) else y
    wavfile.write(os.path.join(args.output, os.path.basename(path)), config.SAMPLE_RATE, np.asarray(y, dtype=np.float32))


def format_metrics(avg):
    """the reference's line (inference_gan.py:142-147)"""
    return (f'pesq: {avg[0]:.3f}\t csig: {avg[1]:.3f}\t cbak: {avg[2]:.3f}\t covl: {avg[3]:.3f}\t '
            f'ssnr: {avg[4]:.3f}\t stoi: {avg[5]:.3f}')


def run_cli(args, config, build, enhance):
    """the loop of inference_gan.py:102-162, shared with inference_diffuse.  build(model_path) -> (model, enhancer), the enhancer as
    metrics.evaluate takes it (None: its whole-utterance default).  enhance(model, enhancer, x) -> the enhanced signal of one file,
    used where there are no clean files to score against."""
    os.makedirs(args.output, exist_ok=True)
    noisy_dir, clean_dir = config.DATA.TEST_NOISY_DIR, config.DATA.TEST_CLEAN_DIR
    data_paths = sorted(glob.glob(f'{noisy_dir}/*.wav'))
    num = len(data_paths)
    if not all(os.path.exists(p.replace(noisy_dir, clean_dir)) for p in data_paths) or not os.path.isdir(clean_dir):
        print(f'no clean signals under DATA.TEST_CLEAN_DIR ({clean_dir}): enhancing only, no metrics')
        model, enhancer = build(args.model_path)
        for path in data_paths:
            y = enhance(model, enhancer, _read(path, config))
            if args.save:
                _save(args, config, path, y)
        return

    def average(model_path):
        """inference_gan.py:102-127: the six metrics over the test set for one checkpoint"""
        model, enhancer = build(model_path)
        pairs = ((_read(p, config), _read(p.replace(noisy_dir, clean_dir), config)) for p in data_paths)
        save = (lambda i, est: _save(args, config, data_paths[i], est)) if args.save else None
        return metrics.evaluate(model, config, pairs, on_enhanced=save, enhancer=enhancer) / num
    if args.validate_epochs:
        best_pesq, best_epoch = 0, 0
        for epoch in range(args.start, args.end):
            avg = average(os.path.join(args.model_path, 'checkpoint_{:04d}.pth.tar'.format(epoch)))
            print('Epoch: {}'.format(epoch))
            print(format_metrics(avg))
            if avg[0] > best_pesq:
                best_pesq, best_epoch = avg[0], epoch
        print(f'Best epoch: {best_epoch}\t best PESQ: {best_pesq}')
    else:
        print(format_metrics(average(args.model_path)))


def main(argv=None):
    args, config = parse_option(argv)
    device = torch.device('cuda', args.gpu)

    def build(model_path):
        model = load_model(model_path, config, device)
        return model, long_enhancer(args, config, model, device)
    # without clean files and without --chunk-len / --stream-block: the eager predict, no graph
    run_cli(args, config, build, lambda model, enh, x: enh(x) if enh is not None else predict(model, config, x, device))


if __name__ == '__main__':
    main()
