"""Live enhancement on a pipe: `python -m speech_enhancement_amd.stream_gan -m CKPT --cfg CFG < noisy.s16le > enhanced.s16le`.
Reads mono signed 16-bit little-endian PCM at config.SAMPLE_RATE from stdin (there is no resampler here: the input must already
be at the model's rate), pushes it through one inference.StreamEnhancer stream block by block, and writes the enhanced PCM to
stdout, flushed after every block, with the withheld tail at the end of the input.  The output lags the input by the delay
D = lookahead + fade; the first D output samples (the estimate of what came before the stream) are dropped unless --keep-delay, so
by default the output has exactly as many samples as the input and is aligned with it.  A last partial block is zero-padded.
The flags --stream-block (default 0.1 s here), --stream-window, --stream-lookahead and --stream-fade are those of inference_gan."""
import argparse
import sys

import numpy as np

from .config import get_config
from .inference import check_streaming


def parse_option(argv=None):
    from .inference_gan import add_stream_flags
    p = argparse.ArgumentParser(description='enhances s16le PCM from stdin to stdout, block by block')
    p.add_argument('--model_path', '-m', type=str, required=True, metavar='FILE')
    p.add_argument('--cfg', type=str, required=True, metavar='FILE')
    p.add_argument('--gpu', default=0, type=int)
    p.add_argument('--opts', default=None, nargs='+')
    p.add_argument('--keep-delay', action='store_true')
    add_stream_flags(p)
    p.set_defaults(stream_block=0.1)
    args, _ = p.parse_known_args(argv)
    config = get_config(args)
    rate = config.SAMPLE_RATE
    check_streaming(round(args.stream_window * rate), round(args.stream_block * rate), round(args.stream_lookahead * rate),
                    round(args.stream_fade * rate), config.HOP_SAMPLES)
    return args, config


def pcm_blocks(read, block, warn=None):
    """the byte framing: `read(n)` returns up to n bytes of s16le PCM and b'' at the end of the input (a file object's read; a pipe
    may return less than asked for, so it is called until a block is full).  Yields (samples float32 [block] in [-1, 1), count):
    count = block for every block but possibly the last, whose missing samples are zeros.  An odd trailing byte is no sample: it
    is dropped, and `warn` (default: a line on stderr) is told.  An empty input yields nothing."""
    warn = warn or (lambda msg: print(msg, file=sys.stderr))
    need = 2 * int(block)
    while True:
        buf = b''
        while len(buf) < need:
            got = read(need - len(buf))
            if not got:
                break
            buf += got
        if len(buf) & 1:
            warn('stream_gan: odd trailing byte dropped (s16le samples are two bytes)')
            buf = buf[:-1]
        if not buf:
            return
        x = np.zeros(int(block), np.float32)
        count = len(buf) // 2
        x[:count] = np.frombuffer(buf, dtype='<i2').astype(np.float32) / 32768.0
        yield x, count
        if len(buf) < need:
            return


def to_pcm(y):
    """float samples -> s16le bytes, rounded to nearest and saturated to [-32768, 32767]"""
    return np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype('<i2').tobytes()


def run(enhancer, read, write, keep_delay=False, warn=None):
    """streams read() through row 0 of `enhancer` and write()s the s16le result block by block -> samples (read, written).
    Output sample i of the stream (blocks, then the flush) carries input sample i - D; it is written if it lies in [D, D + n), or in
    [0, D + n) with keep_delay, n = the number of input samples -- known once a partial block or the end of the input is seen,
    and until then every block was full, so everything a step returns lies below D + n."""
    H, D = enhancer.H, enhancer.delay
    skip = 0 if keep_delay else D
    n = done = written = 0                                  # input samples, output samples produced, output samples written
    for x, count in pcm_blocks(read, H, warn):
        out = enhancer.push(x.reshape(1, H))[0].cpu().numpy()
        n += count
        lo, hi = max(skip - done, 0), min(H, D + n - done)
        if hi > lo:
            write(to_pcm(out[lo:hi]))
            written += hi - lo
        done += H
    if n:
        out = enhancer.flush()[0].cpu().numpy()
        lo, hi = max(skip - done, 0), min(D, D + n - done)
        if hi > lo:
            write(to_pcm(out[lo:hi]))
            written += hi - lo
    return n, written


def main(argv=None, stdin=None, stdout=None):
    args, config = parse_option(argv)
    import torch
    from .inference import load_model
    from .inference_gan import stream_enhancer
    stdin = stdin if stdin is not None else sys.stdin.buffer
    stdout = stdout if stdout is not None else sys.stdout.buffer
    device = torch.device('cuda', args.gpu)
    with torch.cuda.device(device):
        model = load_model(args.model_path, config, device)
        enhancer = stream_enhancer(args, config, model, device)

        def write(data):
            stdout.write(data)
            stdout.flush()
        n, written = run(enhancer, stdin.read, write, args.keep_delay)
    print(f'stream_gan: {n} samples in, {written} out, delay {enhancer.delay} samples, '
          f'algorithmic latency {1e3 * enhancer.latency_seconds:.1f} ms', file=sys.stderr)


if __name__ == '__main__':
    main()
