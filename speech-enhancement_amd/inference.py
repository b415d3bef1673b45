"""inference_gan.py's model loading and per-utterance enhancement (inference_gan.py:60-100) on the HIP path.

Whole-utterance batch-1 forward exactly like the reference (InstanceNorm and attention span the utterance).  The
objective-metric loop over the enhanced audio is metrics.evaluate."""
from collections import OrderedDict

import numpy as np
import torch

from . import frontend as FE
from . import ops as O
from .generator import TSCNet
from .utils import strip_module_prefix


def load_checkpoint_into(model, path, key, device):
    """checkpoint[key] -> model (the 'module.' prefix of DDP checkpoints stripped where present), eval()"""
    checkpoint = torch.load(path, map_location=device)
    model.load_state_dict(strip_module_prefix(checkpoint[key]))
    model.eval()
    return model


def load_model(model_path, config, device=torch.device('cuda')):
    """inference_gan.py:60-72: TSCNet(64, N_FFT//2+1), checkpoint['gen_state_dict'], eval().  The reference strips
    7 characters from every key because its checkpoints always come from DDP ('module.' prefix, main_gan.py:142);
    here the prefix is stripped only where present, so single-GPU checkpoints of this package load as well."""
    model = TSCNet(num_channel=64, num_features=config.N_FFT // 2 + 1).to(device)
    return load_checkpoint_into(model, model_path, 'gen_state_dict', device)


def hop_frames(length, hop):
    """(frames, pad): the STFT frames of `length` samples and the samples missing to frames * hop, which the reference fills
    with the head of the signal (inference_gan.py:84-87)"""
    frames = int(np.ceil(length / hop))
    return frames, frames * hop - length


def spectral_forward(model, config, x, *cond, scale=None, comp='pow', **kw):
    """STFT of x [B, L] (times scale [B]) -> model.forward_planes(planes, *cond, **kw) -> iSTFT: device tensor [B, L].  Nothing
    else: de-normalising, truncating and no_grad are the caller's."""
    planes, _ = FE.stft_planes(x, config.N_FFT, config.HOP_SAMPLES, comp, scale=scale, padded=False)
    return FE.istft_planes(model.forward_planes(planes, *cond, **kw), config.N_FFT, config.HOP_SAMPLES, comp)


@torch.no_grad()
def predict_device(model, config, x):
    """inference_gan.py:75-100 on a device signal [L], result left on the device: normalise by c, wrap-pad the head of the
    signal to a multiple of the hop, STFT -> generator -> iSTFT, de-normalise, truncate."""
    noisy = x.unsqueeze(0)
    c = O.clip_scale(noisy.contiguous())
    length = noisy.size(-1)
    _, padding_len = hop_frames(length, config.HOP_SAMPLES)
    noisy = torch.cat([noisy, noisy[:, :padding_len]], dim=-1)
    est_audio = spectral_forward(model, config, noisy, scale=c) / c[:, None]
    return torch.flatten(est_audio)[:length]


def predict(model, config, noisy_signal, device=torch.device('cuda')):
    """predict_device on a host signal, result on the host"""
    noisy = torch.as_tensor(np.asarray(noisy_signal), dtype=torch.float32, device=device)
    est_audio = predict_device(model, config, noisy).cpu().numpy()
    assert len(est_audio) == noisy.size(-1), "Estimated audio and the origin audio must have the same length"
    return est_audio


def capture(step, device, restore=None):
    """step() captured into a HIP graph on `device` -> (graph, what the captured call of step returned).  All kernels are launched
    on torch's current stream, which is the capture stream inside `torch.cuda.graph`.  The sequence, the same for every graph of
    this package: two eager calls of step on a side stream that has waited for the current one (the warm-up: it raises the
    dynamic-LDS attributes, which a capture cannot), the current stream waits for the side stream, restore() when given (it undoes
    what the warm-up did to the state step advances; the captured call is recorded, not run, so the first replay starts where
    restore left the state), a synchronise, the capture, a synchronise.  Stream, synchronise and graph calls all name `device`: it need
    not be the current one."""
    with torch.no_grad(), torch.cuda.device(device):
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream(device).wait_stream(side)
        if restore is not None:
            restore()
        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
    torch.cuda.synchronize(device)
    return graph, out


class LRU(OrderedDict):
    """a mapping used as a least-recently-used cache: the key looked up last is at the end"""

    def lookup(self, key, build, limit):
        """self[key], moved to the end; a missing key is built by build() first, and entries past `limit` leave from the front"""
        if key in self:
            self.move_to_end(key)
            return self[key]
        value = self[key] = build()
        while len(self) > limit:
            self.popitem(last=False)
        return value


class Enhancer:
    """what metrics.evaluate takes as `enhancer`: enhance_device(signal) -> device tensor [length]; called, the same on the host"""

    def __call__(self, noisy_signal, *args, **kw):
        return self.enhance_device(noisy_signal, *args, **kw).cpu().numpy()


def _require_eval(model, who):
    if model.training:
        raise RuntimeError(f'{who} needs model.eval(): BatchNorm must use its running statistics')


class GraphedEnhancer(Enhancer):
    """predict() with the whole device-side pipeline (STFT, generator, iSTFT, de-normalisation) captured into HIP graphs (capture),
    one graph per LENGTH BUCKET = number of STFT frames (all lengths that pad to the same multiple of the hop share a
    graph; the reference's wrap-padding to the hop multiple (inference_gan.py:84-87) is done on the host copy, the
    clip scale c of the UNPADDED signal by one eager launch in front of the replay, so results equal predict() exactly).

    Batch-1 inference is launch-bound: ~1500 kernel launches cost ~20 ms of host time for ~10 ms of GPU work, a replayed
    graph removes the host side.  `max_graphs` bounds the cache (least recently used bucket is dropped)."""

    def __init__(self, model, config, length=None, device=torch.device('cuda'), max_graphs=8):
        self.model, self.config, self.device, self.max_graphs = model, config, device, max_graphs
        self.buckets = LRU()                  # frames -> dict(graph, static_in, c, out)
        if length is not None:
            self._bucket(hop_frames(int(length), config.HOP_SAMPLES)[0])

    def _pipeline(self, b):
        return spectral_forward(self.model, self.config, b['static_in'], scale=b['c']) / b['c'][:, None]

    def _build(self, frames):
        hop = self.config.HOP_SAMPLES
        b = {'static_in': torch.zeros(1, frames * hop, device=self.device, dtype=torch.float32),
             'c': torch.ones(1, device=self.device, dtype=torch.float32)}
        b['static_in'].normal_(0.0, 0.1)             # warm-up on non-degenerate data
        b['graph'], b['out'] = capture(lambda: self._pipeline(b), self.device)
        return b

    def _bucket(self, frames):
        return self.buckets.lookup(frames, lambda: self._build(frames), self.max_graphs)

    @torch.no_grad()
    def enhance_device(self, noisy_signal):
        """the enhanced signal as a device tensor [length], complete on the current stream: a view of the bucket's output buffer,
        valid until the next utterance of the same bucket is enhanced (metrics.evaluate scores it in place)"""
        x = np.asarray(noisy_signal, dtype=np.float32).reshape(-1)
        length = x.shape[0]
        frames, pad = hop_frames(length, self.config.HOP_SAMPLES)
        b = self._bucket(frames)
        xp = np.concatenate([x, x[:pad]]) if pad else x        # the reference's wrap-pad (head of the signal)
        b['static_in'].copy_(torch.from_numpy(xp).reshape(1, -1), non_blocking=True)
        # c = sqrt(L / sum x^2) over the UNPADDED signal: one eager launch writing the scalar the graph reads
        b['c'].copy_(O.clip_scale(b['static_in'][:, :length].contiguous() if pad else b['static_in']))
        b['graph'].replay()
        return torch.flatten(b['out'])[:length]


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


class LongEnhancer(Enhancer):
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
        _require_eval(model, 'LongEnhancer')
        self.model, self.config, self.batch, self.device = model, config, int(batch), device
        self.forwards = 0               # generator forwards issued so far

    def _whole(self, x):
        self.forwards += 1
        return predict_device(self.model, self.config, x)

    @torch.no_grad()
    def enhance_chunks(self, x):
        """x: device signal [L], L > S -> (y [K, S], c [K], silent [K], starts [K]): the enhanced chunks still scaled by c (rows of
        silent chunks are zeros), as ops.chunk_assemble takes them"""
        _require_eval(self.model, 'LongEnhancer')
        plan = chunk_plan(x.numel(), self.S, self.V, self.config.HOP_SAMPLES)
        starts = torch.tensor(plan, dtype=torch.int64).to(x.device)
        chunks, c, silent = O.chunk_gather(x, starts, self.S)
        live = torch.nonzero(silent.cpu() == 0).flatten()
        y = torch.zeros_like(chunks)
        live_dev = live.to(x.device)
        for g in range(0, live.numel(), self.batch):
            rows = live_dev[g:g + self.batch]
            self.forwards += 1
            y.index_copy_(0, rows, spectral_forward(self.model, self.config, chunks.index_select(0, rows), scale=c.index_select(0, rows)))
        return y, c, silent, starts

    @torch.no_grad()
    def enhance_device(self, noisy_signal):
        """the enhanced recording as a device tensor [length], complete on the current stream"""
        _require_eval(self.model, 'LongEnhancer')
        x = torch.as_tensor(np.asarray(noisy_signal, dtype=np.float32).reshape(-1)).to(self.device)
        if x.numel() <= self.S:
            return self._whole(x)
        y, c, silent, starts = self.enhance_chunks(x)
        return O.chunk_assemble(y, c, silent, starts, self.V, x.numel())


def check_streaming(window, block, lookahead, fade, hop=100):
    """the window W, block H, look-ahead A and crossfade V (samples) a stream accepts -> (W, H, A, V); the delay is D = A + V"""
    W, H, A, V, hop = int(window), int(block), int(lookahead), int(fade), int(hop)
    if hop < 1 or W % hop != 0 or W <= 2 * hop or W % 4 != 0:
        raise ValueError(f'stream window {W} must be a multiple of the hop ({hop}) and of 4 and longer than two hops: the STFT reflect-pads by 2 hops')
    if H < 4 or H % 4 != 0:
        raise ValueError(f'stream block {H} must be a positive multiple of 4 samples')
    if V < 1 or V > H:
        raise ValueError(f'stream fade {V} must lie in [1, block = {H}]: a fade has to end inside the block it starts in')
    if A < 0:
        raise ValueError(f'stream lookahead {A} must not be negative')
    if H + A + V > W:
        raise ValueError(f'stream block + lookahead + fade = {H + A + V} must fit into the window ({W})')
    return W, H, A, V


def stream_plan(length, block, delay):
    """offline use of a stream on a recording of `length` samples: (K, lo, hi) -- push K = ceil(length / H) blocks (the last one
    zero-padded), append the flush, and samples [lo, hi) = [D, D + length) of that concatenation (K H + D samples) are the
    enhanced recording, aligned with the input"""
    L, H, D = int(length), int(block), int(delay)
    if L < 1:
        raise ValueError(f'stream_plan: empty recording (length {L})')
    return -(-L // H), D, D + L


class StreamEnhancer(Enhancer):
    """Enhances `streams` = B live streams side by side, a block of H samples per stream and step, with a bounded delay.  Per row
    the device keeps a ring of the last W input samples, an int64 sample counter and the withheld tail of the previous estimate
    (include/se_hip.h, "streaming").  A step pushes one block per row:
      1. ops.stream_window: the block enters the ring; the window is the last W samples (zeros on the left until W have arrived),
         normalised by its own c = sqrt(r / sum x^2) over its r = min(n, W) real samples -- the statistic of the training crops;
      2. the batched eval forward LongEnhancer uses: STFT -> generator -> iSTFT of c * window;
      3. ops.stream_emit: the H samples that lie D = A + V behind the window's right edge come out, the first V of them crossfaded
         (linear, weights summing to one) with the tail the previous step withheld; the last D samples become the new tail.
    So every emitted sample was estimated with at least A samples of look-ahead (those of the crossfade with at least A + 1),
    the algorithmic latency is H + A + V samples (`latency_seconds`) plus the time of one step, and the pushed outputs followed by
    flush(), with the first D samples dropped, are the enhanced samples aligned with the input.  Nothing but the input ring and the
    tail passes from step to step -- nothing goes through the model twice --, so a step cannot poison the next.  A row whose window
    is exact zeros is still forwarded (the step has one shape, and a graph cannot branch) and comes out as exact zeros through a
    select; rows do not interact beyond the rounding of the forward's shared operand scales (eval mode: InstanceNorm is per
    sample, BatchNorm uses its running statistics).  All rows step together; a row without audio in a step is pushed zeros.

    graph=True captures the whole step into ONE HIP graph over static [B, H] input and output buffers (capture; the state is reset
    after the warm-up): push() is one copy plus one replay.  graph=False issues the same launches eagerly.  Neither path
    synchronises with the host.  The tensor push() returns is the static output buffer: valid until the next push.  Same contract
    as LongEnhancer for whole recordings: enhance_device -> device tensor [L] (streams == 1), __call__ -> numpy, so
    metrics.evaluate(..., enhancer=...) takes it; the last partial block is zero-padded, so the final windows of such an offline
    run see zeros in their look-ahead."""

    def __init__(self, model, config, window_seconds=2.0, block_seconds=0.1, lookahead_seconds=0.05, fade_seconds=0.01, streams=1,
                 device=torch.device('cuda'), graph=True):
        rate = getattr(config, 'SAMPLE_RATE', 16000)
        self.W, self.H, self.A, self.V = check_streaming(round(window_seconds * rate), round(block_seconds * rate),
                                                         round(lookahead_seconds * rate), round(fade_seconds * rate), config.HOP_SAMPLES)
        if int(streams) < 1:
            raise ValueError(f'StreamEnhancer: streams must be at least 1, got {streams}')
        _require_eval(model, 'StreamEnhancer')
        self.model, self.config, self.B, self.device, self.rate = model, config, int(streams), device, rate
        self.delay = self.A + self.V
        self.latency_seconds = (self.H + self.delay) / rate
        self.steps = 0                  # steps issued so far
        self._graph = None
        B, kw = self.B, {'device': device, 'dtype': torch.float32}
        self.ring, self.tail = torch.zeros(B, self.W, **kw), torch.zeros(B, self.delay, **kw)
        self.pos = torch.zeros(B, device=device, dtype=torch.int64)
        self._in, self._out = torch.zeros(B, self.H, **kw), torch.zeros(B, self.H, **kw)
        self._window, self._c = torch.zeros(B, self.W, **kw), torch.ones(B, **kw)
        self._silent = torch.zeros(B, device=device, dtype=torch.uint8)
        if graph:
            self._capture()

    def _step(self):
        O.stream_window(self._in, self.ring, self.pos, self._window, self._c, self._silent)
        y = spectral_forward(self.model, self.config, self._window, scale=self._c)
        O.stream_emit(y, self._c, self._silent, self.tail, self.pos, self.H, self.A, self.V, self._out)

    def _capture(self):
        def restore():                                # the warm-up advanced the state
            self.reset()
            self._in.zero_()
        self._in.normal_(0.0, 0.1)                    # warm-up on non-degenerate data
        self._graph, _ = capture(self._step, self.device, restore)

    def reset(self, rows=None):
        """forget everything the named rows (default: all) have received: counter, ring row and tail row are zeroed"""
        if rows is None:
            for t in (self.ring, self.tail, self.pos):
                t.zero_()
            return
        rows = [int(r) for r in np.atleast_1d(rows)]
        if any(r < 0 or r >= self.B for r in rows):
            raise ValueError(f'StreamEnhancer.reset: rows {rows} outside [0, {self.B})')
        idx = torch.tensor(rows, dtype=torch.int64).to(self.device, non_blocking=True)
        for t in (self.ring, self.tail, self.pos):
            t.index_fill_(0, idx, 0)

    @torch.no_grad()
    def push(self, blocks):
        """blocks [B, H] (device tensor or array; [H] with one stream) -> the device tensor [B, H] of enhanced samples that lie D
        behind them, complete on the current stream and valid until the next push"""
        _require_eval(self.model, 'StreamEnhancer')
        if not torch.is_tensor(blocks):
            blocks = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.float32))
        if blocks.numel() != self.B * self.H or blocks.dim() > 2:
            raise ValueError(f'StreamEnhancer.push: need blocks [{self.B}, {self.H}], got {tuple(blocks.shape)}')
        self._in.copy_(blocks.reshape(self.B, self.H), non_blocking=True)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._step()
        self.steps += 1
        return self._out

    def flush(self):
        """the withheld tail [B, D]: global samples [n - D, n) of the last estimate.  No forward; the state is left as it is."""
        return self.tail.clone()

    @torch.no_grad()
    def enhance_batch(self, signals):
        """up to `streams` recordings of any lengths, one per row -> list of device tensors, each of its recording's own length.
        All rows are reset first; a row whose recording has ended is pushed zeros."""
        sigs = [np.asarray(s, dtype=np.float32).reshape(-1) for s in signals]
        if not 1 <= len(sigs) <= self.B:
            raise ValueError(f'StreamEnhancer.enhance_batch: need 1 to {self.B} signals, got {len(sigs)}')
        plans = [stream_plan(s.shape[0], self.H, self.delay) for s in sigs]
        K, H = max(p[0] for p in plans), self.H
        host = np.zeros((self.B, K * H), np.float32)
        for b, s in enumerate(sigs):
            host[b, :s.shape[0]] = s
        x = torch.from_numpy(host).to(self.device)
        res = torch.empty(self.B, K * H + self.delay, device=self.device, dtype=torch.float32)
        self.reset()
        for k in range(K):
            res[:, k * H:(k + 1) * H] = self.push(x[:, k * H:(k + 1) * H])
        res[:, K * H:] = self.tail
        return [res[b, lo:hi] for b, (_, lo, hi) in enumerate(plans)]

    def enhance_device(self, noisy_signal):
        """the recording streamed through row 0 block by block, as if it had arrived live -> device tensor [length]"""
        if self.B != 1:
            raise ValueError(f'StreamEnhancer.enhance_device runs one recording on one stream; this one has {self.B} (use enhance_batch)')
        return self.enhance_batch([noisy_signal])[0]
