"""CPU-only tests of streaming enhancement: the sizes a stream accepts (inference.check_streaming), the new inference_gan flags,
the PCM framing of stream_gan, and the alignment arithmetic (inference.stream_plan) on a numpy restatement of the window and emit
steps of include/se_hip.h with an identity "model"."""
import io
import types

import numpy as np
import pytest

GEOMETRIES = [(1200, 400, 200, 100), (1200, 200, 0, 1), (1200, 400, 400, 400), (1300, 52, 48, 52), (1200, 208, 100, 8),
              (1600, 400, 200, 100), (32000, 1600, 800, 160)]


@pytest.fixture(scope='module')
def I():
    from speech_enhancement_amd import inference
    return inference


@pytest.mark.parametrize('W,H,A,V', GEOMETRIES)
def test_check_streaming_accepts(I, W, H, A, V):
    assert I.check_streaming(W, H, A, V, 100) == (W, H, A, V)


@pytest.mark.parametrize('W,H,A,V,hop,word', [
    (1250, 400, 200, 100, 100, 'hop'),           # W % hop != 0
    (200, 40, 0, 4, 100, 'two hops'),            # W <= 2 hop
    (1200, 402, 200, 100, 100, 'multiple of 4'),
    (1200, 0, 0, 1, 100, 'multiple of 4'),
    (1200, 400, 200, 0, 100, 'fade'),            # V < 1
    (1200, 400, 200, 401, 100, 'fade'),          # V > H
    (1200, 400, -1, 100, 100, 'lookahead'),
    (1200, 400, 701, 100, 100, 'fit'),           # H + D = W + 1
])
def test_check_streaming_refuses_and_names_the_requirement(I, W, H, A, V, hop, word):
    with pytest.raises(ValueError, match=word):
        I.check_streaming(W, H, A, V, hop)


def test_stream_enhancer_refuses_before_any_gpu_work(I, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'init', lambda *a, **k: pytest.fail('the GPU was initialised'))
    cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=16000)
    ok = types.SimpleNamespace(training=False)
    for kw in ({'window_seconds': 0.103}, {'block_seconds': 0.3, 'window_seconds': 0.2}, {'fade_seconds': 0.0},
               {'fade_seconds': 0.2}, {'lookahead_seconds': -0.1}, {'window_seconds': 0.1, 'lookahead_seconds': 0.01}, {'streams': 0}):
        with pytest.raises(ValueError):
            I.StreamEnhancer(ok, cfg, **kw)
    with pytest.raises(RuntimeError, match='eval'):
        I.StreamEnhancer(types.SimpleNamespace(training=True), cfg)


def _argv(tmp_path):
    cfg = tmp_path / 'c.yaml'
    cfg.write_text('DATA:\n  TEST_NOISY_DIR: n\n  TEST_CLEAN_DIR: c\n')
    return ['-o', 'out', '-m', 'ck.pth.tar', '--cfg', str(cfg)]


def test_cli_stream_flags_are_off_by_default(tmp_path):
    from speech_enhancement_amd import inference_gan as IG
    base, _ = IG.parse_option(_argv(tmp_path))
    assert (base.stream_block, base.stream_window, base.stream_lookahead, base.stream_fade) == (0.0, 2.0, 0.05, 0.01)
    assert IG.long_enhancer(base, None, None, None) is None                             # nothing is built, the model is not touched
    zero, _ = IG.parse_option(_argv(tmp_path) + ['--stream-block', '0'])
    assert vars(zero) == vars(base)
    a, _ = IG.parse_option(_argv(tmp_path) + ['--stream-block', '0.1', '--stream-window', '1', '--stream-lookahead', '0.02',
                                              '--stream-fade', '0.005'])
    assert (a.stream_block, a.stream_window, a.stream_lookahead, a.stream_fade) == (0.1, 1.0, 0.02, 0.005)
    rest = {k: v for k, v in vars(a).items() if not k.startswith('stream_')}
    assert rest == {k: v for k, v in vars(base).items() if not k.startswith('stream_')}
    # a window that would be refused with streaming on is not looked at with streaming off
    off, _ = IG.parse_option(_argv(tmp_path) + ['--stream-window', '0.0131'])
    assert off.stream_block == 0.0


@pytest.mark.parametrize('extra', [['--stream-block', '0.1', '--chunk-len', '4'], ['--stream-block', '-1'],
                                   ['--stream-block', '0.1', '--stream-fade', '0.2'], ['--stream-block', '0.1', '--stream-fade', '0'],
                                   ['--stream-block', '0.1', '--stream-window', '0.12'],
                                   ['--stream-block', '0.1', '--stream-window', '1.003'],
                                   ['--stream-block', '0.1', '--stream-lookahead', '-0.01']])
def test_cli_refuses_bad_stream_flags_before_any_gpu_work(tmp_path, monkeypatch, extra):
    import torch
    from speech_enhancement_amd import inference_gan as IG
    monkeypatch.setattr(IG, 'load_model', lambda *a, **k: pytest.fail('the model was loaded'))
    monkeypatch.setattr(torch.cuda, 'init', lambda *a, **k: pytest.fail('the GPU was initialised'))
    with pytest.raises(ValueError):
        IG.main(_argv(tmp_path) + extra)


def test_stream_gan_flags(tmp_path, monkeypatch):
    import torch
    from speech_enhancement_amd import stream_gan as SG
    cfg = tmp_path / 'c.yaml'
    cfg.write_text('DATA:\n  TEST_NOISY_DIR: n\n')
    a, config = SG.parse_option(['-m', 'ck', '--cfg', str(cfg)])
    assert (a.stream_block, a.stream_window, a.stream_lookahead, a.stream_fade, a.keep_delay) == (0.1, 2.0, 0.05, 0.01, False)
    assert SG.parse_option(['-m', 'ck', '--cfg', str(cfg), '--keep-delay'])[0].keep_delay
    monkeypatch.setattr(torch.cuda, 'init', lambda *a, **k: pytest.fail('the GPU was initialised'))
    with pytest.raises(ValueError):
        SG.main(['-m', 'ck', '--cfg', str(cfg), '--stream-block', '0'], stdin=io.BytesIO(), stdout=io.BytesIO())


def _blocks(data, H, chunk=None):
    from speech_enhancement_amd import stream_gan as SG
    warned = []
    src = io.BytesIO(data)
    read = src.read if chunk is None else (lambda n: src.read(min(n, chunk)))          # chunk: a pipe that returns short reads
    return list(SG.pcm_blocks(read, H, warned.append)), warned


def test_pcm_framing():
    pcm = np.array([0, 1, -1, 32767, -32768, 100, 200, 300, 400, 500, 600], dtype='<i2')
    want = pcm.astype(np.float32) / 32768.0
    # whole blocks: 8 samples = 2 blocks of 4, nothing after them
    got, warned = _blocks(pcm[:8].tobytes(), 4)
    assert [c for _, c in got] == [4, 4] and not warned
    assert np.array_equal(np.concatenate([x for x, _ in got]), want[:8]) and got[0][0].dtype == np.float32
    # a partial last block is zero-padded and says how many samples are real
    got, warned = _blocks(pcm.tobytes(), 4)
    assert [c for _, c in got] == [4, 4, 3] and not warned
    assert np.array_equal(np.concatenate([x for x, _ in got]), np.concatenate([want, [0.0]]).astype(np.float32))
    # an odd trailing byte is dropped with a warning; after whole blocks it leaves no block behind
    got, warned = _blocks(pcm.tobytes() + b'\x7f', 4)
    assert [c for _, c in got] == [4, 4, 3] and len(warned) == 1 and 'odd' in warned[0]
    assert np.array_equal(got[2][0], np.array([want[8], want[9], want[10], 0.0], np.float32))
    got, warned = _blocks(pcm[:8].tobytes() + b'\x01', 4)
    assert [c for _, c in got] == [4, 4] and len(warned) == 1
    # short reads (a pipe) frame the same blocks
    short, warned = _blocks(pcm.tobytes() + b'\x7f', 4, chunk=3)
    assert [c for _, c in short] == [4, 4, 3] and len(warned) == 1
    assert all(np.array_equal(a, b) for (a, _), (b, _) in zip(short, _blocks(pcm.tobytes(), 4)[0]))
    assert _blocks(b'', 4) == ([], [])


def test_pcm_output_saturates():
    from speech_enhancement_amd import stream_gan as SG
    out = np.frombuffer(SG.to_pcm(np.array([0.0, 0.5, -1.0, 1.0, 3.0, -3.0, 1.4 / 32768, 1.6 / 32768])), dtype='<i2')
    assert out.tolist() == [0, 16384, -32768, 32767, 32767, -32768, 1, 2]


class NumpyStream:
    """steps 1, 3 and 4 of the definition in include/se_hip.h, restated in numpy fp64 for one row, the model being the identity"""

    def __init__(self, W, H, A, V):
        self.W, self.H, self.A, self.V, self.delay = W, H, A, V, A + V
        self.ring, self.tail, self.n = np.zeros(W), np.zeros(A + V), 0

    def push(self, blocks):
        W, H, V, D = self.W, self.H, self.V, self.delay
        block = np.asarray(blocks, np.float64).reshape(H)
        self.ring[(self.n + np.arange(H)) % W] = block
        n = self.n + H
        g = n - W + np.arange(W)
        xk = np.where(g >= 0, self.ring[g % W], 0.0)
        P = np.sum(xk * xk)
        c, silent = (1.0, True) if P == 0 else (np.sqrt(min(n, W) / P), False)
        y = c * xk                                                # the identity "model"
        e = np.zeros(W) if silent else y / c
        j = np.arange(H)
        v = e[W - H - D + j]
        w = (j[:V] + 0.5) / V
        v[:V] = w * v[:V] + (1 - w) * self.tail[:V]
        out = np.where(n - H - D + j < 0, 0.0, v)
        self.tail, self.n = e[W - D:].copy(), n
        return out

    def flush(self):
        return self.tail.copy()


@pytest.mark.parametrize('W,H,A,V', GEOMETRIES[:6])
@pytest.mark.parametrize('blocks_and_rest', [(0, 1), (1, 0), (7, 0), (7, 123 % 52), (2, 3)])
def test_identity_model_returns_the_input(I, W, H, A, V, blocks_and_rest):
    """the alignment arithmetic of enhance_batch / enhance_device: K pushes, the flush, samples [D, D + L)"""
    L = blocks_and_rest[0] * H + blocks_and_rest[1]
    x = np.random.RandomState(L + W).randn(L)
    s = NumpyStream(W, H, A, V)
    K, lo, hi = I.stream_plan(L, H, s.delay)
    assert K == -(-L // H) and (lo, hi) == (s.delay, s.delay + L)
    padded = np.concatenate([x, np.zeros(K * H - L)])
    outs = [s.push(padded[k * H:(k + 1) * H]) for k in range(K)] + [s.flush()]
    got = np.concatenate(outs)
    assert got.shape == (K * H + s.delay,) and not got[:lo].any()           # the delay: what came before the stream is silence
    assert np.abs(got[lo:hi] - x).max() <= 1e-12 * max(1.0, np.abs(x).max())


def test_stream_gan_run_counts_and_aligns():
    """stream_gan.run on the numpy stream: the output has as many samples as the input, aligned; --keep-delay adds the D leading ones"""
    from speech_enhancement_amd import stream_gan as SG

    class T:                                                    # the two calls run() makes return [1, .] device tensors
        def __init__(self, a):
            self.a = np.asarray(a)

        def __getitem__(self, i):
            return self

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    for W, H, A, V in GEOMETRIES[:4]:
        for L in (1, H - 1, H, 5 * H + 123 % H, 6 * H):
            pcm = np.random.RandomState(L).randint(-20000, 20000, L).astype('<i2')
            for keep in (False, True):
                s = NumpyStream(W, H, A, V)
                enh = types.SimpleNamespace(H=H, delay=s.delay, push=lambda b: T(s.push(b)), flush=lambda: T(s.flush()))
                sink = io.BytesIO()
                n, written = SG.run(enh, io.BytesIO(pcm.tobytes()).read, sink.write, keep_delay=keep)
                got = np.frombuffer(sink.getvalue(), dtype='<i2')
                assert n == L and written == got.size == L + (s.delay if keep else 0)
                assert np.array_equal(got[-L:], pcm) and not got[:-L].any()


def test_stream_wrappers_have_no_cpu_fallback():
    import torch
    from speech_enhancement_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.SeHipError):
        ops.stream_window(z(2, 400), z(2, 1200), z(2, dtype=torch.int64))
    with pytest.raises(_lib.SeHipError):
        ops.stream_emit(z(2, 1200), torch.ones(2), z(2, dtype=torch.uint8), z(2, 300), z(2, dtype=torch.int64), 400, 200, 100)
