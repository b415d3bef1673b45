"""GPU tests of inference.StreamEnhancer with the generator: against the composition of its parts (windows built in numpy, the same
front-end and generator calls issued eagerly at the same batch, the emit rule in fp64), graph replay against eager launches,
silence, rows of different lengths, metrics.evaluate and the stream_gan command line driven in process.

Small shapes: W = 1600 (17 frames), H = 400, A = 200, V = 100, B = 2 rows with different signals, 7 steps: three partly filled
windows, then full ones, then the ring wraps."""
import io
import os
import types

import numpy as np
import pytest
import torch

import formula

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=16000)
W_, H_, A_, V_, B_, STEPS = 1600, 400, 200, 100, 2, 7
D_ = A_ + V_
SEC = dict(window_seconds=W_ / 16000, block_seconds=H_ / 16000, lookahead_seconds=A_ / 16000, fade_seconds=V_ / 16000)


@pytest.fixture(scope='module')
def P():
    import speech_enhancement_amd as P
    return P


@pytest.fixture(scope='module')
def model(P):
    g = P.TSCNet(64, 201)
    g.load_state_dict(formula.formula_state('generator'))
    return g.cuda().eval()


def signal(seed, L):
    return (0.1 * np.random.RandomState(seed).randn(L)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def predict_bar(got, ref):
    """the project's bar for predict() against the oracle (tests/test_model_gpu.py), the one LongEnhancer is held to"""
    e, bar = rms(got, ref), 2e-4 * float(np.abs(ref).max()) + 1e-5
    print(f'rms {e:.3e}  bar {bar:.3e}')
    return e < bar


def windows_of(blocks):
    """blocks [steps, B, H] -> (windows [steps, B, W] fp32, c [steps, B] fp32 from fp64, silent [steps, B])"""
    steps, B, H = blocks.shape
    hist = np.concatenate([np.zeros((B, W_), np.float32), blocks.transpose(1, 0, 2).reshape(B, steps * H)], axis=1)
    win = np.stack([hist[:, (k + 1) * H:(k + 1) * H + W_] for k in range(steps)])
    P = np.sum(win.astype(np.float64) ** 2, axis=-1)
    r = np.minimum((np.arange(steps) + 1) * H, W_)[:, None]
    silent = P == 0
    return win, np.where(silent, 1.0, np.sqrt(r / np.where(silent, 1.0, P))).astype(np.float32), silent


def emit_all(y, c, silent):
    """step 3 of the definition in fp64 over all steps: y [steps, B, W] (scaled by c) -> [B, steps H + D]: the outputs, then the flush"""
    steps, B, W = y.shape
    tail, outs, j = np.zeros((B, D_)), [], np.arange(H_)
    for k in range(steps):
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.where(silent[k][:, None], 0.0, y[k].astype(np.float64) / c[k].astype(np.float64)[:, None])
        v = e[:, W - H_ - D_ + j]
        w = (j[:V_] + 0.5) / V_
        v[:, :V_] = w * v[:, :V_] + (1 - w) * tail[:, :V_]
        outs.append(np.where(k * H_ - D_ + j < 0, 0.0, v))
        tail = e[:, W - D_:]
    return np.concatenate(outs + [tail], axis=1)


def compose(model, blocks):
    """the stream as the composition of its parts: windows and c in numpy, the front end and the generator eagerly at the same batch"""
    from speech_enhancement_amd import frontend as FE
    win, c, silent = windows_of(blocks)
    ys = []
    with torch.no_grad():
        for k in range(blocks.shape[0]):
            planes, _ = FE.stft_planes(dev(win[k]), CFG.N_FFT, CFG.HOP_SAMPLES, 'pow', scale=dev(c[k]), padded=False)
            ys.append(FE.istft_planes(model.forward_planes(planes), CFG.N_FFT, CFG.HOP_SAMPLES, 'pow'))
        y = torch.stack(ys).cpu().numpy()
    return emit_all(y, c, silent), silent


def stream(enh, blocks):
    """push the blocks [steps, B, H], flush -> [B, steps H + D] numpy"""
    d = dev(blocks)
    outs = [enh.push(d[k]).clone() for k in range(blocks.shape[0])]
    return torch.cat(outs + [enh.flush()], dim=1).cpu().numpy()


@pytest.fixture(scope='module')
def blocks():
    return (0.1 * np.random.RandomState(11).randn(STEPS, B_, H_) * np.array([1.0, 0.3])[None, :, None]).astype(np.float32)


@pytest.fixture(scope='module')
def eager(P, model, blocks):
    """the eager stream over the common blocks, computed once: [B, steps H + D]"""
    enh = P.StreamEnhancer(model, CFG, streams=B_, graph=False, **SEC)
    assert (enh.W, enh.H, enh.A, enh.V, enh.delay) == (W_, H_, A_, V_, D_) and enh.latency_seconds == (H_ + D_) / 16000
    out = stream(enh, blocks)
    assert enh.steps == STEPS and enh.pos.cpu().tolist() == [STEPS * H_] * B_
    out.setflags(write=False)
    return out


def test_eager_stream_against_the_composition(model, blocks, eager):
    ref, silent = compose(model, blocks)
    assert not silent.any() and eager.shape == ref.shape == (B_, STEPS * H_ + D_)
    assert not eager[:, :D_].any() and np.isfinite(eager).all()
    for b in range(B_):
        assert predict_bar(eager[b], ref[b]), b
    assert predict_bar(eager[:, STEPS * H_:], ref[:, STEPS * H_:])          # the flush on its own


@pytest.mark.parametrize('streams', [1, 2])
def test_graph_replay_equals_eager_launches(P, model, blocks, eager, streams):
    b = blocks[:, :streams]
    ref = eager if streams == B_ else stream(P.StreamEnhancer(model, CFG, streams=streams, graph=False, **SEC), b)
    enh = P.StreamEnhancer(model, CFG, streams=streams, graph=True, **SEC)
    assert enh._graph is not None and enh.pos.cpu().tolist() == [0] * streams and not enh.ring.any() and not enh.tail.any()
    out = stream(enh, b)
    diff = np.abs(out - ref).max()
    print('graph vs eager', diff, 'max |ref|', np.abs(ref).max())
    assert diff <= 2e-6 * max(1.0, np.abs(ref).max())
    assert enh.pos.cpu().tolist() == [STEPS * H_] * streams


def test_round_trip_without_a_network(P, blocks):
    """identity in place of the generator: the stream, delay-corrected, returns its input.  The bar is measured here from the front
    end alone: twice the largest error of istft(stft(c x_k)) / c over the regions of the windows that are emitted or withheld
    (the reference's own round-trip error, with a margin of 2 for the blend)."""
    from speech_enhancement_amd import frontend as FE
    stub = types.SimpleNamespace(training=False, forward_planes=lambda p: p)
    got = stream(P.StreamEnhancer(stub, CFG, streams=B_, graph=False, **SEC), blocks)
    win, c, _ = windows_of(blocks)
    worst = 0.0
    for k in range(STEPS):
        planes, _ = FE.stft_planes(dev(win[k]), CFG.N_FFT, CFG.HOP_SAMPLES, 'pow', scale=dev(c[k]), padded=False)
        back = FE.istft_planes(planes, CFG.N_FFT, CFG.HOP_SAMPLES, 'pow').cpu().numpy().astype(np.float64) / c[k][:, None]
        worst = max(worst, np.abs(back - win[k])[:, W_ - H_ - D_:].max())
    x = blocks.transpose(1, 0, 2).reshape(B_, STEPS * H_)
    err = np.abs(got[:, D_:] - x).max()
    print(f'stream round trip {err:.3e}  front end alone {worst:.3e}  bar {2 * worst:.3e}')
    assert not got[:, :D_].any() and 0 < worst < 1e-4 and err <= 2 * worst


_SILENCE = {}


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_silent_rows_and_an_all_silent_step(P, model, blocks, graph):
    """row 1 is silent for its first five blocks (its window for five steps), row 0 for the first: step 0 forwards a batch of exact
    zeros.  Silent windows give exact zeros; what follows still meets the composition bar, and row 1 is finite and non-zero from
    its onset on."""
    quiet = blocks.copy()
    quiet[:5, 1] = 0.0
    quiet[0, 0] = 0.0
    if 'ref' not in _SILENCE:
        _SILENCE['ref'] = compose(model, quiet)
    ref, silent = _SILENCE['ref']
    assert silent[:, 1].tolist() == [True] * 5 + [False] * 2 and silent[:, 0].tolist() == [True] + [False] * 6
    got = stream(P.StreamEnhancer(model, CFG, streams=B_, graph=graph, **SEC), quiet)
    assert np.isfinite(got).all()
    assert not got[:, :H_].any()                                 # the step in which both rows are silent
    assert not got[1, :5 * H_].any()                             # row 1 while its window is silent
    assert np.abs(got[1, 5 * H_:6 * H_]).max() > 0 and np.abs(got[1, 6 * H_:]).max() > 0      # finite and non-zero after the onset
    for b in range(B_):
        assert predict_bar(got[b, H_:], ref[b, H_:]), b


def test_rows_of_different_lengths_are_independent(P, model):
    x0, x1 = signal(21, 2900), signal(22, 1234)
    both = P.StreamEnhancer(model, CFG, streams=2, graph=False, **SEC)
    y0, y1 = both.enhance_batch([x0, x1])
    assert y0.is_cuda and y0.shape == (2900,) and y1.shape == (1234,) and both.steps == 8
    one = P.StreamEnhancer(model, CFG, streams=1, graph=False, **SEC)
    r0 = one.enhance_device(x0).cpu().numpy()
    r1 = one(x1)
    assert r0.shape == (2900,) and r1.shape == (1234,) and r1.dtype == np.float32 and one.steps == 8 + 4
    assert predict_bar(y0.cpu().numpy(), r0) and predict_bar(y1.cpu().numpy(), r1)
    with pytest.raises(ValueError):
        both.enhance_device(x0)
    with pytest.raises(ValueError):
        one.enhance_batch([x0, x1])
    # reset of one row: its state is zeroed, the other row keeps its own
    both.push(np.stack([x0[:H_], x1[:H_]]))
    assert both.pos.cpu().tolist() == [9 * H_] * 2 and both.ring[1].any() and both.tail[1].any()
    both.reset([1])
    assert both.pos.cpu().tolist() == [9 * H_, 0] and not both.ring[1].any() and not both.tail[1].any()
    assert both.ring[0].any() and both.tail[0].any()
    both.reset()
    assert both.pos.cpu().tolist() == [0, 0] and not both.ring.any() and not both.tail.any()


def test_evaluate_takes_a_stream_enhancer(P, model):
    from speech_enhancement_amd import metrics as M
    gm = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_metrics.npz'))
    pairs = [(gm['enh_0'][:20000], gm['clean_0'][:20000])]
    enh = P.StreamEnhancer(model, CFG, **SEC)
    total = M.evaluate(model, CFG, pairs, pesq=2.0, enhancer=enh)
    print('evaluate', total)
    assert total.shape == (6,) and np.isfinite(total).all() and total[0] == 2.0
    assert enh.steps == 20000 // H_


def test_stream_gan_in_process(P, model, tmp_path):
    from speech_enhancement_amd import stream_gan as SG
    ckpt, cfg = tmp_path / 'ck.pth.tar', tmp_path / 'c.yaml'
    torch.save({'gen_state_dict': formula.formula_state('generator')}, str(ckpt))
    cfg.write_text('DATA:\n  TEST_NOISY_DIR: n\n')
    n = 5 * H_ + 123
    pcm = np.clip(np.rint(3000 * np.random.RandomState(31).randn(n)), -32768, 32767).astype('<i2')
    argv = ['-m', str(ckpt), '--cfg', str(cfg), '--stream-window', str(W_ / 16000), '--stream-block', str(H_ / 16000),
            '--stream-lookahead', str(A_ / 16000), '--stream-fade', str(V_ / 16000)]
    sink = io.BytesIO()
    SG.main(argv, stdin=io.BytesIO(pcm.tobytes()), stdout=sink)
    assert len(sink.getvalue()) == 2 * n
    got = np.frombuffer(sink.getvalue(), dtype='<i2').astype(np.int64)
    ref = P.StreamEnhancer(model, CFG, **SEC)(pcm.astype(np.float32) / 32768.0)
    want = np.frombuffer(SG.to_pcm(ref), dtype='<i2').astype(np.int64)
    print('max |LSB| difference', np.abs(got - want).max(), 'max |out|', np.abs(want).max())
    assert np.abs(got - want).max() <= 1 and np.abs(want).max() > 0
    sink = io.BytesIO()
    SG.main(argv + ['--keep-delay'], stdin=io.BytesIO(pcm.tobytes() + b'\x00'), stdout=sink)
    kept = np.frombuffer(sink.getvalue(), dtype='<i2').astype(np.int64)
    assert kept.shape == (n + D_,) and not kept[:D_].any() and np.abs(kept[D_:] - want).max() <= 1
