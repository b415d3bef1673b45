"""GPU tests of chunked enhancement of long recordings: the gather and assemble kernels (csrc/se_long.hip) against their definition
in include/se_hip.h restated in numpy / fp64, and inference.LongEnhancer against predict() per chunk and against the CPU oracle.

Small shapes: chunks of S = 1600 samples (17 frames) with a crossfade of V = 400; L = 4137 is no multiple of the hop, so the chunk
starts are odd and the source rows unaligned.  The elementwise bar of the assemble kernel, 8 * 2^-24 * (|a / c_a| + |b / c_b|) + 1e-12,
covers the handful of fp32 roundings of its formula (two divisions, the weight, its complement, two products, one sum: each at most
2^-24 of a term no larger than the two de-normalised chunk values)."""
import os
import types

import numpy as np
import pytest
import torch

import formula

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_, V_ = 1600, 400
CFG = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=16000)
EPS = 8 * 2.0 ** -24


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
    """the project's bar for predict() against the oracle (tests/test_model_gpu.py, test_predict_and_load_model_vs_oracle)"""
    e, bar = rms(got, ref), 2e-4 * float(np.abs(ref).max()) + 1e-5
    print(f'rms {e:.3e}  bar {bar:.3e}')
    return e < bar


def crossfade64(y, c, silent, starts, V, L):
    """the assemble rule in fp64 on the same fp32 inputs -> (out [L], |a / c_a| + |b / c_b| per sample, samples that only silent
    chunks reach)"""
    y, c = np.asarray(y, np.float64), np.asarray(c, np.float64)
    silent, starts = np.asarray(silent).astype(bool), np.asarray(starts, np.int64)
    S = y.shape[1]
    n = np.arange(L, dtype=np.int64)
    k = np.searchsorted(starts, n, side='right') - 1
    i = n - starts[k]
    assert (k >= 0).all() and (i < S).all()
    a = np.where(silent[k], 0.0, y[k, i] / c[k])
    fade = (k > 0) & (i < V)
    kp = np.maximum(k - 1, 0)
    j = np.where(fade, n - starts[kp], 0)
    assert (j < S).all()
    with np.errstate(invalid='ignore'):
        b = np.where(fade & ~silent[kp], y[kp, j] / c[kp], 0.0)
    w = np.where(fade, (i + 0.5) / V, 1.0)
    return w * a + (1.0 - w) * b, np.abs(a) + np.abs(b), silent[k] & (~fade | silent[kp])


def assert_elementwise(out, ref, mag):
    err, tol = np.abs(out.astype(np.float64) - ref), EPS * mag + 1e-12
    worst = int(np.argmax(err - tol))
    print(f'samples {out.size}  max |err| {err.max():.3e}  tightest margin at {worst}: err {err[worst]:.3e} tol {tol[worst]:.3e}')
    assert np.isfinite(out).all() and (err <= tol).all(), (worst, err[worst], tol[worst])


@pytest.mark.parametrize('L', [4137, S_ + 1])
def test_gather_copies_bits_and_normalises_per_chunk(P, L):
    from speech_enhancement_amd import ops as O
    x = signal(1, L)
    starts = P.chunk_plan(L, S_, V_)
    assert starts[-1] == L - S_ and (L != 4137 or any(s % 4 for s in starts))
    chunks, c, silent = O.chunk_gather(dev(x), dev(np.array(starts, np.int64)), S_)
    want = np.stack([x[s:s + S_] for s in starts])
    assert chunks.shape == want.shape and np.array_equal(chunks.cpu().numpy().view(np.uint32), want.view(np.uint32))
    c64 = np.sqrt(S_ / np.sum(want.astype(np.float64) ** 2, axis=1))
    rel = np.abs(c.cpu().numpy().astype(np.float64) - c64) / c64
    print('c relative error', rel.max())
    assert rel.max() <= 1e-6
    assert silent.dtype == torch.uint8 and silent.cpu().tolist() == [0] * len(starts)


def test_gather_flags_a_chunk_of_exact_zeros(P):
    from speech_enhancement_amd import ops as O
    L = 4137
    starts = P.chunk_plan(L, S_, V_)
    assert len(starts) == 4
    x = signal(2, L)
    x[starts[1]:starts[1] + S_] = 0.0                   # covers chunk 1 exactly; its neighbours keep samples outside the stretch
    chunks, c, silent = O.chunk_gather(dev(x), dev(np.array(starts, np.int64)), S_)
    assert silent.cpu().tolist() == [0, 1, 0, 0]
    c = c.cpu().numpy()
    assert c[1] == 1.0 and not chunks[1].any()
    want = np.stack([x[s:s + S_] for s in starts])
    c64 = np.sqrt(S_ / np.sum(want[[0, 2, 3]].astype(np.float64) ** 2, axis=1))
    assert (np.abs(c[[0, 2, 3]] - c64) <= 1e-6 * c64).all()


@pytest.mark.parametrize('starts,L', [([0, 100], S_ + 100), (None, 2 * S_ - V_ + 37), (None, 8003)], ids=['K2-stride-lt-V', 'K3', 'K7'])
def test_assemble_against_fp64(P, starts, L):
    from speech_enhancement_amd import ops as O
    starts = starts or P.chunk_plan(L, S_, V_)
    K = len(starts)
    assert K == {S_ + 100: 2, 2 * S_ - V_ + 37: 3, 8003: 7}[L]
    rs = np.random.RandomState(10 + K)
    y = rs.randn(K, S_).astype(np.float32)
    c = rs.uniform(0.5, 2.0, K).astype(np.float32)
    silent = np.zeros(K, np.uint8)
    if K == 7:                                          # a silent chunk between live ones: its row must not be used, whatever it holds
        silent[3] = 1
        y[3] = np.nan
    out = O.chunk_assemble(dev(y), dev(c), dev(silent), dev(np.array(starts, np.int64)), V_, L).cpu().numpy()
    ref, mag, quiet = crossfade64(y, c, silent, starts, V_, L)
    assert out.shape == (L,)
    assert_elementwise(out, ref, mag)
    assert (out[quiet] == 0.0).all() and (K != 7 or quiet.sum() > 0)


@pytest.mark.parametrize('L', [S_ + 1, 2 * S_ - V_, 2 * S_ - V_ + 1, 4137])
def test_assemble_of_gather_is_the_identity(P, L):
    from speech_enhancement_amd import ops as O
    x = signal(3, L)
    starts = dev(np.array(P.chunk_plan(L, S_, V_), np.int64))
    chunks, c, silent = O.chunk_gather(dev(x), starts, S_)
    out = O.chunk_assemble(chunks * c[:, None], c, silent, starts, V_, L).cpu().numpy()
    _, mag, _ = crossfade64((chunks * c[:, None]).cpu().numpy(), c.cpu().numpy(), silent.cpu().numpy(), starts.cpu().numpy(), V_, L)
    assert_elementwise(out, x.astype(np.float64), mag)


def test_rows_past_two_to_the_31_elements(P):
    """K * S > 2^31 (what a recording of a day and a half reaches with 4 s chunks), kept small in samples by starting a chunk at every
    sample: row offsets need 64 bits in both kernels.  Compared on the device: the rows against a strided view of the signal, and
    assemble(gather(x)) with c = 1 against x -- a row offset that wrapped would read another sample of the noise."""
    from speech_enhancement_amd import ops as O
    S, V, K = 64000, 8000, 33600
    assert K * S > 2 ** 31
    L = S + K - 1
    x = dev(signal(9, L))
    starts = torch.arange(K, dtype=torch.int64, device='cuda')
    chunks, c, silent = O.chunk_gather(x, starts, S)
    assert torch.equal(chunks, x.unfold(0, S, 1)) and not silent.any()
    tail = x[K - 1:].double()
    assert abs(float(c[K - 1]) - float(torch.sqrt(S / torch.sum(tail * tail)))) <= 1e-6 * float(c[K - 1])
    out = O.chunk_assemble(chunks, torch.ones_like(c), silent, starts, V, L)
    err = (out.double() - x.double()).abs()
    assert bool((err <= 2 * EPS * x.double().abs() + 1e-12).all()), float(err.max())


def test_batched_chunks_equal_single_chunks(P, model):
    L = 4137
    x = signal(4, L)
    enh = P.LongEnhancer(model, CFG, S_ / 16000, V_ / 16000, batch=3)
    y, c, silent, starts = enh.enhance_chunks(dev(x))
    assert enh.forwards == 2 and starts.cpu().tolist() == P.chunk_plan(L, S_, V_) and not silent.any()
    z = (y / c[:, None]).cpu().numpy()
    for k, s in enumerate(starts.cpu().tolist()):
        assert predict_bar(z[k], P.predict(model, CFG, x[s:s + S_])), k


def test_end_to_end_against_the_cpu_oracle(P, model):
    from oracle import se_oracle as Or
    L = 2 * S_ - V_ + 37
    x = signal(5, L)
    starts = P.chunk_plan(L, S_, V_)
    assert len(starts) == 3
    out = P.LongEnhancer(model, CFG, S_ / 16000, V_ / 16000, batch=8)(x)
    assert out.shape == (L,) and out.dtype == np.float32
    xt = torch.from_numpy(np.stack([x[s:s + S_] for s in starts]))
    c = torch.sqrt(S_ / torch.sum(xt ** 2, -1))
    with torch.no_grad():
        er, ei = Or.tscnet_forward(formula.formula_state('generator'), Or.compressed_stft(xt * c[:, None]), False)
        y = Or.uncompressed_istft(torch.complex(er, ei).squeeze(1).permute(0, 2, 1))
    ref, _, _ = crossfade64(y.numpy(), c.numpy(), np.zeros(3, np.uint8), starts, V_, L)
    assert predict_bar(out, ref)


def test_length_silence_and_forward_count(P, model, monkeypatch):
    calls = []
    inner = model.forward_planes
    monkeypatch.setattr(model, 'forward_planes', lambda planes: calls.append(planes.shape[0]) or inner(planes))
    # K = 3 is no multiple of the batch
    L = 2 * S_ - V_ + 37
    out = P.LongEnhancer(model, CFG, S_ / 16000, V_ / 16000, batch=2).enhance_device(signal(6, L))
    assert out.is_cuda and out.shape == (L,) and calls == [2, 1] and bool(torch.isfinite(out).all())
    # the middle 2 S samples are exact zeros: the chunks inside them are not forwarded and give exact zeros
    del calls[:]
    L = 9637
    x = signal(7, L)
    z0 = (L - 2 * S_) // 2
    x[z0:z0 + 2 * S_] = 0.0
    starts = np.array(P.chunk_plan(L, S_, V_))
    silent = (starts >= z0) & (starts + S_ <= z0 + 2 * S_)
    assert len(starts) == 8 and silent.sum() == 2
    out = P.LongEnhancer(model, CFG, S_ / 16000, V_ / 16000, batch=4)(x)
    assert out.shape == (L,) and np.isfinite(out).all()
    assert calls == [4, 2]                               # six live chunks: the two silent ones never reach the model
    _, _, quiet = crossfade64(np.zeros((8, S_)), np.ones(8), silent, starts, V_, L)
    assert quiet.sum() > S_ and (out[quiet] == 0.0).all() and np.abs(out[~quiet]).max() > 0.0


def test_evaluate_takes_a_long_enhancer(P, model):
    from speech_enhancement_amd import metrics as M
    gm = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_metrics.npz'))
    pairs = [(gm['enh_0'][:20000], gm['clean_0'][:20000])]
    enh = P.LongEnhancer(model, CFG, S_ / 16000, V_ / 16000, batch=8)
    total = M.evaluate(model, CFG, pairs, pesq=2.0, enhancer=enh)
    print('evaluate', total)
    assert total.shape == (6,) and np.isfinite(total).all() and total[0] == 2.0
    assert enh.forwards == -(-len(P.chunk_plan(20000, S_, V_)) // 8)


def test_short_recording_is_predict_bit_for_bit(P, model):
    x = signal(8, 1657)
    enh = P.LongEnhancer(model, CFG, 0.2, V_ / 16000)
    assert enh.S == 3200
    got = enh(x)
    want = P.predict(model, CFG, x)
    assert got.shape == want.shape == (1657,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('L', [1657, 1600], ids=['wrap-padded', 'hop-multiple'])
def test_predict_device_is_predict_bit_for_bit(P, model, L):
    from speech_enhancement_amd.inference import predict_device
    x = signal(8, L)
    got = predict_device(model, CFG, dev(x))
    assert got.is_cuda and got.shape == (L,)
    got, want = got.cpu().numpy(), P.predict(model, CFG, x)
    assert want.shape == (L,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
