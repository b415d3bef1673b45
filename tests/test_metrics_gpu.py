"""The device metrics against the reference's utils/compute_metrics.py (tests/golden/golden_metrics.npz, written by
tests/golden/make_golden_metrics.py on the CPU).

Per-frame bars: both sides are fp64, what differs is summation order and FFT against FFT.  The bar of each measure is 100 x the
deviation the reference's OWN formulas show when their FFTs are replaced by direct DFTs and their sums reversed (reorder_dev_* in
the golden file); it is not derived from the kernels.  Every frame of every pair is compared."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def M():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import metrics
    return metrics


@pytest.fixture(scope='module')
def gm():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_metrics.npz'))


def _pair(gm, i, trim=True):
    c, e = gm[f'clean_{i}'], gm[f'enh_{i}']
    if trim:                                   # wss / llr / snr / stoi take equal lengths; compute_metrics cuts to the shorter one
        n = min(c.size, e.size)
        c, e = c[:n], e[:n]
    return torch.from_numpy(c).cuda(), torch.from_numpy(e).cuda()


def _check(name, got, want, bar):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    print(f'{name}: frames {want.size}  max |err| {err.max():.3e}  bar {bar:.3e}')
    assert np.isfinite(got).all() and err.max() <= bar, (name, int(err.argmax()), err.max(), bar)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_per_frame_vectors_match_the_reference(M, gm, i):
    c, e = _pair(gm, i)
    if gm[f'clean_{i}'].size != gm[f'enh_{i}'].size:
        # the golden vectors of a pair of unequal lengths are those compute_metrics works on: cut, promoted to fp64, + spacing(1)
        b = M._Batch(*_pair(gm, i, trim=False), True)
        assert b.rows[0][8] == 1 and b.rows[0][1] == c.numel()
        w, l, s = (v[:b.rows[0][3]] for v in M._frames(b))
        _, d, cnt = M._stoi(b)
        d = d[:int(cnt[0]) - 30]
    else:
        w, l, (_, s), d = M.wss(c, e), M.llr(c, e), M.snr(c, e), M.stoi_frames(c, e)
    _check(f'wss[{i}]', w, gm[f'wss_{i}'], 100 * float(gm['reorder_dev_wss']))
    _check(f'llr[{i}]', l, gm[f'llr_{i}'], 100 * float(gm['reorder_dev_llr']))
    _check(f'snr[{i}]', s, gm[f'snr_{i}'], 100 * float(gm['reorder_dev_snr']))
    _check(f'd_interm[{i}]', d, gm[f'dinterm_{i}'], 100 * float(gm['reorder_dev_dinterm']))


def test_overall_snr_and_stoi_value(M, gm):
    c, e = _pair(gm, 0)
    overall, _ = M.snr(c, e)
    cn, en = gm['clean_0'].astype(np.float64), gm['enh_0'].astype(np.float64)
    assert overall.dtype == torch.float64 and overall.item() == pytest.approx(10 * np.log10(np.sum(cn ** 2) / np.sum((cn - en) ** 2)), abs=1e-4)
    assert M.stoi(c, e).item() == pytest.approx(float(gm['dinterm_0'].mean()), abs=100 * float(gm['reorder_dev_dinterm']))


@pytest.mark.parametrize('i', [0, 1, 2])
def test_six_tuple_matches_the_reference(M, gm, i):
    c, e = _pair(gm, i, trim=False)
    got = np.array(M.compute_metrics(c, e, 16000, 0, pesq=float(gm['pesq_stub'])))
    want = gm[f'final_{i}']
    print(f'six[{i}]: got {got}  want {want}  max |err| {np.abs(got - want).max():.3e}')
    assert got.shape == (6,) and np.abs(got - want).max() <= 5e-4, (got, want)
    assert M.compute_metrics(c, e, 16000, 0, pesq=lambda a, b: 2.5 + 0 * a.size)[0] == 2.5


def test_batch_is_bit_identical_to_one_by_one(M, gm):
    pairs = [_pair(gm, i, trim=False) for i in range(3)]
    batch = M.measures([p[0] for p in pairs], [p[1] for p in pairs])
    single = torch.cat([M.measures(c, e) for c, e in pairs])
    assert batch.shape == (3, 4) and torch.equal(batch, single)
    eq = [_pair(gm, i) for i in range(3)]
    for fn in (M.wss, M.llr, M.stoi_frames):
        many = fn([p[0] for p in eq], [p[1] for p in eq])
        assert all(torch.equal(v, fn(c, e)) for v, (c, e) in zip(many, eq)), fn.__name__
    many = M.snr([p[0] for p in eq], [p[1] for p in eq])[1]
    assert all(torch.equal(v, M.snr(c, e)[1]) for v, (c, e) in zip(many, eq))
    assert torch.equal(M.stoi([p[0] for p in eq], [p[1] for p in eq]), torch.stack([M.stoi(c, e) for c, e in eq]))


def test_short_clip_gives_nan_stoi_and_finite_frame_measures(M):
    """fewer than 30 frames after the silent-frame removal: the reference returns nan, so does the kernel (no exception)"""
    rs = np.random.RandomState(5)
    n = 12345
    t = np.arange(n) / 16000
    c = 0.2 * np.sin(2 * np.pi * 220 * t) * (0.3 + 0.7 * np.sin(2 * np.pi * 2 * t) ** 2) + 1e-4 * rs.randn(n)
    c[2000:10500] *= 0.001                                             # a long gap: about 40 of the 59 frames are silent
    e = 0.9 * c + 0.01 * rs.randn(n)
    c, e = torch.from_numpy(c.astype(np.float32)).cuda(), torch.from_numpy(e.astype(np.float32)).cuda()
    assert torch.isnan(M.stoi(c, e)).item() and M.stoi_frames(c, e).numel() == 0
    for v in (M.wss(c, e), M.llr(c, e), M.snr(c, e)[1]):
        assert v.numel() == int(n / 120 - 4) and torch.isfinite(v).all()
    six = M.compute_metrics(c, e, 16000, 0, pesq=2.5)
    assert np.isnan(six[5]) and np.isfinite(six[:5]).all()
    tiny = M.measures(c[:300], e[:300])                                # shorter than one frame: means of nothing, no fault
    assert torch.isnan(tiny).all()


def test_without_a_pesq_source_only_ssnr_and_stoi_are_numbers(M, gm, monkeypatch):
    from speech_enhancement_amd import train
    monkeypatch.setattr(train, 'have_pesq_scores', lambda: False)
    c, e = _pair(gm, 0)
    M._WARNED = False
    with pytest.warns(UserWarning, match='no PESQ source'):
        six = M.compute_metrics(c, e)
    assert np.isnan(six[:4]).all() and abs(six[4] - gm['final_0'][4]) <= 5e-4 and abs(six[5] - gm['final_0'][5]) <= 5e-4


def test_evaluate_sums_equal_one_by_one_compute_metrics(M, gm):
    import speech_enhancement_amd as S
    from speech_enhancement_amd import inference as INF
    torch.manual_seed(0)
    g = S.TSCNet(64, 201)
    g.apply(S.kaiming_init)
    g.cuda().eval()
    cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=16000)
    pairs = [(gm['enh_0'][:20000], gm['clean_0'][:20000]), (gm['enh_1'][2000:23345], gm['clean_1'][2000:23400])]
    seen = []
    total = M.evaluate(g, cfg, pairs, pesq=2.5, on_enhanced=lambda i, est: seen.append((i, tuple(est.shape), est.is_cuda)))
    assert seen == [(0, (20000,), True), (1, (21345,), True)]
    enh = INF.GraphedEnhancer(g, cfg)
    want = np.zeros(6)
    for noisy, clean in pairs:
        want += np.array(M.compute_metrics(torch.from_numpy(clean).cuda(), torch.from_numpy(enh(noisy)).cuda(), 16000, 0, pesq=2.5))
    print('evaluate', total, 'one by one', want)
    assert total.shape == (6,) and np.isfinite(total).all()
    np.testing.assert_allclose(total, want, rtol=1e-12, atol=1e-12)
    scored = M.evaluate(g, cfg, pairs, pesq=lambda c, e: 1.0 + c.size / 10000.0)        # host-side scorer: sees host copies
    assert scored[0] == pytest.approx(1.0 + 2.0 + 1.0 + 2.1345, abs=1e-12) and scored[4] == pytest.approx(want[4], abs=1e-9)
