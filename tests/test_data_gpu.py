"""GPU tests of the dataset layer: the resampling kernel against the fp64 definition inside the fp32 summation bound, the crop
gather bit for bit against numpy indexing, the resident dataset and its loader, main_gan trained from wav folders, and the
resampling read of inference_gan.  All wavs are generated here with the stdlib `wave` module."""
import logging
import math
import os
import re
import types
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RATIOS = [(1, 3), (160, 441), (1, 2), (2, 1), (2, 3)]


@pytest.fixture(scope='module')
def D():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import data
    return data


def write_wav(path, x, sr, channels=1):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(x, dtype='<i2').tobytes())


def resample_ref(x, h, up, down):
    """y[j] = sum_i x[i] h[j down - i up + half], zero extension, fp64 -> (y, sum_i |x[i] h[..]|)"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    half = (h.size - 1) // 2
    n = x.size
    n_out = -(-n * up // down)
    k = np.arange(n_out)[:, None] * down - np.arange(n)[None, :] * up + half
    H = np.where((k >= 0) & (k < h.size), h[np.clip(k, 0, h.size - 1)], 0.0)
    return H @ x, np.abs(H) @ np.abs(x)


def speechlike(rs, n, sr):
    """a few harmonics under a slow envelope plus a noise floor, |x| < 1"""
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + rs.rand() * 6) for a, f in ((0.3, 180.0), (0.2, 360.0), (0.1, 2500.0), (0.05, 6100.0)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rs.randn(n)).clip(-0.99, 0.99)


@pytest.mark.parametrize('up,down', RATIOS)
@pytest.mark.parametrize('pcm', [True, False])
def test_resample_within_the_fp32_summation_bound(D, up, down, pcm):
    """|err| <= (ceil(ntaps / up) + 2) 2^-24 sum|h x| per sample: the fp32 summation bound of at most ceil(ntaps / up) terms in any
    order, plus one rounding each for the tap and the product.  No sample is excluded.  (Measured on an MI355X: the worst sample of the
    sixty signals sits at 0.19 of its bound.)"""
    from speech_enhancement_amd import _lib
    from speech_enhancement_amd.metrics import resample_fir
    rs = np.random.RandomState(100 * up + down)
    h = resample_fir(np.float32, up, down)
    half = 10 * max(up, down)
    assert h.size == 2 * half + 1
    tile = _lib.lib().se_resample_poly_tile(up, down, h.size)
    assert tile >= 1
    odd = -(-(2 * tile + 37) * down // up)                       # two full tiles and a ragged third
    lengths = [1, max(half // up - 1, 1), odd, 2, 3001, 777]
    if pcm:
        xs = [np.round(speechlike(rs, n, 48000) * 32767).astype(np.int16) for n in lengths]
        xs[2][:3] = (-32768, 32767, -32768)
        vals = [x.astype(np.float64) / 32768.0 for x in xs]
    else:
        xs = [(speechlike(rs, n, 48000) * 3.0).astype(np.float32) for n in lengths]
        vals = [x.astype(np.float64) for x in xs]
    ys = D.resample([torch.from_numpy(x).cuda() for x in xs], down * 1000, up * 1000)
    torch.cuda.synchronize()
    assert D.out_length(odd, up, down) % tile != 0
    terms = math.ceil(h.size / up) + 2
    for n, v, y in zip(lengths, vals, ys):
        ref, mag = resample_ref(v, h, up, down)
        y = y.cpu().numpy()
        assert y.dtype == np.float32 and y.shape == ref.shape == (D.out_length(n, up, down),)
        err, bound = np.abs(y.astype(np.float64) - ref), terms * 2.0 ** -24 * mag
        worst = int(np.argmax(err - bound))
        print(f'{up}:{down} pcm={pcm} n={n}: max err {err.max():.3e}, err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all(), (n, worst, err[worst], bound[worst])
    # a single tensor gives a single tensor, the same samples as in the batch
    one = D.resample(torch.from_numpy(xs[4]).cuda(), down * 1000, up * 1000)
    assert torch.equal(one, ys[4])
    if pcm:                                                        # int16 scaled in the kernel == the float32 of the host
        f = D.resample(torch.from_numpy(xs[2].astype(np.float32) / 32768.0).cuda(), down * 1000, up * 1000)
        assert torch.equal(f, ys[2])


def test_resample_rejects_what_it_cannot_do(D):
    from speech_enhancement_amd import _lib
    with pytest.raises(ValueError):
        D.resample(torch.zeros(100).cuda(), 16000, 33075)
    with pytest.raises(ValueError):
        D.resample([torch.zeros(10).cuda(), torch.zeros(0).cuda()], 48000, 16000)
    x = torch.zeros(64, device='cuda')
    y = torch.full((40,), 7.0, device='cuda')
    with pytest.raises(_lib.SeHipError):                           # an output that does not fit its arena
        D._resample_into(x, [64], 1, 3, y, out_offsets=[30])
    assert float(y.min()) == 7.0


def test_crop_gather_is_indexing(D):
    import ctypes as C
    from speech_enhancement_amd import _lib as L
    rs = np.random.RandomState(4)
    Lc = 1000
    lengths = [5000, Lc, 333, 1, 1001, 999]
    starts = [1234, 0, 0, 0, 1, 0]
    clean = [rs.randn(n).astype(np.float32) for n in lengths]
    noisy = [c + 0.3 * rs.randn(c.size).astype(np.float32) for c in clean]
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    ca, na = torch.from_numpy(np.concatenate(clean)).cuda(), torch.from_numpy(np.concatenate(noisy)).cuda()
    rows = torch.tensor([[o, n, s] for o, n, s in zip(offs, lengths, starts)], dtype=torch.int64).cuda()
    B = len(lengths)
    oc, on = torch.full((B, Lc), 9.0, device='cuda'), torch.full((B, Lc), 9.0, device='cuda')
    st = torch.full((B, 3), -1.0, device='cuda')
    L.call('se_crop_gather', L.ptr(ca), L.ptr(na), C.c_longlong(ca.numel()), L.ptr(rows), C.c_int(B), C.c_int(Lc), L.ptr(oc),
           L.ptr(on), L.ptr(st), L.stream())
    torch.cuda.synchronize()
    oc, on, st = oc.cpu().numpy(), on.cpu().numpy(), st.cpu().numpy().astype(np.float64)
    for b, (n, s) in enumerate(zip(lengths, starts)):
        idx = (np.arange(Lc) % n) if n < Lc else s + np.arange(Lc)
        assert np.array_equal(oc[b], clean[b][idx]) and np.array_equal(on[b], noisy[b][idx]), b
        want = [np.sum(clean[b][idx].astype(np.float64) ** 2), np.sum(noisy[b][idx].astype(np.float64) ** 2),
                np.abs(clean[b][idx]).max()]
        np.testing.assert_allclose(st[b], want, rtol=1e-5, atol=0)
    # the reference collator's construction of a tiled row
    n = 333
    tiled = np.concatenate([clean[2]] * (Lc // n) + [clean[2][:Lc % n]])
    assert np.array_equal(oc[2], tiled)
    # a row that leaves the arena is written as silence, not read
    bad = torch.tensor([[ca.numel() - 10, 2000, 0], [0, 5000, 4001]], dtype=torch.int64).cuda()
    zc, zn, zs = torch.full((2, Lc), 9.0, device='cuda'), torch.full((2, Lc), 9.0, device='cuda'), torch.full((2, 3), 9.0, device='cuda')
    L.call('se_crop_gather', L.ptr(ca), L.ptr(na), C.c_longlong(ca.numel()), L.ptr(bad), C.c_int(2), C.c_int(Lc), L.ptr(zc),
           L.ptr(zn), L.ptr(zs), L.stream())
    torch.cuda.synchronize()
    assert float(zc.abs().max()) == 0 and float(zn.abs().max()) == 0 and float(zs.abs().max()) == 0


def make_corpus(tmp_path, rs, spec, clean_name='clean', noisy_name='noisy'):
    """spec: [(name, sample rate, samples or None for an all-zero pair of 20000)] -> (clean dir, noisy dir, {name: (sr, clean, noisy)})"""
    cdir, ndir = tmp_path / clean_name, tmp_path / noisy_name
    os.makedirs(cdir)
    os.makedirs(ndir)
    raw = {}
    for name, sr, n in spec:
        if n is None:
            c = np.zeros(20000, dtype=np.int16)
            v = c.copy()
        else:
            c = np.round(speechlike(rs, n, sr) * 20000).astype(np.int16)
            v = np.clip(c + np.round(2000 * rs.randn(n)), -32768, 32767).astype(np.int16)
        write_wav(cdir / name, c, sr)
        write_wav(ndir / name, v, sr)
        raw[name] = (sr, c, v)
    return str(cdir), str(ndir), raw


def test_dataset_equals_per_file_resample(D, tmp_path):
    rs = np.random.RandomState(8)
    spec = [('a.wav', 48000, 30011), ('b.wav', 16000, 9000), ('c.wav', 48000, 5), ('d.wav', 44100, 12345), ('e.wav', 16000, 17),
            ('f.wav', 48000, 61000)]
    cdir, ndir, raw = make_corpus(tmp_path, rs, spec)
    ds = D.DeviceDataset(cdir, ndir, device='cuda:0')
    assert len(ds) == 6 and [os.path.basename(p) for p in ds.files] == sorted(raw)
    assert ds.clean.dtype == torch.float32 and ds.clean.numel() == ds.noisy.numel() == sum(ds.lengths) == ds.total
    for i, p in enumerate(ds.files):
        sr, c, v = raw[os.path.basename(p)]
        sr2, x = D.read_wav(p)
        assert sr2 == sr and np.array_equal(x, v.astype(np.float32) / 32768.0)
        got_c, got_n = ds.signal(i)
        for got, src in ((got_c, c), (got_n, v)):
            want = D.resample(torch.from_numpy(src.astype(np.float32) / 32768.0).cuda(), sr, 16000)
            assert got.shape == want.shape and torch.equal(got, want), p
    # mismatched pair: the error names the file, nothing is allocated
    write_wav(os.path.join(cdir, 'c.wav'), np.zeros(6, dtype=np.int16), 48000)
    with pytest.raises(ValueError, match='c.wav'):
        D.DeviceDataset(cdir, ndir, device='cuda:0')
    with pytest.raises(MemoryError):
        D.DeviceDataset(*make_corpus(tmp_path, rs, spec[:2], 'c2', 'n2')[:2], device='cuda:0', max_bytes=1000)


def test_loader_visits_everything_once_and_never_yields_silence(D, tmp_path):
    rs = np.random.RandomState(9)
    spec = [(f'u{k:02d}.wav', 48000 if k % 3 else 16000, int(n)) for k, n in
            enumerate([30000, 5000, 2999, 12000, 9000, 3000, 700, 20000, 4000, 3001, 15000])]
    spec.append(('zz_silent.wav', 48000, None))
    cdir, ndir, _ = make_corpus(tmp_path, rs, spec)
    ds = D.DeviceDataset(cdir, ndir, device='cuda:0')
    silent = len(ds) - 1
    Lc = 3000
    ld = D.DeviceLoader(ds, 4, Lc, shuffle=True, seed=2)
    assert len(ld) == 3
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        items = list(ld)
        keys = [k for it in items for k in it['keys']]
        assert sorted(f for f, _ in keys) == list(range(silent))          # every index once, the all-zero file never
        for it in items:
            assert it['audio'].is_cuda and it['audio'].shape == it['noisy'].shape == (len(it['keys']), Lc)
            for row, (f, s) in enumerate(it['keys']):
                c, v = ds.signal(f)
                if s < 0:
                    assert ds.lengths[f] < Lc
                    idx = torch.arange(Lc, device='cuda') % ds.lengths[f]
                    c, v = c[idx], v[idx]
                else:
                    c, v = c[s:s + Lc], v[s:s + Lc]
                assert torch.equal(it['audio'][row], c) and torch.equal(it['noisy'][row], v)
                assert float(c.abs().max()) > 0
    ld.set_epoch(0)
    first = [it['keys'] for it in ld]
    assert first == [it['keys'] for it in ld]                             # an epoch repeats itself
    ld.set_epoch(1)
    assert first != [it['keys'] for it in ld]
    # a caller's rule replaces the default one: every yielded row satisfies it, rows that cannot are dropped
    thr = float((ds.signal(0)[0][:Lc].double() ** 2).sum())
    ld2 = D.DeviceLoader(ds, 4, Lc, shuffle=False, reject=lambda st: (st[:, 0] > thr) | (st[:, 0] == 0))
    rows = [(f, float((it['audio'][r].double() ** 2).sum())) for it in ld2 for r, (f, _) in enumerate(it['keys'])]
    assert rows and all(0 < e <= thr * (1 + 1e-5) for _, e in rows)
    assert len({f for f, _ in rows}) == len(rows) < len(ds) and silent not in [f for f, _ in rows]


def test_main_gan_trains_from_wav_folders(D, tmp_path, caplog):
    from speech_enhancement_amd import main_gan, train
    rs = np.random.RandomState(10)
    spec = [(f's{k}.wav', 48000 if k % 2 else 16000, n) for k, n in enumerate([60000, 18000, 52000, 20000, 9000, 49000])]
    tc, tn, _ = make_corpus(tmp_path, rs, spec, 'train_clean', 'train_noisy')
    vc, vn, _ = make_corpus(tmp_path, rs, spec[:2], 'test_clean', 'test_noisy')
    calls = []

    def provider(clean_list, other_list):
        calls.append(len(clean_list))
        return torch.full((len(clean_list),), 0.5)

    train.set_pesq_provider(provider)
    cache = train.label_cache()
    cache.q.clear()
    out = str(tmp_path / 'out')
    caplog.set_level(logging.INFO)
    try:
        main_gan.main(['--cfg', '/dev/null', '-a', 'scp', '-b', '2', '--epochs', '1', '--crop-len', '1', '--optimizer', 'adamw',
                       '--lr', '5e-4', '--output', out, '--gpu', '0', '-p', '1', '--opts', 'DATA.TRAIN_CLEAN_DIR', tc,
                       'DATA.TRAIN_NOISY_DIR', tn, 'DATA.TEST_CLEAN_DIR', vc, 'DATA.TEST_NOISY_DIR', vn,
                       'TRAIN.SCHEDULER.CYCLE_LIMIT', '1'])      # the schedule's cycle is EPOCHS // CYCLE_LIMIT epochs: 1 // 4 = 0 by default
    finally:
        train.set_pesq_provider(None)
    ck = torch.load(os.path.join(out, 'scp', 'default', 'checkpoint_0000.pth.tar'), map_location='cpu')
    assert ck['epoch'] == 1 and all(torch.isfinite(v).all() for v in ck['gen_state_dict'].values() if v.is_floating_point())
    line = [r.getMessage() for r in caplog.records if 'Train Generator Loss' in r.getMessage()]
    assert len(line) == 1
    losses = [float(v) for v in re.findall(r'Loss: (\S+)', line[0])]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), line
    steps = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Train: [0/1]')]
    assert len(steps) == 3                                                 # 6 files, batches of 2
    files = sorted(k[1][0] for k in cache.q if k[0] == 'clean')
    assert files == list(range(6)) and all(k[0] in ('clean', 'noisy') for k in cache.q)      # crop keys reached the label cache
    assert all(isinstance(k[1], tuple) and -1 <= k[1][1] <= 60000 for k in cache.q)
    assert calls


def test_inference_read_resamples(D, tmp_path):
    from speech_enhancement_amd import inference_gan
    rs = np.random.RandomState(12)
    x48 = np.round(speechlike(rs, 24000, 48000) * 20000).astype(np.int16)
    x16 = np.round(speechlike(rs, 8000, 16000) * 20000).astype(np.int16)
    write_wav(tmp_path / 'hi.wav', x48, 48000)
    write_wav(tmp_path / 'lo.wav', x16, 16000)
    pytest.importorskip('scipy')
    cfg = types.SimpleNamespace(SAMPLE_RATE=16000)
    got = inference_gan._read(str(tmp_path / 'hi.wav'), cfg)
    want = D.resample(torch.from_numpy(x48.astype(np.float32) / 32768.0).cuda(), 48000, 16000).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (8000,) and np.array_equal(got, want)
    lo = inference_gan._read(str(tmp_path / 'lo.wav'), cfg)
    assert np.array_equal(lo, x16.astype(np.float32) / 32768.0)
