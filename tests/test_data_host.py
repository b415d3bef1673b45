"""CPU-only tests of the dataset layer (speech-enhancement_amd/data.py): the resampling filter and formula against scipy, the
sampler order against torch's DistributedSampler, the crop plan against an independent restatement, the wav reader, and the choice
of loaders in main_gan -- the device work is stubbed out."""
import os
import random
import wave

import numpy as np
import pytest
import torch

RATIOS = [(1, 3), (160, 441), (1, 2), (2, 1), (2, 3)]


@pytest.fixture(scope='module')
def D():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import data
    return data


def write_wav(path, x, sr, channels=1):
    """x: int16 [n] or [n, channels]"""
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


def test_taps_are_scipys_default(D):
    signal = pytest.importorskip('scipy.signal')
    from speech_enhancement_amd.metrics import resample_fir
    for up, down in ((1, 3), (160, 441)):
        half = 10 * max(up, down)
        ref = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=('kaiser', 5.0)) * up
        np.testing.assert_allclose(resample_fir(np.float64, up, down), ref, rtol=1e-12, atol=1e-16)
        h32 = resample_fir(np.float32, up, down)
        assert h32.dtype == np.float32 and h32.size == 2 * half + 1
        np.testing.assert_allclose(h32, ref, rtol=1e-6, atol=1e-9)
    assert resample_fir(np.float32, 160, 441).size == 8821


def test_formula_is_resample_poly(D):
    signal = pytest.importorskip('scipy.signal')
    from speech_enhancement_amd.metrics import resample_fir
    rs = np.random.RandomState(11)
    for up, down in RATIOS:
        for n in (1, 7, 1000, 1531):
            x = rs.randn(n)
            y, _ = resample_ref(x, resample_fir(np.float64, up, down), up, down)
            ref = signal.resample_poly(x, up, down)
            assert y.shape == ref.shape == (D.out_length(n, up, down),)
            np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12)


def test_ratio_and_tables(D):
    assert D.ratio(48000, 16000) == (1, 3) and D.ratio(44100, 16000) == (160, 441) and D.ratio(8000, 16000) == (2, 1)
    with pytest.raises(ValueError):
        D.ratio(16000, 11025 * 3)                  # 640:1323
    x = torch.zeros(4)
    assert D.resample(x, 16000, 16000) is x        # equal rates: the input, no device needed
    from speech_enhancement_amd._lib import SeHipError
    with pytest.raises(SeHipError):
        D.resample(torch.zeros(100), 48000, 16000)     # a CPU tensor: no fallback
    utt, tiles, n_out = D.resample_tables([1, 3000, 3073 * 3], 1, 3, 1024)
    assert n_out.tolist() == [1, 1000, 3073]
    assert utt.tolist() == [[0, 1, 0], [1, 3000, 1], [3001, 9219, 1001]]
    assert tiles.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1024], [2, 2048], [2, 3072]] and tiles.dtype == np.int32
    lib = __import__('speech_enhancement_amd')._lib.lib()
    for up, down in RATIOS:
        assert lib.se_resample_poly_tile(up, down, 20 * max(up, down) + 1) == 1024
    assert lib.se_resample_poly_tile(1, 441, 8821) >= 1 and lib.se_resample_poly_tile(1, 3, 60) == 0


@pytest.mark.parametrize('world', [1, 2, 3])
def test_index_order_is_distributed_samplers(D, world):
    from torch.utils.data import DistributedSampler
    N = 17

    class DS(list):
        lengths = [100] * N
    ds = DS(range(N))
    for shuffle in (True, False):
        for seed in (0, 5):
            for rank in range(world):
                ref = DistributedSampler(range(N), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
                ld = D.DeviceLoader(ds, 4, 50, shuffle, seed=seed, rank=rank, world=world)
                for epoch in (0, 3):
                    ref.set_epoch(epoch)
                    ld.set_epoch(epoch)
                    assert ld.indices() == list(ref)
                    assert len(ld) == -(-len(list(ref)) // 4)
    g = torch.Generator()
    g.manual_seed(5 + 3)
    ld = D.DeviceLoader(ds, 4, 50, True, seed=5)
    ld.set_epoch(3)
    assert ld.indices() == torch.randperm(N, generator=g).tolist()
    assert world > 1 or len(set(ld.indices())) == N
    # more replicas than samples: the sampler wraps more than once
    few = DS(range(2))
    for rank in range(5):
        ref = DistributedSampler(range(2), num_replicas=5, rank=rank, shuffle=True, seed=1)
        assert D.DeviceLoader(few, 1, 50, True, seed=1, rank=rank, world=5).indices() == list(ref)


class HostDataset:
    """lengths + host signals: what the crop plan needs of a DeviceDataset"""

    def __init__(self, signals):
        self.signals = signals
        self.lengths = [len(s) for s in signals]

    def __len__(self):
        return len(self.signals)


def host_loader(D, ds, *args, **kwargs):
    """a DeviceLoader whose one device step (the gather launch) is numpy; everything else is the product code"""
    launches = []

    class Gathered:
        def __init__(self, clean, stats):
            self.clean, self.noisy, self._stats = torch.from_numpy(clean), torch.from_numpy(clean * 2), stats

        def stats(self):
            return self._stats

    class Loader(D.DeviceLoader):
        def _gather(self, files, starts):
            Lc = self.crop_samples
            rows = [ds.signals[f][s:s + Lc] if s >= 0 else np.resize(ds.signals[f], Lc) for f, s in zip(files, starts)]
            clean = np.stack(rows).astype(np.float32)
            launches.append((list(files), list(starts)))
            return Gathered(clean, np.stack([(clean ** 2).sum(1), (4 * clean ** 2).sum(1), np.abs(clean).max(1)], 1))

    ld = Loader(ds, *args, **kwargs)
    ld.launches = launches
    return ld


def plan_restated(lengths, order, batch, Lc, rng, rejected):
    """the crop plan in plain Python: rejected(file, start) -> bool.  Returns the yielded key lists.  The loader launches batch
    i + 1 before it judges batch i, so the first draws of batch i + 1 precede the redraws of batch i in the stream."""
    def first(files):
        return [rng.randint(0, lengths[f] - Lc) if lengths[f] >= Lc else -1 for f in files]

    def judge(files, starts):
        starts = list(starts)
        attempts = {r: 1 for r in range(len(files))}
        alive = {r: not rejected(files[r], starts[r]) for r in range(len(files))}
        while True:
            again = [r for r in range(len(files)) if not alive[r] and lengths[files[r]] >= Lc and attempts[r] < 10]
            if not again:
                break
            for r in again:                       # one pass: every draw of the pass first, in batch order
                starts[r] = rng.randint(0, lengths[files[r]] - Lc)
            for r in again:
                attempts[r] += 1
                alive[r] = not rejected(files[r], starts[r])
        return [(files[r], starts[r]) for r in range(len(files)) if alive[r]]

    out, pending = [], None
    for i in range(0, len(order), batch):
        files = order[i:i + batch]
        cur = (files, first(files))
        if pending is not None:
            out.append(judge(*pending))
        pending = cur
    if pending is not None:
        out.append(judge(*pending))
    return [k for k in out if k]


def test_crop_plan_equals_restatement(D):
    Lc = 64
    rs = np.random.RandomState(3)
    lengths = [200, 64, 30, 500, 1, 90, 64, 333, 40, 1000, 65]
    sig = [(0.01 * rs.randn(n)).astype(np.float32) for n in lengths]
    sig[3][:] = 0.01
    sig[3][::50] = 1.0              # a spike in every crop: ten attempts, then dropped
    sig[9][:500] = 1.0              # a spike in most crops: redrawn until one lies in the tail
    sig[8][5] = 1.0                 # a tiled row with a spike: dropped at once
    sig[6][:] = 0.0                 # silence of exactly L samples: the default rule drops it after ten identical draws
    ds = HostDataset(sig)
    spike = lambda st: st[:, 2] > 0.5

    def rejected_spike(f, s):
        crop = sig[f][s:s + Lc] if s >= 0 else np.resize(sig[f], Lc)
        return bool(np.abs(crop).max() > 0.5)

    def rejected_zero(f, s):
        crop = sig[f][s:s + Lc] if s >= 0 else np.resize(sig[f], Lc)
        return bool((crop ** 2).sum() == 0)

    for reject, restated in ((spike, rejected_spike), (None, rejected_zero)):
        for epoch in (0, 1):
            ld = host_loader(D, ds, 4, Lc, True, seed=7, rank=0, world=1, reject=reject)
            ld.set_epoch(epoch)
            items = list(ld)
            want = plan_restated(lengths, ld.indices(), 4, Lc, D.crop_rng(7, epoch, 0), restated)
            assert [it['keys'] for it in items] == want
            seen = [f for it in items for f, _ in it['keys']]
            if reject is spike:
                assert 3 not in seen and 8 not in seen and 9 in seen and 6 in seen
                assert sum(launch[0].count(3) for launch in ld.launches) == 10      # ten attempts, then dropped
                assert sum(launch[0].count(8) for launch in ld.launches) == 1
            else:
                assert 6 not in seen and sorted(seen) == [f for f in range(len(lengths)) if f != 6]
            for it in items:
                assert it['audio'].shape == it['noisy'].shape == (len(it['keys']), Lc)
                for row, (f, s) in enumerate(it['keys']):
                    assert (s == -1) == (lengths[f] < Lc) and (s == -1 or 0 <= s <= lengths[f] - Lc)
                    crop = sig[f][s:s + Lc] if s >= 0 else np.resize(sig[f], Lc)
                    assert np.array_equal(it['audio'][row].numpy(), crop) and np.array_equal(it['noisy'][row].numpy(), 2 * crop)
    # two epochs and two ranks draw from different streams; the same (seed, epoch, rank) repeats itself
    a, b = D.crop_rng(7, 0, 0), D.crop_rng(7, 0, 0)
    assert [a.random() for _ in range(4)] == [b.random() for _ in range(4)]
    assert len({D.crop_rng(*k).random() for k in ((7, 0, 0), (7, 1, 0), (7, 0, 1), (8, 0, 0))}) == 4
    # length == L draws randint(0, 0): a draw is consumed, the start is 0
    ld = host_loader(D, HostDataset([sig[1]]), 1, Lc, False)
    assert [it['keys'] for it in ld] == [[(0, 0)]]
    # the tiling rule of the collator
    assert np.array_equal(np.resize(sig[2], Lc), np.concatenate([sig[2]] * (Lc // 30) + [sig[2][:Lc % 30]]))
    assert random.Random(1).randint(0, 0) == 0


def test_read_wav_pcm16(D, tmp_path):
    rs = np.random.RandomState(0)
    mono = rs.randint(-32768, 32768, size=1000).astype(np.int16)
    mono[:2] = (-32768, 32767)
    write_wav(tmp_path / 'm.wav', mono, 48000)
    sr, x = D.read_wav(str(tmp_path / 'm.wav'))
    assert sr == 48000 and x.dtype == np.float32 and np.array_equal(x, mono.astype(np.float32) / 32768.0)
    assert D._wav_info(str(tmp_path / 'm.wav')) == (48000, 1000)
    stereo = rs.randint(-32768, 32768, size=(500, 2)).astype(np.int16)
    write_wav(tmp_path / 's.wav', stereo, 16000, channels=2)
    sr, x = D.read_wav(str(tmp_path / 's.wav'))
    assert sr == 16000 and x.shape == (500,) and x.dtype == np.float32
    np.testing.assert_allclose(x, (stereo.astype(np.float64) / 32768.0).mean(1), rtol=0, atol=2 ** -24)
    wavfile = pytest.importorskip('scipy.io.wavfile')
    f = (0.5 * rs.randn(300, 2)).astype(np.float32)
    wavfile.write(str(tmp_path / 'f.wav'), 22050, f)                       # IEEE float: not the stdlib's format
    sr, x = D.read_wav(str(tmp_path / 'f.wav'))
    assert sr == 22050 and np.allclose(x, f.mean(1), atol=1e-7)


def test_main_gan_chooses_the_device_loader(D, tmp_path, monkeypatch):
    from speech_enhancement_amd import main_gan as MG
    built = []

    class FakeSet:
        def __init__(self, clean_dir, noisy_dir, sample_rate=16000, device=None, max_bytes=None):
            self.args = (clean_dir, noisy_dir, sample_rate, device)

    class FakeLoader:
        def __init__(self, dataset, batch_size, crop_samples, shuffle, seed=0, rank=0, world=1, reject=None):
            self.dataset, self.geom, self.epochs = dataset, (batch_size, crop_samples, shuffle, seed, rank, world), []
            built.append(self)

        def set_epoch(self, e):
            self.epochs.append(e)

    class Net:
        def apply(self, fn):
            pass

        def cuda(self, gpu):
            return self

    class Done(Exception):
        pass

    def stop(train_loader, *a, **k):
        raise Done(train_loader)

    monkeypatch.setattr(D, 'DeviceDataset', FakeSet)
    monkeypatch.setattr(D, 'DeviceLoader', FakeLoader)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(MG, 'TSCNet', lambda **k: Net())
    monkeypatch.setattr(MG, 'Discriminator', lambda **k: Net())
    monkeypatch.setattr(MG, 'build_optimizer', lambda *a, **k: None)
    monkeypatch.setattr(MG, 'train_gan', stop)
    dirs = [str(tmp_path / n) for n in ('train_clean', 'train_noisy', 'test_clean', 'test_noisy')]
    opts = ['--opts', 'DATA.TRAIN_CLEAN_DIR', dirs[0], 'DATA.TRAIN_NOISY_DIR', dirs[1], 'DATA.TEST_CLEAN_DIR', dirs[2],
            'DATA.TEST_NOISY_DIR', dirs[3]]
    argv = ['--cfg', '/dev/null', '-a', 'scp', '-b', '6', '--crop-len', '2', '--epochs', '5', '--start-epoch', '3', '--gpu', '0',
            '--output', str(tmp_path / 'out')] + opts
    for d in dirs[:3]:
        os.makedirs(d)
    with pytest.raises(RuntimeError) as e:                # one directory missing: the message of before, word for word
        MG.main(argv)
    assert str(e.value) == ('the VoiceBank dataset / collator is outside this package: pass --synthetic N or set '
                            'speech_enhancement_amd.main_gan.DATASET_FACTORY') and not built
    os.makedirs(dirs[3])
    with pytest.raises(Done) as e:
        MG.main(argv)
    train, valid = built
    assert e.value.args[0] is train
    assert train.dataset.args == (dirs[0], dirs[1], 16000, torch.device('cuda', 0))
    assert valid.dataset.args == (dirs[2], dirs[3], 16000, torch.device('cuda', 0))
    assert train.geom == (6, 160 * 100 * 2, True, 0, 0, 1) and valid.geom == (6, 32000, False, 0, 0, 1)
    assert train.epochs == [3] and valid.epochs == [3]
    # a factory keeps its precedence over the directories
    built.clear()
    monkeypatch.setattr(MG, 'DATASET_FACTORY', lambda args, config: (['factory'], ['factory']))
    with pytest.raises(Done) as e:
        MG.main(argv)
    assert e.value.args[0] == ['factory'] and not built
    # the per-rank batch size and rank / world of a distributed run
    args, config = MG.parse_option(argv)
    args.distributed, args.rank, args.world_size, args.batch_size = True, 1, 2, 3
    MG.device_loaders(args, config, 16000)
    assert built[0].geom == (3, 16000, True, 0, 1, 2) and built[1].geom == (3, 16000, True, 0, 1, 2)
