"""CPU-only tests of noise remixing in the dataset layer (speech-enhancement_amd/data.py): the C ABI of se_crop_gather_mix, the
Remix value class, the host draws of the noise stream, the loader's key and redraw plan with the device launch stubbed out, and the
two flags of main_gan."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def D():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import data
    return data


def test_library_exports_and_header_declare_the_mixed_gather(D):
    from speech_enhancement_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, 'se_crop_gather_mix') and hasattr(lib, 'se_crop_gather_mix_workspace_bytes')
    header = open(os.path.join(ROOT, 'include', 'se_hip.h')).read()
    assert re.search(r'^#define SE_MIX_CHUNK 4096$', header, re.M)
    assert re.search(r'^size_t se_crop_gather_mix_workspace_bytes\(int B, int L\);', header, re.M)
    assert re.search(r'^int se_crop_gather_mix\(const float\* clean_arena, const float\* noisy_arena, long long arena_total,', header, re.M)
    assert D.MIX_CHUNK == 4096


def test_workspace_query(D):
    from speech_enhancement_amd import _lib
    q = _lib.lib().se_crop_gather_mix_workspace_bytes
    assert q.restype is C.c_size_t
    for B, Lc in ((1, 1), (3, 4096), (3, 4097), (16, 32000)):
        assert q(B, Lc) == B * math.ceil(Lc / 4096) * 16 == 16 * B * D.mix_chunks(Lc)
    for B, Lc in ((0, 100), (-1, 100), (4, 0), (4, -5), (0, 0)):
        assert q(B, Lc) == 0


def test_null_and_bad_sizes_are_errors_not_launches(D):
    """the argument checks come before any device call: they can be exercised without a GPU"""
    from speech_enhancement_amd import _lib
    with pytest.raises(_lib.SeHipError, match='null operand'):
        _lib.call('se_crop_gather_mix', None, None, 10, None, None, 1, 1, None, None, None, None, None, 16, None)
    one = C.c_void_p(8)                          # never dereferenced: the size check fails first
    with pytest.raises(_lib.SeHipError, match='bad sizes'):
        _lib.call('se_crop_gather_mix', one, one, 10, one, one, 0, 16, one, one, one, one, one, 16, None)
    with pytest.raises(_lib.SeHipError, match='workspace'):
        _lib.call('se_crop_gather_mix', one, one, 10, one, one, 2, 4097, one, one, one, one, one, 63, None)


def test_remix_validation(D):
    r = D.Remix(0.25, (-5, 15))
    assert r.prob == 0.25 and r.snr_db == (-5.0, 15.0)
    assert D.Remix(0.0).snr_db == (0.0, 20.0) and D.Remix(1, (3, 3)).prob == 1.0
    for prob in (-0.01, 1.01, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            D.Remix(prob, (0, 20))
    for snr in ((5, 4), (float('nan'), 3), (0, float('inf')), (float('-inf'), 0)):
        with pytest.raises(ValueError):
            D.Remix(0.5, snr)

    class DS(list):
        lengths = [100] * 4
    with pytest.raises(TypeError):
        D.DeviceLoader(DS(range(4)), 2, 50, True, remix=0.5)
    assert D.DeviceLoader(DS(range(4)), 2, 50, True).remix is None


def test_draw_mix_is_a_function_of_seed_epoch_rank(D):
    lengths = [200, 64, 30, 500, 1, 90, 64, 333]
    files = [3, 1, 0, 7, 2, 5, 4, 6, 3, 3]
    Lc = 64
    half = D.Remix(0.5, (-5, 15))
    a = D.draw_mix(files, lengths, Lc, D.mix_rng(7, 2, 1), half)
    assert a == D.draw_mix(files, lengths, Lc, D.mix_rng(7, 2, 1), half)
    assert len(a) == len(files)
    for other in ((7, 3, 1), (7, 2, 0), (8, 2, 1)):
        assert a != D.draw_mix(files, lengths, Lc, D.mix_rng(*other), half)
    none = D.draw_mix(files, lengths, Lc, D.mix_rng(7, 2, 1), D.Remix(0.0, (-5, 15)))
    every = D.draw_mix(files, lengths, Lc, D.mix_rng(7, 2, 1), D.Remix(1.0, (-5, 15)))
    assert none == [None] * len(files) and all(m is not None for m in every)
    # the draws do not depend on prob: a mixed row of prob = 0.5 is the row of prob = 1
    assert any(m is not None for m in a) and any(m is None for m in a)
    assert all(m is None or m == e for m, e in zip(a, every))
    many = D.draw_mix(list(range(8)) * 50, lengths, Lc, D.mix_rng(0, 0, 0), D.Remix(1.0, (-5, 15)))
    assert {j for j, _, _ in many} == set(range(8))                       # every file serves as noise, a row's own included
    assert any(j == f for (j, _, _), f in zip(many, list(range(8)) * 50))
    for j, s, snr in many:
        assert (s == -1) if lengths[j] < Lc else (0 <= s <= lengths[j] - Lc)
        assert -5 <= snr <= 15
    assert {s for j, s, _ in many if lengths[j] == Lc} == {0}
    assert max(s for j, s, _ in many if j == 3) > 300 and min(s for j, s, _ in many if j == 3) < 100
    # the restatement of the stream: u, j, [start], snr per row
    rng = D.mix_rng(7, 2, 1)
    for got in a:
        u, j = rng.random(), rng.randrange(len(lengths))
        s = rng.randint(0, lengths[j] - Lc) if lengths[j] >= Lc else -1
        snr = rng.uniform(-5, 15)
        assert got == ((j, s, snr) if u < 0.5 else None)
    assert D.mix_rng(7, 2, 1).random() != D.crop_rng(7, 2, 1).random()


class HostDataset:
    def __init__(self, signals, noise):
        self.signals, self.noise = signals, noise
        self.lengths = [len(s) for s in signals]

    def __len__(self):
        return len(self.signals)


def host_loader(D, ds, *args, **kwargs):
    """a DeviceLoader whose device steps (both gather launches) are numpy; everything else is the product code.  The stub mixes at
    scale 1 and reports scale 0 (a fallback) for a silent noise crop, as the kernel does."""
    launches = []

    def crop(x, s, Lc):
        return x[s:s + Lc] if s >= 0 else np.resize(x, Lc)

    class Gathered:
        def __init__(self, clean, noisy, scale):
            self.clean, self.noisy, self.scale = torch.from_numpy(clean), torch.from_numpy(noisy), scale

        def stats(self):
            c, v = self.clean.numpy().astype(np.float64), self.noisy.numpy().astype(np.float64)
            return np.stack([(c ** 2).sum(1), (v ** 2).sum(1), np.abs(c).max(1)], 1)

    class Loader(D.DeviceLoader):
        def _gather(self, files, starts):
            return self._gather_mix(files, starts, [None] * len(files))

        def _gather_mix(self, files, starts, mix):
            Lc = self.crop_samples
            clean = np.stack([crop(ds.signals[f], s, Lc) for f, s in zip(files, starts)]).astype(np.float32)
            noise, scale = [], np.zeros(len(files), dtype=np.float32)
            for r, (f, s, m) in enumerate(zip(files, starts, mix)):
                d = crop(ds.noise[f], s, Lc)
                if m is not None and np.any(crop(ds.noise[m[0]], m[1], Lc)) and np.any(clean[r]):
                    d, scale[r] = crop(ds.noise[m[0]], m[1], Lc), 1.0
                noise.append(d)
            launches.append((list(files), list(starts), list(mix)))
            return Gathered(clean, clean + np.stack(noise).astype(np.float32), scale)

    ld = Loader(ds, *args, **kwargs)
    ld.launches = launches
    return ld


def test_loader_plan_keys_and_streams(D):
    """order and crop starts with remix on are those with remix off; every launch carries one noise tuple per row, a redraw pass a
    fresh one; a mixed row's key is its 5-tuple, a row the launch did not mix keeps the plain pair"""
    Lc = 64
    rs = np.random.RandomState(5)
    lengths = [200, 64, 30, 500, 1, 90, 64, 333, 40, 1000, 65]
    sig = [(0.01 * rs.randn(n)).astype(np.float32) for n in lengths]
    noise = [(0.003 * rs.randn(n)).astype(np.float32) for n in lengths]
    sig[9][:700] = 1.0                          # a spike in most crops of file 9: redrawn until one lies in the tail
    silent = (2, 5, 8)                          # silent noise sources: rows that draw one fall back
    for f in silent:
        noise[f][:] = 0.0
    ds = HostDataset(sig, noise)
    spike = lambda st: st[:, 2] > 0.5
    redraws, lens = 0, set()
    for epoch in (0, 1):
        plain = host_loader(D, ds, 4, Lc, True, seed=7, reject=spike)
        mixed = host_loader(D, ds, 4, Lc, True, seed=7, reject=spike, remix=D.Remix(1.0, (0, 15)))
        off = host_loader(D, ds, 4, Lc, True, seed=7, reject=spike, remix=D.Remix(0.0, (0, 15)))
        for ld in (plain, mixed, off):
            ld.set_epoch(epoch)
        p_items, m_items, o_items = list(plain), list(mixed), list(off)
        assert [[k[:2] for k in it['keys']] for it in m_items] == [it['keys'] for it in p_items] == [it['keys'] for it in o_items]
        assert [(f, s) for f, s, _ in mixed.launches] == [(f, s) for f, s, _ in plain.launches]      # the crop stream is untouched
        redraws += len(mixed.launches) - len(mixed)
        # the mix stream restated: first draws of batch i + 1 precede the redraw draws of batch i, as in the crop stream
        mrng = D.mix_rng(7, epoch, 0)
        for files, _, mix in mixed.launches:
            assert mix == D.draw_mix(files, lengths, Lc, mrng, D.Remix(1.0, (0, 15)))
        last = {}
        for files, starts, mix in mixed.launches:
            for f, s, m in zip(files, starts, mix):
                last[f] = (s, m)                # the final attempt of a file is the one that was kept
        for it, po in zip(m_items, o_items):
            assert torch.equal(it['audio'], po['audio'])
            for row, key in enumerate(it['keys']):
                s, m = last[key[0]]
                assert key[1] == s
                if m[0] in silent:                   # silent noise: the stub (like the kernel) reports scale 0
                    assert key == (key[0], s) and torch.equal(it['noisy'][row], po['noisy'][row])
                else:
                    assert key == (key[0], s, m[0], m[1], m[2]) and len(key) == 5
                    want = it['audio'][row].numpy() + (noise[m[0]][m[1]:m[1] + Lc] if m[1] >= 0 else np.resize(noise[m[0]], Lc))
                    assert np.array_equal(it['noisy'][row].numpy(), want)
        lens |= {len(k) for it in m_items for k in it['keys']}
        assert all(len(k) == 2 for it in o_items for k in it['keys'])
    assert lens == {2, 5}                       # both kinds of key were seen
    assert redraws > 0                          # redraw passes happened, with fresh noise tuples (restated above)
    # consuming the mix stream leaves the crop stream alone (separate generators, separately seeded)
    a, b = D.crop_rng(7, 0, 0), D.crop_rng(7, 0, 0)
    D.draw_mix(list(range(11)), lengths, Lc, D.mix_rng(7, 0, 0), D.Remix(1.0))
    assert [a.randint(0, 1000) for _ in range(8)] == [b.randint(0, 1000) for _ in range(8)]


def test_parse_option_takes_the_flags_and_keeps_the_defaults(D, tmp_path):
    from speech_enhancement_amd import main_gan as MG
    args, _ = MG.parse_option(['--cfg', '/dev/null'])
    assert args.remix_prob == 0.0 and args.remix_snr == [0.0, 20.0]
    args, _ = MG.parse_option(['--cfg', '/dev/null', '--remix-prob', '0.5', '--remix-snr', '-5', '15', '-b', '4'])
    assert args.remix_prob == 0.5 and args.remix_snr == [-5.0, 15.0] and args.batch_size == 4
    # the train loader alone gets the Remix; without the flag the loaders are built exactly as before
    built = []

    class FakeSet:
        def __init__(self, *a, **k):
            pass

    class FakeLoader:
        def __init__(self, dataset, batch_size, crop_samples, shuffle, **kw):
            built.append(kw)

    import unittest.mock as mock
    with mock.patch.object(D, 'DeviceDataset', FakeSet), mock.patch.object(D, 'DeviceLoader', FakeLoader):
        args.distributed, args.gpu = False, 0
        MG.device_loaders(args, types_config(), 16000)
        assert isinstance(built[0]['remix'], D.Remix) and (built[0]['remix'].prob, built[0]['remix'].snr_db) == (0.5, (-5.0, 15.0))
        assert 'remix' not in built[1]
        args.remix_prob = 0.0
        MG.device_loaders(args, types_config(), 16000)
        assert 'remix' not in built[2] and 'remix' not in built[3]
        args.remix_prob = 1.5
        with pytest.raises(ValueError):
            MG.device_loaders(args, types_config(), 16000)
    for extra in (['--synthetic', '2'], []):
        with mock.patch.object(MG, 'DATASET_FACTORY', None if extra else (lambda a, c: ([], []))):
            with pytest.raises(RuntimeError, match='--remix-prob'):
                MG.main(['--cfg', '/dev/null', '--remix-prob', '0.3', '--output', str(tmp_path)] + extra)


def types_config():
    import types
    return types.SimpleNamespace(DATA=types.SimpleNamespace(TRAIN_CLEAN_DIR='a', TRAIN_NOISY_DIR='b', TEST_CLEAN_DIR='c', TEST_NOISY_DIR='d'),
                                 SAMPLE_RATE=16000, CROP_LEN=1)
