"""CPU-only tests of the noise bank in the dataset layer (speech-enhancement_amd/data.py): the C ABI of se_crop_gather_bank, the
BankMix value class, the host draws of the bank stream, the loader's key and redraw plan -- paired and clean-only -- with the device
launches stubbed out, and the flags of main_gan."""
import bisect
import ctypes as C
import math
import os
import re
import types

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


def stand_in(lengths, arena=None):
    """what the loader uses of a NoiseBank"""
    offsets = [0] + np.cumsum(lengths)[:-1].tolist()
    return types.SimpleNamespace(lengths=list(lengths), offsets=offsets, total=int(sum(lengths)), arena=arena)


def test_library_exports_and_header_declare_the_bank_gather(D):
    import speech_enhancement_amd as S
    from speech_enhancement_amd import _lib
    assert hasattr(_lib.lib(), 'se_crop_gather_bank')
    header = open(os.path.join(ROOT, 'include', 'se_hip.h')).read()
    assert re.search(r'^int se_crop_gather_bank\(const float\* clean_arena, const float\* noisy_arena, long long arena_total, '
                     r'const float\* bank,\s+long long bank_total, const long long\* rows, const double\* gain, int B, int L,', header,
                     re.M)
    for name in ('NoiseBank', 'BankMix', 'bank_rng', 'draw_bank', 'mix_bank_at_snr'):
        assert getattr(S, name) is getattr(D, name)


def test_null_and_bad_sizes_are_errors_not_launches(D):
    """the argument checks come before any device call: they can be exercised without a GPU"""
    from speech_enhancement_amd import _lib
    with pytest.raises(_lib.SeHipError, match='null operand'):
        _lib.call('se_crop_gather_bank', None, None, 10, None, 10, None, None, 1, 1, None, None, None, None, None, 16, None)
    one = C.c_void_p(8)                          # never dereferenced: the checks fail first
    with pytest.raises(_lib.SeHipError, match='null operand'):                  # the bank alone is missing
        _lib.call('se_crop_gather_bank', one, one, 10, None, 10, one, one, 1, 16, one, one, one, one, one, 16, None)
    with pytest.raises(_lib.SeHipError, match='bad sizes'):
        _lib.call('se_crop_gather_bank', one, one, 10, one, 10, one, one, 0, 16, one, one, one, one, one, 16, None)
    for bank_total in (0, -4):
        with pytest.raises(_lib.SeHipError, match='bad sizes'):
            _lib.call('se_crop_gather_bank', one, one, 10, one, bank_total, one, one, 1, 16, one, one, one, one, one, 16, None)
    with pytest.raises(_lib.SeHipError, match='workspace'):                     # too small
        _lib.call('se_crop_gather_bank', one, one, 10, one, 10, one, one, 2, 4097, one, one, one, one, one, 63, None)
    with pytest.raises(_lib.SeHipError, match='workspace'):                     # misaligned
        _lib.call('se_crop_gather_bank', one, one, 10, one, 10, one, one, 2, 4097, one, one, one, one, C.c_void_p(12), 64, None)


def test_bankmix_validation(D):
    bank = stand_in([100, 50])
    m = D.BankMix(bank, 0.25, (-5, 15))
    assert m.bank is bank and m.prob == 0.25 and m.snr_db == (-5.0, 15.0)
    assert D.BankMix(bank, 0.0).snr_db == (0.0, 20.0) and D.BankMix(bank, 1, (3, 3)).prob == 1.0
    for prob in (-0.01, 1.01, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            D.BankMix(bank, prob, (0, 20))
    for snr in ((5, 4), (float('nan'), 3), (0, float('inf')), (float('-inf'), 0)):
        with pytest.raises(ValueError):
            D.BankMix(bank, 0.5, snr)
    with pytest.raises(TypeError):
        D.BankMix([1.0, 2.0], 0.5)

    class DS(list):
        lengths = [100] * 4
    with pytest.raises(TypeError):
        D.DeviceLoader(DS(range(4)), 2, 50, True, bank=0.5)
    with pytest.raises(ValueError):
        D.DeviceLoader(DS(range(4)), 2, 50, True, remix=D.Remix(0.5), bank=m)
    ld = D.DeviceLoader(DS(range(4)), 2, 50, True, bank=m)
    assert ld.bank is m and ld.remix is None and D.DeviceLoader(DS(range(4)), 2, 50, True).bank is None


def test_draw_bank_is_a_function_of_seed_epoch_rank(D):
    lengths = [200, 64, 30, 500, 1, 90]
    bank = stand_in(lengths)
    offs, total = bank.offsets, bank.total
    half = D.BankMix(bank, 0.5, (-5, 15))
    a = D.draw_bank(40, offs, total, D.bank_rng(7, 2, 1), half)
    assert a == D.draw_bank(40, offs, total, D.bank_rng(7, 2, 1), half) and len(a) == 40
    for other in ((7, 3, 1), (7, 2, 0), (8, 2, 1)):
        assert a != D.draw_bank(40, offs, total, D.bank_rng(*other), half)
    none = D.draw_bank(40, offs, total, D.bank_rng(7, 2, 1), D.BankMix(bank, 0.0, (-5, 15)))
    every = D.draw_bank(40, offs, total, D.bank_rng(7, 2, 1), D.BankMix(bank, 1.0, (-5, 15)))
    assert none == [None] * 40 and all(m is not None for m in every)
    # the draws do not depend on prob: a mixed row of prob = 0.5 is the row of prob = 1
    assert any(m is not None for m in a) and any(m is None for m in a)
    assert all(m is None or m == e for m, e in zip(a, every))
    for j, s, snr in every:
        assert 0 <= j < len(lengths) and 0 <= s < lengths[j] and -5 <= snr <= 15
    # the restatement of the stream: u, p, snr per row; file and start from p
    rng = D.bank_rng(7, 2, 1)
    for got in a:
        u, p, snr = rng.random(), rng.randrange(total), rng.uniform(-5, 15)
        j = bisect.bisect_right(offs, p) - 1
        assert got == ((j, p - offs[j], snr) if u < 0.5 else None)
    assert D.bank_rng(7, 2, 1).random() != D.crop_rng(7, 2, 1).random() != D.mix_rng(7, 2, 1).random()
    assert D.bank_rng(7, 2, 1).random() != D.mix_rng(7, 2, 1).random()


def test_draw_bank_boundaries(D):
    """p = offsets[j] is start 0 of file j, p = offsets[j + 1] - 1 its last sample"""
    lengths = [200, 64, 30, 500, 1, 90]
    bank = stand_in(lengths)
    mix = D.BankMix(bank, 1.0, (0, 0))

    class Fixed:
        def __init__(self, p):
            self.p = p

        def random(self):
            return 0.0

        def randrange(self, n):
            assert n == bank.total
            return self.p

        def uniform(self, lo, hi):
            return lo
    for j, n in enumerate(lengths):
        assert D.draw_bank(1, bank.offsets, bank.total, Fixed(bank.offsets[j]), mix) == [(j, 0, 0.0)]
        assert D.draw_bank(1, bank.offsets, bank.total, Fixed(bank.offsets[j] + n - 1), mix) == [(j, n - 1, 0.0)]


def test_draw_bank_weights_files_by_duration(D):
    """20 000 draws over files of 7000 / 300 / 64 / 1 / 5000 samples: every count inside five binomial standard errors of
    n len / total (11322 / 485 / 104 / 2 / 8087; bank_rng(0, 0, 0) gives 11239 / 499 / 105 / 3 / 8154)"""
    lengths = [7000, 300, 64, 1, 5000]
    bank = stand_in(lengths)
    n = 20000
    draws = D.draw_bank(n, bank.offsets, bank.total, D.bank_rng(0, 0, 0), D.BankMix(bank, 1.0))
    counts = np.bincount([j for j, _, _ in draws], minlength=len(lengths))
    print('counts', counts.tolist())
    for j, length in enumerate(lengths):
        q = length / bank.total
        assert abs(counts[j] - n * q) <= 5.0 * math.sqrt(n * q * (1 - q)), (j, counts[j], n * q)
    starts = [s for j, s, _ in draws if j == 0]
    assert min(starts) < 100 and max(starts) > 6900            # a start anywhere in the file, its last samples included


class HostDataset:
    def __init__(self, signals, noise=None):
        self.signals, self.noise, self.paired = signals, noise, noise is not None
        self.lengths = [len(s) for s in signals]

    def __len__(self):
        return len(self.signals)


def crop(x, s, Lc):
    return x[s:s + Lc] if s >= 0 else np.resize(x, Lc)


def wrapped(x, s, Lc):
    return x[(s + np.arange(Lc)) % len(x)]


def host_loader(D, ds, noise, *args, **kwargs):
    """a DeviceLoader whose device steps (the gather launches) are numpy; everything else is the product code.  The stub mixes at
    scale 1 and reports scale 0 (a fallback) for a silent noise crop, as the kernel does; an unpaired dataset's own noise is zero."""
    launches = []

    class Gathered:
        def __init__(self, clean, noisy, scale):
            self.clean, self.noisy, self.scale = torch.from_numpy(clean), torch.from_numpy(noisy), scale

        def stats(self):
            c, v = self.clean.numpy().astype(np.float64), self.noisy.numpy().astype(np.float64)
            return np.stack([(c ** 2).sum(1), (v ** 2).sum(1), np.abs(c).max(1)], 1)

    class Loader(D.DeviceLoader):
        def _gather(self, files, starts):
            return self._gather_bank(files, starts, [None] * len(files))

        def _gather_mix(self, files, starts, mix):
            raise AssertionError('a bank loader launches no corpus remix')

        def _gather_bank(self, files, starts, mix):
            Lc = self.crop_samples
            clean = np.stack([crop(ds.signals[f], s, Lc) for f, s in zip(files, starts)]).astype(np.float32)
            out, scale = [], np.zeros(len(files), dtype=np.float32)
            for r, (f, s, m) in enumerate(zip(files, starts, mix)):
                d = crop(ds.noise[f], s, Lc) if ds.paired else np.zeros(Lc, dtype=np.float32)
                if m is not None and np.any(wrapped(noise[m[0]], m[1], Lc)) and np.any(clean[r]):
                    d, scale[r] = wrapped(noise[m[0]], m[1], Lc), 1.0
                out.append(d)
            launches.append((list(files), list(starts), list(mix)))
            return Gathered(clean, clean + np.stack(out).astype(np.float32), scale)

    ld = Loader(ds, *args, **kwargs)
    ld.launches = launches
    return ld


def test_loader_plan_keys_and_streams(D):
    """order and crop starts with the bank on are those with it off; every launch carries one noise tuple per row, a redraw pass a
    fresh one; a mixed row's key is (file, start, 'bank', j, start_n, snr), a row the launch did not mix keeps the plain pair"""
    Lc = 64
    rs = np.random.RandomState(5)
    lengths = [200, 64, 30, 500, 1, 90, 64, 333, 40, 1000, 65]
    sig = [(0.01 * rs.randn(n)).astype(np.float32) for n in lengths]
    own = [(0.003 * rs.randn(n)).astype(np.float32) for n in lengths]
    sig[9][:700] = 1.0                          # a spike in most crops of file 9: redrawn until one lies in the tail
    ds = HostDataset(sig, own)
    bank_lengths = [300, 40, 500, 1, 700]
    noise = [(0.003 * rs.randn(n)).astype(np.float32) for n in bank_lengths]
    silent = 2
    noise[silent][:] = 0.0                      # rows that draw this file fall back
    bank = stand_in(bank_lengths)
    spike = lambda st: st[:, 2] > 0.5
    redraws, lens, hit_silent = 0, set(), 0
    for epoch in (0, 1):
        plain = host_loader(D, ds, noise, 4, Lc, True, seed=7, reject=spike)
        mixed = host_loader(D, ds, noise, 4, Lc, True, seed=7, reject=spike, bank=D.BankMix(bank, 1.0, (0, 15)))
        off = host_loader(D, ds, noise, 4, Lc, True, seed=7, reject=spike, bank=D.BankMix(bank, 0.0, (0, 15)))
        for ld in (plain, mixed, off):
            ld.set_epoch(epoch)
        p_items, m_items, o_items = list(plain), list(mixed), list(off)
        assert [[k[:2] for k in it['keys']] for it in m_items] == [it['keys'] for it in p_items] == [it['keys'] for it in o_items]
        assert [(f, s) for f, s, _ in mixed.launches] == [(f, s) for f, s, _ in plain.launches]      # the crop stream is untouched
        redraws += len(mixed.launches) - len(mixed)
        # the bank stream restated: first draws of batch i + 1 precede the redraw draws of batch i, as in the crop stream
        brng = D.bank_rng(7, epoch, 0)
        for files, _, mix in mixed.launches:
            assert len(mix) == len(files)
            assert mix == D.draw_bank(len(files), bank.offsets, bank.total, brng, D.BankMix(bank, 1.0, (0, 15)))
        last = {}
        for files, starts, mix in mixed.launches:
            for f, s, m in zip(files, starts, mix):
                last[f] = (s, m)                # the final attempt of a file is the one that was kept
        for it, po in zip(m_items, o_items):
            assert torch.equal(it['audio'], po['audio'])
            for row, key in enumerate(it['keys']):
                s, m = last[key[0]]
                assert key[1] == s
                if m[0] == silent:              # silent noise: the stub (like the kernel) reports scale 0
                    hit_silent += 1
                    assert key == (key[0], s) and torch.equal(it['noisy'][row], po['noisy'][row])
                else:
                    assert key == (key[0], s, 'bank', m[0], m[1], m[2]) and len(key) == 6
                    assert np.array_equal(it['noisy'][row].numpy(), it['audio'][row].numpy() + wrapped(noise[m[0]], m[1], Lc))
        lens |= {len(k) for it in m_items for k in it['keys']}
        assert all(len(k) == 2 for it in o_items for k in it['keys'])
    assert lens == {2, 6} and hit_silent > 0    # both kinds of key were seen: the seed's draws hit the silent file
    assert redraws > 0                          # redraw passes happened, with fresh noise tuples (restated above)
    # consuming the bank stream leaves the crop stream alone (separate generators, separately seeded)
    a, b = D.crop_rng(7, 0, 0), D.crop_rng(7, 0, 0)
    D.draw_bank(11, bank.offsets, bank.total, D.bank_rng(7, 0, 0), D.BankMix(bank, 1.0))
    assert [a.randint(0, 1000) for _ in range(8)] == [b.randint(0, 1000) for _ in range(8)]


def test_clean_only_dataset_needs_the_bank_and_redraws_unmixed_rows(D):
    Lc = 64
    rs = np.random.RandomState(6)
    lengths = [200, 64, 30, 500, 90, 333, 1000, 65]
    sig = [(0.01 * rs.randn(n)).astype(np.float32) for n in lengths]
    ds = HostDataset(sig)
    assert not ds.paired
    bank_lengths = [300, 900, 40]
    noise = [(0.003 * rs.randn(n)).astype(np.float32) for n in bank_lengths]
    silent = 1
    noise[silent][:] = 0.0                      # most of the bank is silent: many rows need a second draw
    bank = stand_in(bank_lengths)
    for kw in ({}, {'remix': D.Remix(1.0)}, {'bank': D.BankMix(bank, 0.5)}, {'bank': D.BankMix(bank, 0.0)}):
        with pytest.raises(ValueError):
            D.DeviceLoader(ds, 4, Lc, True, **kw)
    ld = host_loader(D, ds, noise, 4, Lc, True, seed=3, bank=D.BankMix(bank, 1.0, (0, 15)))
    items = list(ld)
    assert len(ld.launches) > len(ld)           # redraw passes happened
    # every delivered row is mixed, and from a file that is not the silent one
    keys = [k for it in items for k in it['keys']]
    assert keys and all(len(k) == 6 and k[2] == 'bank' and k[3] != silent for k in keys)
    for it in items:
        assert not torch.equal(it['audio'], it['noisy']) and it['audio'].shape == (len(it['keys']), Lc)
    # both streams restated over the launches: a redrawn row draws a fresh start (a tiled one draws none) and a fresh noise tuple
    rng, brng = D.crop_rng(3, 0, 0), D.bank_rng(3, 0, 0)
    first, tiled_again, silent_first = set(), 0, 0
    for files, starts, mix in ld.launches:
        assert starts == [rng.randint(0, lengths[f] - Lc) if lengths[f] >= Lc else -1 for f in files]
        assert mix == D.draw_bank(len(files), bank.offsets, bank.total, brng, ld.bank)
        redraw = all(f in first for f in files)
        if not redraw:
            silent_first += sum(m[0] == silent for m in mix)
        else:
            tiled_again += sum(lengths[f] < Lc for f in files)
        first |= set(files)
    assert silent_first > 0 and tiled_again > 0         # the draws hit the silent file, also for the tiled row (file 2)
    last = {}
    for files, starts, mix in ld.launches:
        for f, s, m in zip(files, starts, mix):
            last[f] = (s, m)
    assert all(k == (k[0], last[k[0]][0], 'bank') + last[k[0]][1] for k in keys)
    # a bank without any sound: ten attempts per batch, every row dropped, nothing delivered
    mute = [np.zeros(n, dtype=np.float32) for n in bank_lengths]
    ld = host_loader(D, ds, mute, 4, Lc, True, seed=3, bank=D.BankMix(bank, 1.0, (0, 15)))
    assert list(ld) == []
    assert len(ld.launches) == D.MAX_ATTEMPTS * len(ld)
    assert all(len(f) == 4 for f, _, _ in ld.launches)
    # rows that `reject` flags behave as before: a tiled one is dropped at once, whatever its noise
    assert 2 in {k[0] for k in keys}                        # file 2 (30 samples, tiled) was delivered above
    energy2 = float((np.resize(sig[2], Lc).astype(np.float64) ** 2).sum())
    only2 = lambda st: np.isclose(st[:, 0], energy2, rtol=1e-6)
    ld = host_loader(D, ds, noise, 4, Lc, True, seed=3, reject=only2, bank=D.BankMix(bank, 1.0, (0, 15)))
    assert 2 not in {k[0] for it in ld for k in it['keys']}
    assert sum(2 in f for f, _, _ in ld.launches) == 1


def types_config(noisy='b'):
    return types.SimpleNamespace(DATA=types.SimpleNamespace(TRAIN_CLEAN_DIR='a', TRAIN_NOISY_DIR=noisy, TEST_CLEAN_DIR='c',
                                                            TEST_NOISY_DIR='d'), SAMPLE_RATE=16000, CROP_LEN=1)


def test_parse_option_takes_the_flags_and_keeps_the_defaults(D, tmp_path):
    import unittest.mock as mock
    from speech_enhancement_amd import main_gan as MG
    base, _ = MG.parse_option(['--cfg', '/dev/null'])
    assert base.noise_dir is None and base.noise_prob == 1.0 and base.noise_snr == [0.0, 20.0]
    args, _ = MG.parse_option(['--cfg', '/dev/null', '--noise-dir', 'x', 'y', '--noise-prob', '0.5', '--noise-snr', '-5', '15', '-b', '4'])
    assert args.noise_dir == ['x', 'y'] and args.noise_prob == 0.5 and args.noise_snr == [-5.0, 15.0] and args.batch_size == 4
    same = {k for k in vars(base) if getattr(base, k) == getattr(args, k)}
    assert set(vars(base)) - same == {'noise_dir', 'noise_prob', 'noise_snr', 'batch_size'}
    # the train loader alone gets the BankMix; without the flag the loaders are built exactly as before
    sets, banks, built = [], [], []

    class FakeSet:
        def __init__(self, *a, **k):
            sets.append(a)

    class FakeBank:
        def __init__(self, noise_dir, sample_rate, device=None):
            banks.append((noise_dir, sample_rate))
            self.files, self.lengths, self.offsets, self.total, self.nbytes, self.arena = ['f'], [100], [0], 100, 400, None

    class FakeLoader:
        def __init__(self, dataset, batch_size, crop_samples, shuffle, **kw):
            built.append(kw)

    with mock.patch.object(D, 'DeviceDataset', FakeSet), mock.patch.object(D, 'DeviceLoader', FakeLoader), \
            mock.patch.object(D, 'NoiseBank', FakeBank):
        args.distributed, args.gpu = False, 0
        MG.device_loaders(args, types_config(), 16000)
        assert banks == [(['x', 'y'], 16000)] and sets[0][:2] == ('a', 'b')
        mix = built[0]['bank']
        assert isinstance(mix, D.BankMix) and (mix.prob, mix.snr_db) == (0.5, (-5.0, 15.0)) and 'remix' not in built[0]
        assert 'bank' not in built[1] and 'remix' not in built[1]
        base.distributed, base.gpu = False, 0
        MG.device_loaders(base, types_config(), 16000)
        assert 'bank' not in built[2] and 'bank' not in built[3] and len(banks) == 1
        # clean speech alone: needs the bank at probability 1
        with pytest.raises(RuntimeError, match='--noise-dir'):
            MG.device_loaders(base, types_config(''), 16000)
        with pytest.raises(RuntimeError, match='--noise-prob'):
            MG.device_loaders(args, types_config(''), 16000)
        args.noise_prob = 1.0
        MG.device_loaders(args, types_config(''), 16000)
        assert sets[-2][:2] == ('a', None) and built[-2]['bank'].prob == 1.0 and 'bank' not in built[-1]
    # the conflicts raise in main(), before any GPU work
    common = ['--cfg', '/dev/null', '--noise-dir', str(tmp_path), '--output', str(tmp_path)]
    with pytest.raises(RuntimeError, match='--noise-dir'):
        MG.main(common + ['--synthetic', '2'])
    with mock.patch.object(MG, 'DATASET_FACTORY', lambda a, c: ([], [])):
        with pytest.raises(RuntimeError, match='--noise-dir'):
            MG.main(common)
    with pytest.raises(RuntimeError, match='--noise-dir'):
        MG.main(common + ['--remix-prob', '0.3'])
    with pytest.raises(RuntimeError, match='--noise-dir'):
        MG.main(['--cfg', '/dev/null', '--output', str(tmp_path), '--opts', 'DATA.TRAIN_NOISY_DIR', ''])
    with pytest.raises(RuntimeError, match='--noise-prob'):
        MG.main(common + ['--noise-prob', '0.5', '--opts', 'DATA.TRAIN_NOISY_DIR', ''])
