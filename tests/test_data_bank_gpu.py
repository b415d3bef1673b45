"""GPU tests of the noise bank (se_crop_gather_bank, data.NoiseBank, data.BankMix): the kernel pair against the definition in
include/se_hip.h -- indexing and wrapping bit for bit, the scale and the mixed samples inside one fp32 ulp of their fp64 values, the
achieved SNR -- and against se_crop_gather_mix on a bank that holds the corpus' own noise; then NoiseBank against read_wav +
resample, the loader reproduced from its own keys (paired and clean-only), mix_bank_at_snr, and main_gan trained for one epoch with
a noise folder.  Wavs are generated here."""
import ctypes as C
import logging
import math
import os
import re
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LENGTHS = [9000, 5000, 257, 64, 1, 700]         # the speech corpus; utterance 5 has noisy == clean
BANK = [7000, 4500, 300, 64, 1, 600]            # the bank; file 5 is silent


@pytest.fixture(scope='module')
def D():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import data
    return data


@pytest.fixture(scope='module')
def arena():
    rs = np.random.RandomState(21)
    clean = [(0.1 * rs.randn(n)).astype(np.float32) for n in LENGTHS]
    noisy = [c + (0.03 * rs.randn(c.size)).astype(np.float32) for c in clean]
    noisy[5] = clean[5].copy()
    bank = [(0.05 * rs.randn(n)).astype(np.float32) for n in BANK]
    bank[5][:] = 0.0
    offs = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]]).astype(np.int64)
    boffs = np.concatenate([[0], np.cumsum(BANK)[:-1]]).astype(np.int64)
    dev = lambda xs: torch.from_numpy(np.concatenate(xs)).cuda()
    return clean, noisy, bank, offs, boffs, dev(clean), dev(noisy), dev(bank)


def index(n, start, Lc):
    return (np.arange(Lc) % n) if n < Lc else start + np.arange(Lc)


def ulp32(x):
    """the spacing of fp32 at |x| (x: fp64 array or scalar)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def snr_db(c, v):
    c, v = c.astype(np.float64), v.astype(np.float64)
    return 10.0 * np.log10(np.sum(c * c) / np.sum((v - c) ** 2))


def launch(name, ca, na, ba, rows, gain, Lc):
    """se_crop_gather_bank (ba: the bank arena) or se_crop_gather_mix (ba None) into poisoned outputs"""
    from speech_enhancement_amd import _lib as L
    B, n = len(rows), -(-Lc // 4096)
    rows_d = torch.tensor(rows, dtype=torch.int64).cuda()
    gain_d = torch.tensor(gain, dtype=torch.float64).cuda()
    oc, on = torch.full((B, Lc), 9.0, device='cuda'), torch.full((B, Lc), 9.0, device='cuda')
    st = torch.full((B, n, 3), -1.0, dtype=torch.float64, device='cuda')
    sc = torch.full((B,), -1.0, device='cuda')
    need = L.lib().se_crop_gather_mix_workspace_bytes(B, Lc)
    assert need == 16 * B * n
    ws = torch.full((need // 8,), float('nan'), dtype=torch.float64, device='cuda')
    src = (L.ptr(ca), L.ptr(na), ca.numel()) + ((L.ptr(ba), ba.numel()) if ba is not None else ())
    L.call(name, *src, L.ptr(rows_d), L.ptr(gain_d), B, Lc, L.ptr(oc), L.ptr(on), L.ptr(st), L.ptr(sc), L.ptr(ws), need, L.stream())
    torch.cuda.synchronize()
    return oc, on, st, sc


def plain_gather(ca, na, rows, Lc):
    from speech_enhancement_amd import _lib as L
    B = len(rows)
    pc, pn = torch.full((B, Lc), 9.0, device='cuda'), torch.full((B, Lc), 9.0, device='cuda')
    pst = torch.empty(B, 3, device='cuda')
    L.call('se_crop_gather', L.ptr(ca), L.ptr(na), C.c_longlong(ca.numel()), L.ptr(torch.tensor([r[:3] for r in rows]).cuda()),
           C.c_int(B), C.c_int(Lc), L.ptr(pc), L.ptr(pn), L.ptr(pst), L.stream())
    torch.cuda.synchronize()
    return pc, pn


@pytest.mark.parametrize('clean_only', [False, True])
@pytest.mark.parametrize('Lc', [4500, 300])
def test_kernel_equals_the_definition(D, arena, Lc, clean_only):
    """L = 4500: two chunks, the second partial, neither a multiple of 256; L = 300: one chunk.  clean_only: noisy_arena is
    clean_arena.  Bounds (those of the corpus remix): the scale is the fp32 rounding of an fp64 value whose sums differ from numpy's
    in order only (relative 1e-13): one ulp; a mixed sample is one fma rounding of c + a d (half an ulp) next to the fp64 evaluation
    here: one ulp; the statistics are fp64 sums of at most 4500 terms: 1e-12 relative; the SNR is met to rounding (1e-5 dB): 0.01 dB."""
    clean, noisy, bank, offs, boffs, ca, na, ba = arena
    if clean_only:
        noisy, na = clean, ca
    total, btotal = ca.numel(), ba.numel()
    # (speech utterance, start, bank file or None, noise start); the start of a tiled speech source is ignored
    plan = [(0, 1234, None, 0),                 # unmixed
            (0, 17, 0, 100),                    # no wrap (7000 from 100)
            (1, 3, 0, 6999),                    # one wrap, at the second sample
            (0, 9, 1, 1),                       # 4500 from 1: one wrap at L = 4500 (its last sample), none at L = 300
            (1, 5, 2, 299),                     # 300 from 299: many wraps at L = 4500
            (0, 4500, 3, 63),                   # 64 from 63: many wraps, the period no divisor of 256 + start
            (1, 0, 4, 0),                       # a file of one sample
            (2, 0, 0, 6900),                    # tiled speech (257), wrapped noise
            (3, 0, 3, 5),                       # tiled speech (64), wrapped noise (64)
            (4, 0, 2, 7),                       # tiled speech (1)
            (1, 7, 5, 100),                     # silent noise: falls back
            (1, 7, 0, 7000),                    # start_n == len_n: falls back
            (1, 7, 0, -1),                      # start_n < 0: falls back
            (1, 7, None, 0),                    # off_n + len_n > bank_total: falls back (patched below)
            (0, 0, 1, 11)]                      # speech source beyond the arena: zeros (patched below)
    rows = []
    for f, s, j, sj in plan:
        rows.append([offs[f], LENGTHS[f], s] + ([-1, 0, 0] if j is None else [boffs[j], BANK[j], sj]))
    rows[13][3:] = [btotal - 10, 11, 0]
    rows[14][:3] = [total - 10, 2000, 0]
    rows = [[int(v) for v in r] for r in rows]
    mixed = tuple(range(1, 10))
    # the plain gather of the speech sources: what unmixed and fallen-back rows must equal bit for bit
    pc, pn = plain_gather(ca, na, rows, Lc)
    for target in (-5.0, 0.0, 20.0):
        gain = [10.0 ** (-target / 20.0)] * len(rows)
        oc, on, st, sc = launch('se_crop_gather_bank', ca, na, ba, rows, gain, Lc)
        again = launch('se_crop_gather_bank', ca, na, ba, rows, gain, Lc)
        for x, y in zip((oc, on, st, sc), again):
            assert torch.equal(x, y)                                       # a fixed order: two launches agree bit for bit
        oc_h, on_h, st_h, sc_h = oc.cpu().numpy(), on.cpu().numpy(), st.cpu().numpy(), sc.cpu().numpy()
        for b, (f, s, j, sj) in enumerate(plan):
            if b == 14:
                assert not oc_h[b].any() and not on_h[b].any() and sc_h[b] == 0 and not st_h[b].any()
                continue
            c = clean[f][index(LENGTHS[f], s, Lc)]
            assert np.array_equal(oc_h[b], c), b
            # the chunk partials, added in index order, are the fp64 sums of what was written
            got = np.array([st_h[b, :, 0].sum(), st_h[b, :, 1].sum(), st_h[b, :, 2].max()])
            want = np.array([np.sum(oc_h[b].astype(np.float64) ** 2), np.sum(on_h[b].astype(np.float64) ** 2), np.abs(oc_h[b]).max()])
            print(f'L={Lc} snr={target} row {b}: stats rel err {np.max(np.abs(got - want) / want):.2e}')
            np.testing.assert_allclose(got[:2], want[:2], rtol=1e-12, atol=0)
            assert got[2] == want[2]
            if b not in mixed:
                assert sc_h[b] == 0, b
                assert torch.equal(oc[b], pc[b]) and torch.equal(on[b], pn[b]), b
                assert np.array_equal(on_h[b], noisy[f][index(LENGTHS[f], s, Lc)]), b
                continue
            d = bank[j][(sj + np.arange(Lc)) % BANK[j]]
            assert d.dtype == np.float32
            a64 = math.sqrt(np.sum(c.astype(np.float64) ** 2) / np.sum(d.astype(np.float64) ** 2)) * gain[b]
            print(f'L={Lc} snr={target} row {b}: scale {sc_h[b]!r} vs {a64!r} ({abs(float(sc_h[b]) - a64) / ulp32(a64):.3f} ulp)')
            assert abs(float(sc_h[b]) - a64) <= ulp32(a64), (b, sc_h[b], a64)
            ref = c.astype(np.float64) + float(sc_h[b]) * d.astype(np.float64)
            err = np.abs(on_h[b].astype(np.float64) - ref)
            bound = np.maximum(ulp32(ref), ulp32(on_h[b]))
            print(f'L={Lc} snr={target} row {b}: worst sample {np.max(err / bound):.3f} ulp, SNR {snr_db(oc_h[b], on_h[b]):.6f} dB')
            assert (err <= bound).all(), (b, int(np.argmax(err - bound)))
            assert abs(snr_db(oc_h[b], on_h[b]) - target) <= 0.01, (b, snr_db(oc_h[b], on_h[b]))
    # a gain that is not finite, or zero, falls back as well
    oc, on, st, sc = launch('se_crop_gather_bank', ca, na, ba, rows[1:4], [float('inf'), 0.0, float('nan')], Lc)
    assert float(sc.abs().max()) == 0 and torch.equal(on, pn[1:4]) and torch.equal(oc, pc[1:4])


@pytest.mark.parametrize('Lc', [4500, 300])
def test_bank_of_the_corpus_noise_equals_the_corpus_remix(D, arena, Lc):
    """a bank that holds noisy - clean of the corpus (the one fp32 subtraction se_crop_gather_mix makes per sample), in the corpus'
    layout, and noise sources that do not tile: the same row table means the same samples to both entries, and everything they
    return agrees bit for bit"""
    clean, noisy, _, offs, _, ca, na, _ = arena
    ba = na - ca
    long_enough = [j for j, n in enumerate(LENGTHS) if n >= Lc]          # 0, 1 and at L = 300 also 5, the silent one
    rows, k = [], 0
    for f in range(len(LENGTHS)):
        for j in long_enough:
            s = min(13 * k, max(LENGTHS[f] - Lc, 0))
            sj = (LENGTHS[j] - Lc) if k % 3 == 0 else (37 * k) % (LENGTHS[j] - Lc + 1)
            rows.append([int(offs[f]), LENGTHS[f], s, int(offs[j]), LENGTHS[j], sj])
            k += 1
    rows.append([int(offs[0]), LENGTHS[0], 5, -1, 0, 0])                 # an unmixed row
    gain = [10.0 ** (-(k % 7 - 2) * 2.5 / 20.0) for k in range(len(rows))]
    want = launch('se_crop_gather_mix', ca, na, None, rows, gain, Lc)
    got = launch('se_crop_gather_bank', ca, na, ba, rows, gain, Lc)
    assert int((want[3] != 0).sum()) >= 2 * len(LENGTHS) - 2             # the rows were mixed, not fallen back
    for name, x, y in zip(('clean', 'noisy', 'stats', 'scale'), want, got):
        assert torch.equal(x, y), name


def write_wav(path, x, sr, channels=1):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(x, dtype='<i2').tobytes())


def speechlike(rs, n, sr):
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + rs.rand() * 6) for a, f in ((0.3, 180.0), (0.2, 360.0), (0.1, 2500.0), (0.05, 6100.0)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rs.randn(n)).clip(-0.99, 0.99)


def make_corpus(tmp_path, rs, spec, clean_name='clean', noisy_name='noisy'):
    """spec: [(name, sample rate, samples or None for an all-zero pair of 20000)] -> (clean dir, noisy dir)"""
    cdir, ndir = tmp_path / clean_name, tmp_path / noisy_name
    os.makedirs(cdir)
    os.makedirs(ndir)
    for name, sr, n in spec:
        if n is None:
            c = np.zeros(20000, dtype=np.int16)
            v = c.copy()
        else:
            c = np.round(speechlike(rs, n, sr) * 20000).astype(np.int16)
            v = np.clip(c + np.round(2000 * rs.randn(n)), -32768, 32767).astype(np.int16)
        write_wav(cdir / name, c, sr)
        write_wav(ndir / name, v, sr)
    return str(cdir), str(ndir)


def make_noise(root, rs, silent=True):
    """a noise folder: files at 16, 48 and 44.1 kHz, a stereo one, one in a nested subfolder, a short one and (optionally) a silent one"""
    os.makedirs(root / 'street' / 'night')
    noise = lambda n: np.round(3000 * rs.randn(n)).astype(np.int16)
    write_wav(root / 'a16.wav', noise(21000), 16000)
    write_wav(root / 'b48.wav', noise(40000), 48000)
    write_wav(root / 'c441.wav', noise(30000), 44100)
    write_wav(root / 'street' / 'd_stereo.wav', np.stack([noise(9000), noise(9000)], 1), 48000, channels=2)
    write_wav(root / 'street' / 'night' / 'e_short.wav', noise(1000), 16000)
    if silent:
        write_wav(root / 'street' / 'z_silent.wav', np.zeros(24000, dtype=np.int16), 48000)
    return str(root)


def crop(x, n, start, Lc):
    return x[torch.arange(Lc, device=x.device) % n] if n < Lc else x[start:start + Lc]


def wrapped(x, start, Lc):
    return x[(start + torch.arange(Lc, device=x.device)) % x.numel()]


def check_mixed_row(c, d, v, snr):
    """v (fp32) against c + a d: a is the fp32 scale (inside one ulp of its fp64 value: the kernel test), the sample one fma
    rounding -> |err| <= ulp(v) + ulp(a) |d|; and the SNR the key states, to 0.01 dB"""
    c, d, v = (t.cpu().numpy() for t in (c, d, v))
    a = math.sqrt(np.sum(c.astype(np.float64) ** 2) / np.sum(d.astype(np.float64) ** 2)) * 10.0 ** (-snr / 20.0)
    ref = c.astype(np.float64) + a * d.astype(np.float64)
    bound = np.maximum(ulp32(ref), ulp32(v)) + ulp32(a) * np.abs(d.astype(np.float64))
    assert (np.abs(v.astype(np.float64) - ref) <= bound).all()
    assert abs(snr_db(c, v) - snr) <= 0.01


SPEC = [(f'u{k:02d}.wav', 48000 if k % 3 else 16000, int(n)) for k, n in
        enumerate([30000, 5000, 2999, 12000, 9000, 3000, 700, 20000, 4000, 3001, 15000])] + [('zz_silent.wav', 48000, None)]


@pytest.fixture(scope='module')
def folders(D, tmp_path_factory):
    root = tmp_path_factory.mktemp('bank')
    cdir, ndir = make_corpus(root, np.random.RandomState(31), SPEC)
    return cdir, ndir, make_noise(root / 'noise', np.random.RandomState(32))


@pytest.fixture(scope='module')
def corpus(D, folders):
    return D.DeviceDataset(folders[0], folders[1], device='cuda:0')


@pytest.fixture(scope='module')
def bank(D, folders):
    return D.NoiseBank(folders[2], device='cuda:0')


def test_noise_bank_is_read_wav_and_resample(D, folders, bank, tmp_path):
    root = folders[2]
    want = [os.path.join(root, p) for p in ('a16.wav', 'b48.wav', 'c441.wav', 'street/d_stereo.wav', 'street/night/e_short.wav',
                                            'street/z_silent.wav')]
    assert bank.files == want and len(bank) == 6
    assert bank.rates == [16000, 48000, 44100, 48000, 16000, 48000] and bank.raw_lengths == [21000, 40000, 30000, 9000, 1000, 24000]
    assert bank.lengths == [21000, 13334, 10885, 3000, 1000, 8000]
    assert bank.offsets == [0] + np.cumsum(bank.lengths)[:-1].tolist() and bank.total == sum(bank.lengths)
    assert bank.nbytes == 4 * bank.total and bank.arena.shape == (bank.total,) and bank.arena.dtype == torch.float32
    assert bank.device == torch.device('cuda:0') and bank.arena.device == bank.device
    for i, p in enumerate(bank.files):
        sr, x = D.read_wav(p)
        assert x.ndim == 1 and x.dtype == np.float32
        y = D.resample(torch.from_numpy(x).cuda(), sr, 16000)
        assert torch.equal(bank.signal(i), y), p
        assert torch.equal(bank.arena[bank.offsets[i]:bank.offsets[i] + bank.lengths[i]], y)
    assert not bank.signal(5).any() and bank.signal(3).any()
    # a list of folders: each searched on its own, in the order given
    two = D.NoiseBank([os.path.join(root, 'street', 'night'), os.path.join(root, 'street')], device='cuda:0')
    assert [os.path.relpath(p, root) for p in two.files] == ['street/night/e_short.wav', 'street/d_stereo.wav',
                                                             'street/night/e_short.wav', 'street/z_silent.wav']
    assert torch.equal(two.signal(1), bank.signal(3))
    # the limit is checked before anything is allocated
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError):
        D.NoiseBank(root, device='cuda:0', max_bytes=4 * bank.total)
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(FileNotFoundError):
        D.NoiseBank(str(tmp_path), device='cuda:0')
    write_wav(tmp_path / 'empty.wav', np.zeros(0, dtype=np.int16), 16000)
    with pytest.raises(ValueError, match='empty.wav'):
        D.NoiseBank(str(tmp_path), device='cuda:0')


def test_loader_with_prob_zero_is_the_plain_loader(D, corpus, bank):
    Lc = 3000
    plain = D.DeviceLoader(corpus, 4, Lc, shuffle=True, seed=2)
    off = D.DeviceLoader(corpus, 4, Lc, shuffle=True, seed=2, bank=D.BankMix(bank, 0.0, (0, 15)))
    for epoch in (0, 1):
        plain.set_epoch(epoch)
        off.set_epoch(epoch)
        a, b = list(plain), list(off)
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            assert x['keys'] == y['keys'] and torch.equal(x['audio'], y['audio']) and torch.equal(x['noisy'], y['noisy'])


def test_loader_items_follow_from_their_keys(D, corpus, bank):
    ds, Lc = corpus, 3000
    silent_speech, silent_noise = len(ds) - 1, 5
    plain = D.DeviceLoader(ds, 4, Lc, shuffle=True, seed=2)
    ld = D.DeviceLoader(ds, 4, Lc, shuffle=True, seed=2, bank=D.BankMix(bank, 1.0, (0, 15)))
    seen, files_used, wraps = set(), set(), 0
    for epoch in (0, 1, 2):
        plain.set_epoch(epoch)
        ld.set_epoch(epoch)
        items, ref = list(ld), list(plain)
        assert [[k[:2] for k in it['keys']] for it in items] == [it['keys'] for it in ref]       # order and crop starts unchanged
        assert sorted(k[0] for it in items for k in it['keys']) == list(range(silent_speech))
        for it, pl in zip(items, ref):
            assert torch.equal(it['audio'], pl['audio'])                                         # the speech is the plain crop
            assert it['audio'].shape == it['noisy'].shape == (len(it['keys']), Lc)
            for row, key in enumerate(it['keys']):
                f, s = key[:2]
                c, v = (crop(x, ds.lengths[f], s, Lc) for x in ds.signal(f))
                assert torch.equal(it['audio'][row], c)
                seen.add(len(key))
                if len(key) == 2:                                  # only the silent file of the bank gives no noise to mix
                    assert torch.equal(it['noisy'][row], v)
                    continue
                _, _, tag, j, sj, snr = key
                assert tag == 'bank' and j != silent_noise and 0 <= snr <= 15 and 0 <= sj < bank.lengths[j]
                files_used.add(j)
                wraps += sj + Lc > bank.lengths[j]
                check_mixed_row(c, wrapped(bank.signal(j), sj, Lc), it['noisy'][row], snr)
        again = list(ld)                                                   # an epoch repeats itself bit for bit
        assert [it['keys'] for it in again] == [it['keys'] for it in items]
        assert all(torch.equal(x['noisy'], y['noisy']) and torch.equal(x['audio'], y['audio']) for x, y in zip(again, items))
        if epoch:
            assert [it['keys'] for it in items] != first
        else:
            first = [it['keys'] for it in items]
    assert 6 in seen and len(files_used) >= 4 and wraps > 0
    # the first draws of the stream (no redraw pass has touched it before them): a row that drew the silent file kept its own noise
    ld.set_epoch(0)
    order = ld.indices()
    drawn = D.draw_bank(8, bank.offsets, bank.total, D.bank_rng(2, 0, 0), ld.bank)
    keys = {k[0]: k for it in ld for k in it['keys']}
    for f, m in zip(order[:8], drawn):
        if f in keys:
            assert len(keys[f]) == (2 if m[0] == silent_noise else 6)
            assert m[0] == silent_noise or keys[f][3:] == m


def test_clean_only_dataset(D, folders, bank):
    Lc = 3000
    ds = D.DeviceDataset(folders[0], None, device='cuda:0')
    paired = D.DeviceDataset(folders[0], folders[1], device='cuda:0')
    assert not ds.paired and paired.paired and ds.noisy is ds.clean and ds.noisy.data_ptr() == ds.clean.data_ptr()
    assert ds.nbytes == 4 * ds.total and paired.nbytes == 8 * ds.total
    assert [os.path.basename(p) for p in ds.files] == [s[0] for s in SPEC] and ds.clean_files == ds.files
    assert ds.lengths == paired.lengths and torch.equal(ds.clean, paired.clean)
    assert D.DeviceDataset(folders[0], '', device='cuda:0').paired is False
    for kw in ({}, {'remix': D.Remix(1.0)}, {'bank': D.BankMix(bank, 0.5)}):
        with pytest.raises(ValueError):
            D.DeviceLoader(ds, 4, Lc, True, **kw)
    ld = D.DeviceLoader(ds, 4, Lc, shuffle=True, seed=4, bank=D.BankMix(bank, 1.0, (-5, 10)))
    delivered = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        for it in ld:
            assert it['audio'].shape == it['noisy'].shape == (len(it['keys']), Lc)
            for row, key in enumerate(it['keys']):
                assert len(key) == 6 and key[2] == 'bank' and key[3] != 5            # every delivered row is mixed
                f, s, _, j, sj, snr = key
                c = crop(ds.signal(f)[0], ds.lengths[f], s, Lc)
                assert torch.equal(it['audio'][row], c) and -5 <= snr <= 10
                check_mixed_row(c, wrapped(bank.signal(j), sj, Lc), it['noisy'][row], snr)
                delivered.append(f)
    # the all-zero utterance cannot be mixed (Pc == 0): redrawn, then dropped; every other one came through in both epochs
    assert sorted(delivered) == sorted(list(range(len(ds) - 1)) * 2)


def test_mix_bank_at_snr_is_the_definition(D, corpus, bank):
    ds = corpus
    # (utterance, bank file, start, snr): no wrap; a wrap near the end of the file; a file shorter than the utterance, many wraps
    for i, j, start, snr in ((3, 0, 777, 5.0), (4, 1, 13000, -3.0), (0, 4, 999, 12.5), (6, 3, 0, 0.0)):
        c, _ = ds.signal(i)
        n = ds.lengths[i]
        got_c, got_v = D.mix_bank_at_snr(ds, bank, i, j, snr, noise_start=start)
        assert got_c.shape == got_v.shape == (n,) and torch.equal(got_c, c)
        check_mixed_row(c, wrapped(bank.signal(j), start, n), got_v, snr)
    for start in (-1, bank.lengths[3]):
        with pytest.raises(ValueError):
            D.mix_bank_at_snr(ds, bank, 3, 3, 5.0, noise_start=start)
    # the silent file has no noise to give: the pair as stored
    got_c, got_v = D.mix_bank_at_snr(ds, bank, 1, 5, 5.0)
    assert torch.equal(got_c, ds.signal(1)[0]) and torch.equal(got_v, ds.signal(1)[1])


@pytest.mark.parametrize('clean_only', [False, True])
def test_main_gan_trains_with_a_noise_folder(D, tmp_path, caplog, capsys, clean_only):
    from speech_enhancement_amd import main_gan, train
    rs = np.random.RandomState(10)
    spec = [(f's{k}.wav', 48000 if k % 2 else 16000, n) for k, n in enumerate([60000, 18000, 52000, 20000])]
    tc, tn = make_corpus(tmp_path, rs, spec, 'train_clean', 'train_noisy')
    vc, vn = make_corpus(tmp_path, rs, spec[:2], 'test_clean', 'test_noisy')
    nd = make_noise(tmp_path / 'noise', rs, silent=False)
    train.set_pesq_provider(lambda clean_list, other_list: torch.full((len(clean_list),), 0.5))
    cache = train.label_cache()
    cache.q.clear()
    out = str(tmp_path / 'out')
    caplog.set_level(logging.INFO)
    try:
        main_gan.main(['--cfg', '/dev/null', '-a', 'scp', '-b', '2', '--epochs', '1', '--crop-len', '1', '--optimizer', 'adamw',
                       '--lr', '5e-4', '--output', out, '--gpu', '0', '-p', '1', '--noise-dir', nd, '--noise-snr', '0', '15',
                       '--opts', 'DATA.TRAIN_CLEAN_DIR', tc, 'DATA.TRAIN_NOISY_DIR', '' if clean_only else tn,
                       'DATA.TEST_CLEAN_DIR', vc, 'DATA.TEST_NOISY_DIR', vn, 'TRAIN.SCHEDULER.CYCLE_LIMIT', '1'])
    finally:
        train.set_pesq_provider(None)
    ck = torch.load(os.path.join(out, 'scp', 'default', 'checkpoint_0000.pth.tar'), map_location='cpu')
    assert ck['epoch'] == 1 and all(torch.isfinite(v).all() for v in ck['gen_state_dict'].values() if v.is_floating_point())
    line = [r.getMessage() for r in caplog.records if 'Train Generator Loss' in r.getMessage()]
    assert len(line) == 1
    losses = [float(v) for v in re.findall(r'Loss: (\S+)', line[0])]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), line
    assert len([r for r in caplog.records if r.getMessage().startswith('Train: [0/1]')]) == 2      # 4 files, batches of 2
    said = [l for l in capsys.readouterr().out.split('\n') if l.startswith('Noise bank:')]
    assert len(said) == 1 and re.fullmatch(r'Noise bank: 5 files, 0\.00 hours, \d+ bytes resident', said[0]), said
    # every training crop reached the label cache under its bank key (validation labels are not cached)
    assert cache.q and all(k[0] in ('clean', 'noisy') and len(k[1]) == 6 and k[1][2] == 'bank' for k in cache.q)
    assert sorted({k[1][0] for k in cache.q}) == list(range(4))
    assert all(0 <= k[1][5] <= 15 and 0 <= k[1][3] < 5 for k in cache.q)
