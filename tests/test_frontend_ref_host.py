"""CPU checks of tests/frontend_ref.py, the fp64 reference and the bars of tests/test_frontend_edges_gpu.py:
  1. the reference STFT / iSTFT equal torch.stft / torch.istft in fp64 (numpy's FFT where this torch has no CPU FFT) to 1e-10;
  2. a sequential fp32 emulation of every formula passes every bar, with no element left out;
  3. five deliberate slips of that emulation (a reflected tail one sample off, a frame taken from its neighbour at a tile edge, Re / Im
     swapped in one bin, a zeroed halo frame of an iSTFT tile, a hop of output taken from the neighbouring tile) fail their bars.
No GPU and no kernel of the project is involved: this shows that the bars are loose enough for fp32 and tight enough for a slip."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R  # noqa: E402

STFT_LENGTHS = [201, 3100, 3150, 3200, 6399, 6400]
ISTFT_FRAMES = [2, 4, 29, 30, 31, 59, 60]
C_ROWS = np.array([1.7, 0.6], np.float32)


def torch_stft(x, n_fft, hop):
    x = torch.from_numpy(np.asarray(x, np.float64))
    try:
        z = torch.stft(x, n_fft, hop, window=torch.hamming_window(n_fft, periodic=True, dtype=torch.float64), center=True,
                       pad_mode='reflect', onesided=True, return_complex=True)
        return z.real.numpy().transpose(0, 2, 1), z.imag.numpy().transpose(0, 2, 1)
    except RuntimeError:                                     # no CPU FFT in this build: numpy's
        z = np.fft.rfft(R.frames(x.numpy(), n_fft, hop) * R.hamming(n_fft), axis=-1)
        return z.real, z.imag


def torch_istft(re, im, n_fft, hop):
    z = torch.complex(torch.from_numpy(re), torch.from_numpy(im)).transpose(1, 2)
    try:
        return torch.istft(z, n_fft, hop, window=torch.hamming_window(n_fft, periodic=True, dtype=torch.float64), center=True,
                           onesided=True).numpy()
    except RuntimeError:
        fr = np.fft.irfft(re + 1j * im, n_fft, axis=-1) * R.hamming(n_fft)
        return R.ola(fr, n_fft, hop, R.envelope(n_fft, hop, re.shape[1]))


def close(a, b, rel=1e-10):
    return float(np.abs(a - b).max()) <= rel * float(np.abs(b).max())


@pytest.mark.parametrize('L,n_fft,hop', [(201, 400, 100), (3150, 400, 100), (3200, 400, 100), (6400, 400, 100), (4224, 512, 128)])
def test_reference_stft_is_torch_stft(L, n_fft, hop):
    x = R.signals(1, 2, L).astype(np.float64)
    re, im = R.stft(x, n_fft, hop)
    tre, tim = torch_stft(x, n_fft, hop)
    assert re.shape == tre.shape == (2, L // hop + 1, n_fft // 2 + 1)
    assert close(re, tre) and close(im, tim)
    # the scale is linear
    sre, sim = R.stft(x, n_fft, hop, c=np.array([1.7, 0.6]))
    assert close(sre, tre * np.array([1.7, 0.6])[:, None, None]) and close(sim, tim * np.array([1.7, 0.6])[:, None, None])


@pytest.mark.parametrize('T,n_fft,hop', [(2, 400, 100), (31, 400, 100), (60, 400, 100), (5, 512, 128)])
def test_reference_istft_is_torch_istft(T, n_fft, hop):
    rs = np.random.RandomState(T)
    re, im = rs.randn(2, T, n_fft // 2 + 1), rs.randn(2, T, n_fft // 2 + 1)
    im[..., 0] = im[..., -1] = 0.0                          # a one-sided spectrum's DC and Nyquist bins are real
    y = R.istft(re, im, n_fft, hop)
    assert y.shape == (2, hop * (T - 1)) and close(y, torch_istft(re, im, n_fft, hop))


def test_reference_round_trip_and_inverse_maps():
    x = R.signals(2, 2, 3200).astype(np.float64)
    re, im = R.stft(x)
    assert close(R.istft(re, im), x)
    for mode in R.MODES:
        mag, cre, cim = R.compress(re, im, mode)
        ure, uim = R.uncompress(cre, cim, mode)
        assert close(ure, re) and close(uim, im) and close(mag, np.hypot(cre, cim)), mode
    assert R.compress(np.zeros(3), np.zeros(3), 'pow')[1].tolist() == [0, 0, 0]
    assert R.uncompress(np.zeros(3), np.zeros(3), 'log')[0].tolist() == [0, 0, 0]


def test_adjoints_are_transposes():
    rs = np.random.RandomState(3)
    for L in (201, 202, 3150):
        x, g, c = rs.randn(2, L), rs.randn(2, L + 400), np.array([1.7, 0.6])
        dx, mag = R.reflect_pad_adjoint(g, L, 200, c)
        assert abs(np.sum(R.reflect_pad(x, 200, c) * g) - np.sum(x * dx)) <= 1e-12 * np.sum(np.abs(x) * mag * 1.7)
        assert (mag >= np.abs(g[:, 200:200 + L])).all()
    for T, n_fft, hop in ((2, 400, 100), (33, 512, 128)):
        env = R.envelope(n_fft, hop, T)
        fr, dy = rs.randn(2, T, n_fft), rs.randn(2, hop * (T - 1))
        lhs, rhs = np.sum(R.ola(fr, n_fft, hop, env) * dy), np.sum(fr * R.ola_adjoint(dy, env, T, n_fft, hop))
        assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(fr)) * np.abs(dy).max()


@pytest.mark.parametrize('n_fft,hop', [(400, 100), (512, 128)])
def test_the_project_matrices_are_the_reference_rounded_to_fp32(n_fft, hop):
    """frontend.dft_matrices reduces f k mod n before taking the angle: its entries are the fp64 ones rounded once, and the Im column
    of the Nyquist bin (sin(pi k)) is exactly zero -- at the unreduced angle it held noise of 1e-13, which the kernels turned into
    an Im part of 1e-14 where the bar (a multiple of sum |x| |W|) is zero"""
    from speech_enhancement_amd import frontend as FE
    FE._CACHE.pop((n_fft, hop, 'cpu'), None)
    Wf, Wi, _ = FE.dft_matrices(n_fft, hop, 'cpu')
    Fq = n_fft // 2 + 1
    assert np.array_equal(Wf.numpy().T, R.dft_matrix(n_fft).astype(np.float32))
    assert np.array_equal(Wi.numpy()[:, :2 * Fq].T, R.idft_matrix(n_fft).astype(np.float32)) and not Wi.numpy()[:, 2 * Fq:].any()
    assert not Wf.numpy()[Fq].any() and not Wf.numpy()[2 * Fq - 1].any()         # Im of DC and of Nyquist


# ---------------------------------------------------------------------------------------------------- the emulation passes the bars
@pytest.mark.parametrize('L', STFT_LENGTHS)
def test_fp32_emulation_passes_the_stft_bars(L):
    x = R.signals(10 + L, 2, L)
    re, im = R.stft(x, c=C_ROWS)
    bre, bim = R.stft_raw_bar(x, c=C_ROWS)
    ere, eim = R.emulate_stft(x, c=C_ROWS)
    w = max(R.check('Re', ere, re, bre), R.check('Im', eim, im, bim))
    emag = R.emulate_compress(ere, eim, 'none')[0]
    R.check('|z|', emag, np.hypot(re, im), R.stft_mag_bar(bre, bim, np.hypot(re, im)))
    assert w <= 0.05                 # sequential fp32 sits two orders of magnitude under the worst-case bar (the issue measured 1.1 %)
    for mode in ('norm', 'pow', 'log'):
        want = R.compress(ere, eim, mode)
        for name, g, r in zip(('mag', 're', 'im'), R.emulate_compress(ere, eim, mode), want):
            R.check(f'{mode} {name}', g, r, R.epilogue_bar(r))
    xp = R.frames32(x, c=C_ROWS)
    R.check('pad', xp, R.frames(x, c=C_ROWS), R.pad_bar(R.frames(x, c=C_ROWS)))


def test_fp32_emulation_passes_the_stft_bars_for_512_128():
    x = R.signals(5, 2, 4224)
    re, im = R.stft(x, 512, 128, c=C_ROWS)
    bre, bim = R.stft_raw_bar(x, 512, 128, c=C_ROWS)
    ere, eim = R.emulate_stft(x, 512, 128, c=C_ROWS)
    R.check('Re', ere, re, bre)
    R.check('Im', eim, im, bim)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('T', ISTFT_FRAMES)
def test_fp32_emulation_passes_the_istft_bar(T, mode):
    re, im = R.spectra(100 + T, 2, T)
    ru, iu = R.uncompress(re, im, mode)
    y = R.istft(ru, iu)
    got = R.emulate_istft(re, im, mode)
    assert R.check(f'T={T} {mode}', got, y, R.istft_bar(ru, iu, y)) <= 0.25


def gradient_inputs(seed, rows=33, Fq=201):
    """|z| log-uniform in [1e-3, 10] with exact zeros, random phases, upstream gradients of order 1"""
    rs = np.random.RandomState(seed)
    r = 10.0 ** rs.uniform(-3, 1, (rows, Fq))
    ph = rs.uniform(0, 2 * np.pi, (rows, Fq))
    re, im = (r * np.cos(ph)).astype(np.float32), (r * np.sin(ph)).astype(np.float32)
    zero = rs.rand(rows, Fq) < 0.03
    re[zero] = 0.0
    im[zero] = 0.0
    return re, im, rs.randn(3, rows, Fq).astype(np.float32)


@pytest.mark.parametrize('mode', R.MODES)
def test_fp32_emulation_passes_the_gradient_bars(mode):
    re, im, d = gradient_inputs(7)
    s = R.pre_scale(mode, 400)
    r = np.hypot(re.astype(np.float64), im.astype(np.float64))
    # compress_planes_bwd
    want = R.compress_vjp(re, im, d[0], d[1], d[2], mode)
    got = R.emulate_compress_bwd(re, im, d[0], d[1], d[2], mode)
    bar = R.grad_bar(R.compress_bwd_K(r * s, mode), np.abs(d).astype(np.float64).sum(0), s)
    for g, w in zip(got, want):
        R.check(f'compress_bwd {mode}', g, w, bar)
        assert (g[r == 0] == 0).all() and (w[r == 0] == 0).all() and np.isfinite(w).all()
    # uncompress_rows_bwd
    want = R.uncompress_vjp(re, im, d[1], d[2], mode)
    got = R.emulate_uncompress_bwd(re, im, d[1], d[2], mode)
    bar = R.grad_bar(R.uncompress_bwd_K(r, mode), np.abs(d[1:]).astype(np.float64).sum(0), 1.0 / s)
    for g, w in zip(got, want):
        R.check(f'uncompress_bwd {mode}', g, w, bar)
        assert (g[r == 0] == 0).all() and (w[r == 0] == 0).all()
        h_only = R.grad_bar(R.uncompress_bwd_K(r, mode, terms=False), np.abs(d[1:]).astype(np.float64).sum(0), 1.0 / s)
        print(f'uncompress_bwd {mode}: against 64 u h(r) alone {R.worst_ratio(g, w, h_only):.4f}')


@pytest.mark.parametrize('mode', R.MODES)
def test_fp32_emulation_passes_the_elementwise_bars(mode):
    re, im, _ = gradient_inputs(8)
    for g, w in zip(R.emulate_compress(re, im, mode), R.compress(re, im, mode)):
        R.check(f'compress {mode}', g, w, R.epilogue_bar(w))
    for g, w in zip(R.emulate_uncompress(re, im, mode), R.uncompress(re, im, mode)):
        R.check(f'uncompress {mode}', g, w, R.epilogue_bar(w))


# ---------------------------------------------------------------------------------------------------- the slips fail the bars
def fails(got, ref, bar):
    return R.worst_ratio(got, ref, bar) > 1.0


def test_a_one_sample_slip_in_the_reflected_tail_fails():
    L = 3150
    x = R.signals(20, 2, L)
    re, im = R.stft(x, c=C_ROWS)
    bre, bim = R.stft_raw_bar(x, c=C_ROWS)
    fr = R.frames32(x, c=C_ROWS)
    T = L // 100 + 1
    p = (T - 1) * 100 + np.arange(400) - 200                # sample indices of the last frame before reflection
    tail = p >= L
    assert tail.sum() == 150
    xs = x * C_ROWS[:, None]
    fr[:, T - 1, tail] = xs[:, 2 * (L - 1) - p[tail] - 1]   # mirrored about L - 1/2 instead of L - 1
    ere, eim = R.emulate_dft(fr)
    bad = np.abs(ere[:, T - 1] - re[:, T - 1]) > bre[:, T - 1]
    print('bins of the last frame over the bar:', bad.mean())
    assert bad.mean() > 0.9 and fails(ere, re, bre) and fails(eim, im, bim)
    assert not fails(ere[:, :T - 1], re[:, :T - 1], bre[:, :T - 1])


def test_a_frame_taken_from_its_neighbour_at_a_tile_edge_fails():
    x = R.signals(21, 2, 6400)
    re, im = R.stft(x, c=C_ROWS)
    bre, bim = R.stft_raw_bar(x, c=C_ROWS)
    fr = R.frames32(x, c=C_ROWS)
    for t in (32, 64):
        bad = fr.copy()
        bad[:, t] = fr[:, min(t + 1, 64)] if t < 64 else 0.0        # frame 64 is the last: a tile that stops one frame early leaves zeros
        ere, eim = R.emulate_dft(bad)
        assert fails(ere, re, bre) and fails(eim, im, bim), t


def test_re_and_im_swapped_in_one_bin_fails():
    x = R.signals(22, 2, 3200)
    re, im = R.stft(x, c=C_ROWS)
    bre, bim = R.stft_raw_bar(x, c=C_ROWS)
    ere, eim = R.emulate_stft(x, c=C_ROWS)
    assert not fails(ere, re, bre)
    ere, eim = ere.copy(), eim.copy()
    ere[1, 32, 17], eim[1, 32, 17] = eim[1, 32, 17], ere[1, 32, 17]
    assert fails(ere, re, bre) and fails(eim, im, bim)


@pytest.mark.parametrize('mode', ['none', 'pow'])
def test_a_zeroed_halo_frame_of_an_istft_tile_fails(mode):
    T = 60
    re, im = R.spectra(23, 2, T)
    ru, iu = R.uncompress(re, im, mode)
    y = R.istft(ru, iu)
    bar = R.istft_bar(ru, iu, y)
    fr = R.emulate_idft(*R.emulate_uncompress(re, im, mode))
    assert not fails(R.emulate_ola(fr), y, bar)
    for halo in (28, 29, 30):                                # tile 1 finishes padded hops 31 .. 59 from frames 28 .. 59
        assert R.istft_tile_of_hop(31) == (1, 28) and R.istft_tile_of_hop(30) == (0, -1)
        stale = fr.copy()
        stale[:, halo] = 0.0
        got = R.emulate_ola(fr, tile_frames=lambda h: stale if R.istft_tile_of_hop(h)[0] == 1 else fr)
        assert fails(got, y, bar), halo
        wrong = np.abs(got.astype(np.float64) - y) > bar
        assert not wrong[:, :2900].any() and wrong[:, 2900:3000].any()     # only tile 1's first hops see the halo


def test_a_hop_taken_from_the_neighbouring_tile_fails():
    T = 60
    re, im = R.spectra(24, 2, T)
    ru, iu = R.uncompress(re, im, 'log')
    y = R.istft(ru, iu)
    bar = R.istft_bar(ru, iu, y)
    good = R.emulate_istft(re, im, 'log')
    assert not fails(good, y, bar)
    for hop_out in (28, 29, 57):                             # output hop = padded hop - 2: last of tile 0, first of tile 1, last of tile 1
        got = good.copy()
        src = hop_out + 29 if hop_out + 29 < T - 1 else hop_out - 29
        got[:, hop_out * 100:hop_out * 100 + 100] = good[:, src * 100:src * 100 + 100]
        assert fails(got, y, bar), hop_out
