"""Per-element fp64 tests of the STFT / iSTFT front end at the edges of its tiles: the fused kernels of csrc/se_front.hip
(stft_fused_kernel: tiles of 32 frames, reflect padding at both ends, a lane-pair shuffle in the epilogue; istft_fused_kernel: 29
hops per workgroup from 32 staged frames, 3 of them halo) and their elementwise relatives in csrc/se_elem.hip, called through
frontend / ops.  The reference, the bars and a sequential fp32 emulation live in tests/frontend_ref.py; each bar is derived in the
docstring of its function there, and tests/test_frontend_ref_host.py shows on the CPU that fp32 passes them and a one-sample or
one-frame slip does not.  u = 2^-24 throughout.

  raw STFT bin            (n_fft + 4) u sum_k |c x_k| |W_kf|             worst-case fp32 dot product + rounding of matrix and scale
  |z|                     the two in quadrature + 4 u |z|
  'pow' / 'log' / 'norm'  32 u |value| + 1e-30, against the fp64 compression of the kernel's own 'none' planes (same launch inputs)
  xp (padded=True)        2 u |value|
  iSTFT sample            (404 + 4 + 32) u sum |A_u| |Wi| / env + 4 u |y|
  RMS error               <= 2 x the RMS error of the sequential fp32 emulation at the same inputs (fused kernels)
  clip_scale              2 u relative (the kernel sums in fp64)
  reflect_pad_bwd         4 u (sum of the <= 3 |terms|) |c|
  (un)compress            32 u |value|
  (un)compress backward   64 u K(r) (sum of upstream magnitudes) scale, K from frontend_ref.compress_bwd_K / uncompress_bwd_K;
                          uncompress_rows_bwd adds into dP, which costs one more rounding of the sum: + u |dP after|
  ola / ola_bwd           6 u sum |terms| / env

No element is left out of any comparison.  Every test prints the largest err / bar it saw."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U
C_ROWS = np.array([1.7, 0.6], np.float32)
STFT_LENGTHS = [201, 3100, 3150, 3200, 6399, 6400]
ISTFT_FRAMES = [2, 4, 29, 30, 31, 59, 60]
NAN = float('nan')


@pytest.fixture(scope='module')
def FE():
    from speech_enhancement_amd import frontend
    return frontend


@pytest.fixture(scope='module')
def O():
    from speech_enhancement_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared cases are read-only


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def stft_case(L, n_fft=400, hop=100, scaled=True):
    """inputs, fp64 reference, bars and the fp32 emulation of one STFT case, computed once and shared by the tests of that length"""
    x = R.signals(10 + L, 2, L)
    c = C_ROWS if scaled else None
    re, im = R.stft(x, n_fft, hop, c)
    bre, bim = R.stft_raw_bar(x, n_fft, hop, c)
    ere, eim = R.emulate_stft(x, n_fft, hop, c)
    emu_rms = R.rms(np.concatenate([ere - re, eim - im]))
    for a in (x, re, im, bre, bim):
        a.setflags(write=False)
    return x, re, im, bre, bim, emu_rms


def check_raw_planes(P, L, n_fft, hop, case, tag):
    x, re, im, bre, bim, emu_rms = case
    T, Fq = L // hop + 1, n_fft // 2 + 1
    P = host(P)
    assert P.shape == (2, T, Fq, 4) and np.isfinite(P).all()
    assert (P[..., 3] == 0).all()
    R.check(f'{tag} Re', P[..., 1], re, bre)
    R.check(f'{tag} Im', P[..., 2], im, bim)
    mag = np.hypot(re, im)
    R.check(f'{tag} |z|', P[..., 0], mag, R.stft_mag_bar(bre, bim, mag))
    ratio = R.rms(np.concatenate([P[..., 1] - re, P[..., 2] - im])) / emu_rms
    print(f'{tag}: RMS error / RMS error of the sequential fp32 emulation = {ratio:.3f}')
    return ratio


# ------------------------------------------------------------------------------------------------ fused STFT
@pytest.mark.parametrize('L', STFT_LENGTHS)
def test_fused_stft_none_against_fp64(FE, L):
    case = stft_case(L)
    P, xp = FE.stft_planes(dev(case[0]), 400, 100, 'none', scale=dev(C_ROWS), padded=False)
    assert xp is None
    assert check_raw_planes(P, L, 400, 100, case, f'L={L}') <= 2.0


@pytest.mark.parametrize('mode', ['norm', 'pow', 'log'])
@pytest.mark.parametrize('L', STFT_LENGTHS)
def test_fused_stft_epilogue_against_its_own_raw_planes(FE, L, mode):
    x, c = dev(stft_case(L)[0]), dev(C_ROWS)
    raw = host(FE.stft_planes(x, 400, 100, 'none', scale=c, padded=False)[0])
    P = host(FE.stft_planes(x, 400, 100, mode, scale=c, padded=False)[0])
    assert P.shape == raw.shape and np.isfinite(P).all() and (P[..., 3] == 0).all()
    for ch, want in enumerate(R.compress(raw[..., 1], raw[..., 2], mode)):
        R.check(f'L={L} {mode} channel {ch}', P[..., ch], want, R.epilogue_bar(want))


@pytest.mark.parametrize('mode', ['pow', 'log', 'none', 'norm'])
def test_fused_stft_of_zero_frames_is_exactly_zero(FE, mode):
    L = 3200
    x = R.signals(3, 2, L)
    x[:, :700] = 0.0
    # frame t reads samples |100 t - 200| .. 100 t + 199: all zero for t <= 5
    P = host(FE.stft_planes(dev(x), 400, 100, mode, scale=dev(C_ROWS), padded=False)[0])
    assert np.isfinite(P).all()
    assert (P[:, :6] == 0).all() and (P[:, 6:, :, 0] > 0).all()
    print(f'{mode}: frames 0 .. 5 are exact zeros, err/bar 0')


def test_fused_stft_padded_returns_the_scaled_reflect_pad(FE):
    L = 3200
    x, c = dev(stft_case(L)[0]), dev(C_ROWS)
    P, xp = FE.stft_planes(x, 400, 100, 'pow', scale=c, padded=True)
    want = R.reflect_pad(stft_case(L)[0], 200, C_ROWS)
    assert xp.shape == (2, L + 400)
    R.check('xp', host(xp), want, R.pad_bar(want))
    P2, none = FE.stft_planes(x, 400, 100, 'pow', scale=c, padded=False)
    assert none is None and torch.equal(P, P2)


# ------------------------------------------------------------------------------------------------ unfused STFT forward
def test_unfused_stft_forward_of_stft_planes_grad(FE):
    """the differentiable re-STFT: reflect_pad_scale -> tap GEMM -> compress_planes.  Its descriptor carries precision 0 (the exact
    fp32 MFMA kernel), so the fp32 worst-case bar of the fused kernel applies unchanged."""
    from speech_enhancement_amd import gemm as GM
    L, B = 3200, 2
    T = L // 100 + 1
    assert GM.make_desc(B, 1, T, 1, (L + 400) // 100, [(0, 0)], 400, 100, 402, 404, ldw=400).precision == 0
    case = stft_case(L, scaled=False)
    x = dev(case[0])
    raw = FE.stft_planes_grad(x, 400, 100, 'none')
    check_raw_planes(raw, L, 400, 100, case, 'stft_planes_grad')
    raw = host(raw)
    for mode in ('norm', 'pow', 'log'):
        P = host(FE.stft_planes_grad(x, 400, 100, mode))
        assert np.isfinite(P).all() and (P[..., 3] == 0).all()
        for ch, want in enumerate(R.compress(raw[..., 1], raw[..., 2], mode)):
            R.check(f'stft_planes_grad {mode} channel {ch}', P[..., ch], want, R.epilogue_bar(want))


def test_unfused_stft_of_another_analysis(FE):
    """n_fft = 512, hop = 128 through stft_planes: the pad -> tap GEMM -> compress sequence, again with a precision-0 descriptor"""
    from speech_enhancement_amd import gemm as GM
    L, n_fft, hop = 4224, 512, 128
    T = L // hop + 1
    assert GM.make_desc(2, 1, T, 1, (L + n_fft) // hop, [(0, 0)], n_fft, hop, 514, 516, ldw=n_fft).precision == 0
    case = stft_case(L, n_fft, hop)
    P, xp = FE.stft_planes(dev(case[0]), n_fft, hop, 'none', scale=dev(C_ROWS))
    check_raw_planes(P, L, n_fft, hop, case, '512/128')
    want = R.reflect_pad(case[0], n_fft // 2, C_ROWS)
    R.check('512/128 xp', host(xp), want, R.pad_bar(want))


# ------------------------------------------------------------------------------------------------ fused iSTFT
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('T', ISTFT_FRAMES)
def test_fused_istft_against_fp64(FE, T, mode):
    re, im = R.spectra(100 + T, 2, T)
    assert ((re == 0) & (im == 0)).sum() > 0 and np.hypot(re, im).max() <= 2.0001
    planes = np.full((2, T, 201, 4), NAN, np.float32)        # channels 0 and 3 are not part of the definition: never read
    planes[..., 1], planes[..., 2] = re, im
    y = host(FE.istft_planes(dev(planes), 400, 100, mode))
    assert y.shape == (2, 100 * (T - 1)) and np.isfinite(y).all()
    ru, iu = R.uncompress(re, im, mode)
    want = R.istft(ru, iu)
    R.check(f'T={T} {mode}', y, want, R.istft_bar(ru, iu, want))
    ratio = R.rms(y - want) / R.rms(R.emulate_istft(re, im, mode) - want)
    print(f'T={T} {mode}: RMS error / RMS error of the sequential fp32 emulation = {ratio:.3f}')
    assert ratio <= 2.0


# ------------------------------------------------------------------------------------------------ clip_scale
@pytest.mark.parametrize('L', [12, 201, 202, 3076, 4096, 4100, 32000])
def test_clip_scale_against_fp64(O, L):
    x = R.signals(L, 3, L)
    want = np.sqrt(L / np.sum(x.astype(np.float64) ** 2, axis=1))
    c = O.clip_scale(dev(x))
    assert c.shape == (3,)
    R.check(f'clip_scale L={L}', host(c), want, R.clip_scale_bar(want))


def test_clip_scale_of_a_view_off_16_byte_alignment(O):
    """a contiguous [3, 4096] view that starts 4 bytes into its buffer: L % 4 == 0, yet no row is 16-byte aligned -> the scalar loop"""
    L = 4096
    x = R.signals(L, 3, L)
    buf = torch.zeros(3 * L + 4, dtype=torch.float32, device='cuda')
    view = buf[1:1 + 3 * L].view(3, L)
    view.copy_(dev(x))
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    want = np.sqrt(L / np.sum(x.astype(np.float64) ** 2, axis=1))
    R.check('clip_scale off alignment', host(O.clip_scale(view)), want, R.clip_scale_bar(want))
    R.check('clip_scale aligned', host(O.clip_scale(dev(x))), want, R.clip_scale_bar(want))


# ------------------------------------------------------------------------------------------------ reflect_pad_scale / _bwd
@pytest.mark.parametrize('scaled', [True, False], ids=['c', 'no-c'])
@pytest.mark.parametrize('L', [201, 202, 400, 401, 3150])
def test_reflect_pad_and_its_backward(O, L, scaled):
    pad = 200
    x = R.signals(L + 1, 2, L)
    g = np.random.RandomState(L).randn(2, L + 2 * pad).astype(np.float32)
    c = C_ROWS if scaled else None
    dc = dev(C_ROWS) if scaled else None
    xp = host(O.reflect_pad_scale(dev(x), dc, pad))
    want = R.reflect_pad(x, pad, c)
    if scaled:
        R.check(f'reflect_pad L={L}', xp, want, R.pad_bar(want))
    else:
        assert np.array_equal(xp.astype(np.float64), want)
        print(f'reflect_pad L={L}: exact copy, err/bar 0')
    dx = host(O.reflect_pad_bwd(dev(g), dc, 2, L, pad))
    ref, mag = R.reflect_pad_adjoint(g, L, pad, c)
    R.check(f'reflect_pad_bwd L={L}', dx, ref, R.reflect_pad_bwd_bar(mag, c))
    # <pad(x), g> == <x, pad_bwd(g)> on the kernels' outputs, with non-negative operands so that 'relative' has a denominator that does not cancel
    xa, ga = np.abs(x), np.abs(g)
    xp, dx = host(O.reflect_pad_scale(dev(xa), dc, pad)), host(O.reflect_pad_bwd(dev(ga), dc, 2, L, pad))
    lhs, rhs = np.sum(xp.astype(np.float64) * ga), np.sum(xa.astype(np.float64) * dx)
    print(f'<pad(x), g> = {lhs:.9e}  <x, pad_bwd(g)> = {rhs:.9e}  relative difference {abs(lhs - rhs) / abs(lhs):.2e}')
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)


# ------------------------------------------------------------------------------------------------ (un)compression
def bins(seed, rows, Fq=201):
    """|z| log-uniform in [1e-3, 10] with exact zeros, random phases -> (re, im) fp32 [rows, F]"""
    rs = np.random.RandomState(seed)
    r = 10.0 ** rs.uniform(-3, 1, (rows, Fq))
    ph = rs.uniform(0, 2 * np.pi, (rows, Fq))
    re, im = (r * np.cos(ph)).astype(np.float32), (r * np.sin(ph)).astype(np.float32)
    zero = rs.rand(rows, Fq) < 0.03
    re[zero] = 0.0
    im[zero] = 0.0
    assert zero.sum() > 0
    return re, im


def as_rows(re, im, ld, fill=NAN):
    """GEMM layout [rows, ld]: re | im | `fill` in the pad columns"""
    rows, Fq = re.shape
    A = np.full((rows, ld), fill, np.float32)
    A[:, :Fq], A[:, Fq:2 * Fq] = re, im
    return A


def as_planes(re, im, ch0=NAN, ch3=NAN):
    P = np.empty(re.shape + (4,), np.float32)
    P[..., 0], P[..., 1], P[..., 2], P[..., 3] = ch0, re, im, ch3
    return P


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('rows', [1, 33])
def test_compress_planes_and_uncompress_rows(O, rows, mode):
    Fq, ldr, lda = 201, 404, 408
    re, im = bins(rows, rows)
    s = R.pre_scale(mode, 400)
    P = host(O.compress_planes(dev(as_rows(re, im, ldr)), ldr, rows, Fq, mode, s))
    assert P.shape == (rows, Fq, 4) and np.isfinite(P).all() and (P[..., 3] == 0).all()
    for ch, want in enumerate(R.compress(re, im, mode)):
        R.check(f'compress_planes {mode} rows={rows} channel {ch}', P[..., ch], want, R.epilogue_bar(want))
    assert (P[(re == 0) & (im == 0)] == 0).all()
    A = host(O.uncompress_rows(dev(as_planes(re, im)), rows, Fq, lda, mode, 1.0 / s))
    assert A.shape == (rows, lda) and np.isfinite(A).all() and (A[:, 2 * Fq:] == 0).all()
    for name, got, want in zip(('Re', 'Im'), (A[:, :Fq], A[:, Fq:2 * Fq]), R.uncompress(re, im, mode)):
        R.check(f'uncompress_rows {mode} rows={rows} {name}', got, want, R.epilogue_bar(want))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('rows', [1, 33])
def test_compress_and_uncompress_backward_against_autograd(O, rows, mode):
    Fq, ldr, lda = 201, 404, 408
    re, im = bins(40 + rows, rows)
    rs = np.random.RandomState(50 + rows)
    d = rs.randn(3, rows, Fq).astype(np.float32)
    s = R.pre_scale(mode, 400)
    r = np.hypot(re.astype(np.float64), im.astype(np.float64))
    zero = r == 0
    # compress_planes_bwd: dP (d|z|', dRe', dIm', unused) -> dR [rows, ldr]
    dP = as_planes(d[1], d[2], ch0=d[0])
    dR = host(O.compress_planes_bwd(dev(as_rows(re, im, ldr)), ldr, dev(dP), rows, Fq, mode, s))
    assert dR.shape == (rows, ldr) and np.isfinite(dR).all() and (dR[:, 2 * Fq:] == 0).all()
    bar = R.grad_bar(R.compress_bwd_K(r * s, mode), np.abs(d).astype(np.float64).sum(0), s)
    for name, got, want in zip(('Re', 'Im'), (dR[:, :Fq], dR[:, Fq:2 * Fq]), R.compress_vjp(re, im, d[0], d[1], d[2], mode)):
        R.check(f'compress_planes_bwd {mode} rows={rows} {name}', got, want, bar)
        assert (got[zero] == 0).all() and (want[zero] == 0).all()
    # uncompress_rows_bwd adds to channels 1 and 2 of a dP that is not zero, and leaves channels 0 and 3 alone
    dP0 = rs.randn(rows, Fq, 4).astype(np.float32)
    dP1 = host(O.uncompress_rows_bwd(dev(as_planes(re, im)), dev(as_rows(d[1], d[2], lda)), lda, dev(dP0), rows, Fq, mode, 1.0 / s))
    assert np.array_equal(dP1[..., 0].view(np.uint32), dP0[..., 0].view(np.uint32))
    assert np.array_equal(dP1[..., 3].view(np.uint32), dP0[..., 3].view(np.uint32))
    dsum = np.abs(d[1:]).astype(np.float64).sum(0)
    bar = R.grad_bar(R.uncompress_bwd_K(r, mode), dsum, 1.0 / s)
    h_only = R.grad_bar(R.uncompress_bwd_K(r, mode, terms=False), dsum, 1.0 / s)
    for ch, want in zip((1, 2), R.uncompress_vjp(re, im, d[1], d[2], mode)):
        total = dP0[..., ch].astype(np.float64) + want
        R.check(f'uncompress_rows_bwd {mode} rows={rows} channel {ch}', dP1[..., ch], total, bar + U * np.abs(total))
        print(f'   against 64 u h(r) alone: {R.worst_ratio(dP1[..., ch], total, h_only + U * np.abs(total)):.4f}')
        assert np.array_equal(dP1[..., ch][zero].view(np.uint32), dP0[..., ch][zero].view(np.uint32))


# ------------------------------------------------------------------------------------------------ overlap-add
@pytest.mark.parametrize('n_fft,hop', [(400, 100), (512, 128)])
@pytest.mark.parametrize('T', [2, 5, 33])
def test_ola_and_its_backward(O, T, n_fft, hop):
    B, L = 2, hop * (T - 1)
    rs = np.random.RandomState(T + n_fft)
    fr = rs.randn(B, T, n_fft).astype(np.float32)
    dy = rs.randn(B, L).astype(np.float32)
    env = R.envelope(n_fft, hop, T).astype(np.float32)       # the reference divides by the same fp32 envelope
    dfr, denv = dev(fr.reshape(B * T, n_fft)), dev(env)
    # the iSTFT's call: envelope, trim = n_fft / 2
    y = host(O.ola(dfr, denv, B, T, n_fft, hop))
    want = R.ola(fr, n_fft, hop, env)
    assert y.shape == (B, L)
    R.check(f'ola T={T} {n_fft}/{hop}', y, want, R.ola_bar(R.ola(fr, n_fft, hop, env, absolute=True)))
    # the STFT backward's call: no envelope, no trim, the whole padded length
    full = host(O.ola(dfr, None, B, T, n_fft, hop, trim=0, L_out=L + n_fft))
    want_full = R.ola(fr, n_fft, hop, None, trim=0, L_out=L + n_fft)
    assert full.shape == (B, L + n_fft)
    R.check(f'ola env=None T={T} {n_fft}/{hop}', full, want_full, R.ola_bar(R.ola(fr, n_fft, hop, None, 0, L + n_fft, absolute=True)))
    # the transpose
    g = host(O.ola_bwd(dev(dy), denv, B, T, n_fft, hop)).reshape(B, T, n_fft)
    want_g = R.ola_adjoint(dy, env, T, n_fft, hop)
    R.check(f'ola_bwd T={T} {n_fft}/{hop}', g, want_g, R.ola_bar(np.abs(want_g)))
    # <ola(fr), dy> == <fr, ola_bwd(dy)> on the kernels' outputs, with non-negative operands so that 'relative' has a denominator that does not cancel
    fa, da = np.abs(fr), np.abs(dy)
    y, g = host(O.ola(dev(fa.reshape(B * T, n_fft)), denv, B, T, n_fft, hop)), host(O.ola_bwd(dev(da), denv, B, T, n_fft, hop)).reshape(B, T, n_fft)
    lhs, rhs = np.sum(y.astype(np.float64) * da), np.sum(fa.astype(np.float64) * g)
    print(f'<ola(fr), dy> = {lhs:.9e}  <fr, ola_bwd(dy)> = {rhs:.9e}  relative difference {abs(lhs - rhs) / abs(lhs):.2e}')
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)
