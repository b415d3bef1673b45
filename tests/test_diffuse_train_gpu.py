"""GPU tests of the hybrid's training prologue on the device (csrc/se_sampler.hip: se_diffuse_draw_steps, se_diffuse_noise), of the
seeded training step and of the main_diffuse command line."""
import json
import logging
import math
import os
import re
import sys
import types
import wave
from unittest import mock

import numpy as np
import pytest
import torch

import formula

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampler_host import FAST, NOISE_SCHEDULE, sampler_words  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def TD():
    import __graft_entry__
    __graft_entry__.build()
    from speech_enhancement_amd import tsc_diffusion
    return tsc_diffusion


@pytest.fixture(scope='module')
def gtt():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_tsc_train.npz'))


def oracle_add_noise_f64(xc, xn, schedule, t, z):
    """oracle.tsc_oracle.add_noise evaluated in fp64.  The oracle keeps noise_level -- cumprod(1 - beta) rounded to fp32, the
    reference's starting values -- in an fp32 tensor, so with fp64 signals its coefficient arithmetic would still be fp32 (and
    1 - (1 + m^2) noise_level cancels to nothing at the first steps); here the same rounded values are handed to it as fp64, which
    makes every operation of its expression fp64."""
    from oracle import tsc_oracle as TO
    as_f64 = lambda a, **kw: torch.as_tensor(np.asarray(a, np.float64))
    with mock.patch.object(torch, 'tensor', as_f64):
        x_t, combine = TO.add_noise(xc, xn, schedule, t, z)
    assert x_t.dtype == torch.float64 and combine.dtype == torch.float64
    return x_t.numpy(), combine.numpy()


def check_supplied(TD, clean, noisy, t, noise, schedule):
    """se_diffuse_noise with supplied noise against the fp64 oracle, elementwise:
      |x_t - ref| <= 8 eps (|A xc| + |Bn xn| + |S z|),   |combine - ref| <= 8 eps (G (|xc| + |xn|) + H |z|),   eps = 2^-24
    (at most five roundings per term: coefficient, input product, term product, two additions; the subtraction xn - xc cancels, hence
    |xc| + |xn|), and noisy_n == torch's noisy * c[:, None] bit for bit."""
    from speech_enhancement_amd import ops
    c = ops.clip_scale(noisy)
    coef = torch.from_numpy(TD.noise_coefficients(schedule)).cuda()
    noisy_n, x_t, combine = TD.diffusion_noise(clean, noisy, c, coef, t, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(noisy_n, noisy * c[:, None])
    c64 = c.double().cpu()[:, None]
    xc, xn, z = clean.double().cpu() * c64, noisy.double().cpu() * c64, noise.double().cpu()
    ref_x, ref_c = oracle_add_noise_f64(xc, xn, schedule, t.cpu(), z)
    k = TD.noise_coefficients(schedule).astype(np.float64)[t.cpu().numpy()]
    A, Bn, S, G, H = (k[:, j:j + 1] for j in range(5))
    xc, xn, z = xc.numpy(), xn.numpy(), z.numpy()
    bx = 8 * EPS * (np.abs(A * xc) + np.abs(Bn * xn) + np.abs(S * z))
    bc = 8 * EPS * (G * (np.abs(xc) + np.abs(xn)) + H * np.abs(z))
    ex, ec = np.abs(x_t.double().cpu().numpy() - ref_x), np.abs(combine.double().cpu().numpy() - ref_c)
    print(f'B x L {tuple(clean.shape)} t {t.tolist()}: worst err / bound  x_t {np.max(ex / np.maximum(bx, 1e-300)):.3f}  '
          f'combine {np.max(ec / np.maximum(bc, 1e-300)):.3f}')
    assert np.all(ex <= bx), np.argwhere(ex > bx)[:4]
    assert np.all(ec <= bc), np.argwhere(ec > bc)[:4]


def test_supplied_noise_on_the_golden_batch(TD, gtt):
    clean, noisy = torch.from_numpy(gtt['clean']).cuda(), torch.from_numpy(gtt['noisy']).cuda()
    t, noise = torch.from_numpy(gtt['t']).cuda(), torch.from_numpy(gtt['noise']).float().cuda()
    check_supplied(TD, clean, noisy, t, noise, NOISE_SCHEDULE)


@pytest.mark.parametrize('Ls', [1, 3, 1023, 1025, 4097])
@pytest.mark.parametrize('schedule', [NOISE_SCHEDULE, FAST], ids=['linspace50', 'fast6'])
def test_supplied_noise_on_unaligned_rows(TD, Ls, schedule):
    """B = 3 with rows that are no multiple of four samples: groups straddle rows (all three at L = 1); t holds 0 and steps - 1"""
    rs = np.random.RandomState(100 + Ls)
    B, steps = 3, len(schedule)
    clean = (0.1 * rs.randn(B, Ls)).astype(np.float32)
    noisy = (clean + 0.05 * rs.randn(B, Ls)).astype(np.float32)
    t = torch.tensor([0, steps - 1, steps // 2]).cuda()
    noise = torch.from_numpy(rs.randn(B, Ls).astype(np.float32)).cuda()
    check_supplied(TD, torch.from_numpy(clean).cuda(), torch.from_numpy(noisy).cuda(), t, noise, schedule)


def test_supplied_noise_from_a_base_address_off_16_bytes(TD):
    """inputs that start one float into an allocation: the element-by-element form of the kernel gives what the 16-byte form gives"""
    from speech_enhancement_amd import ops
    rs = np.random.RandomState(5)
    B, Ls = 3, 1025
    buf = [torch.from_numpy((0.1 * rs.randn(B * Ls + 1)).astype(np.float32)).cuda() for _ in range(3)]
    off = [b[1:].view(B, Ls) for b in buf]
    assert all(x.is_contiguous() and x.data_ptr() % 16 == 4 for x in off)
    al = [x.clone() for x in off]
    t = torch.tensor([0, 49, 17]).cuda()
    coef = torch.from_numpy(TD.noise_coefficients(NOISE_SCHEDULE)).cuda()
    c = ops.clip_scale(al[1])
    want = TD.diffusion_noise(al[0], al[1], c, coef, t, noise=al[2])
    got = TD.diffusion_noise(off[0], off[1], c, coef, t, noise=off[2])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    check_supplied(TD, off[0], off[1], t, off[2], NOISE_SCHEDULE)
    want = TD.diffusion_noise(al[0], al[1], c, coef, t, seed=3, c2=1, c3=2)
    got = TD.diffusion_noise(off[0], off[1], c, coef, t, seed=3, c2=1, c3=2)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def drawn(TD, B, Ls, seed, c2, c3):
    """x_t and combine with the coefficient rows (0, 0, 1, 0, 1): the drawn noise itself"""
    rs = np.random.RandomState(B * Ls)
    clean = torch.from_numpy((0.1 * rs.randn(B, Ls)).astype(np.float32)).cuda()
    noisy = torch.from_numpy((0.1 * rs.randn(B, Ls)).astype(np.float32)).cuda()
    coef = torch.tensor([[0.0, 0.0, 1.0, 0.0, 1.0]] * 4).cuda()
    t = (torch.arange(B) % 4).cuda()
    c = torch.ones(B).cuda()
    _, x_t, combine = TD.diffusion_noise(clean, noisy, c, coef, t, seed=seed, c2=c2, c3=c3)
    return x_t, combine


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_drawn_noise_is_the_sampler_generator(TD):
    from speech_enhancement_amd import sampler
    seed, c2, c3 = 0x1234567887654321, 11, (1 << 31) | 5
    out = {}
    for B, Ls in ((1, 1000), (3, 1025), (1, 100000)):
        x_t, combine = drawn(TD, B, Ls, seed, c2, c3)
        _, z = sampler.philox_normal(seed, c2, c3, 0, -(-B * Ls // 4))
        torch.cuda.synchronize()
        assert same_bits(x_t.view(-1), z[:B * Ls]) and same_bits(combine.view(-1), z[:B * Ls]), (B, Ls)
        out[(B, Ls)] = x_t.view(-1)
        again, _ = drawn(TD, B, Ls, seed, c2, c3)
        assert same_bits(again, x_t)                                    # the same (seed, c2, c3): the same draw
    assert same_bits(out[(1, 100000)][:1000], out[(1, 1000)])           # a draw does not depend on the launch geometry
    assert same_bits(out[(3, 1025)][:1000], out[(1, 1000)])             # ... nor on the row length
    base = out[(1, 1000)]
    for other in ((seed, c2 + 1, c3), (seed, c2, c3 ^ 1), (seed + 1, c2, c3)):
        assert not torch.equal(drawn(TD, 1, 1000, *other)[0].view(-1), base), other
    assert abs(float(out[(1, 100000)].mean())) < 0.02 and abs(float(out[(1, 100000)].std()) - 1) < 0.02


@pytest.mark.parametrize('seed', [0, 2 ** 64 - 1])
def test_step_draw_is_the_numpy_formula(TD, seed):
    for B in (1, 16, 4096):
        for steps in (1, 6, 50):
            t = TD.draw_steps(seed, 3, 1 << 30, B, steps)
            assert t.dtype == torch.int64 and t.shape == (B,)
            w0 = sampler_words(seed, 3, 1 << 30, 0, B).reshape(B, 4)[:, 0].astype(np.uint64)
            want = ((w0 * np.uint64(steps)) >> np.uint64(32)).astype(np.int64)
            assert np.array_equal(t.cpu().numpy(), want), (B, steps)
    assert not torch.equal(TD.draw_steps(seed, 3, 1 << 30, 4096, 50), TD.draw_steps(seed, 4, 1 << 30, 4096, 50))


@pytest.mark.parametrize('bad', [50, -1])
@pytest.mark.parametrize('supplied', [True, False])
def test_a_step_outside_the_table_zeroes_its_row_only(TD, bad, supplied):
    """the contract of se_diffuse_noise for t[b] outside [0, steps): zeros in that row's three outputs, the other rows as without it
    (the kernel compares t[b] with the table's length before it indexes the table)"""
    from speech_enhancement_amd import ops
    rs = np.random.RandomState(9)
    B, Ls = 4, 1025                                # rows that begin inside a group of four
    clean = torch.from_numpy((0.1 * rs.randn(B, Ls)).astype(np.float32)).cuda()
    noisy = torch.from_numpy((0.1 * rs.randn(B, Ls)).astype(np.float32)).cuda()
    noise = torch.from_numpy(rs.randn(B, Ls).astype(np.float32)).cuda()
    coef = torch.from_numpy(TD.noise_coefficients(NOISE_SCHEDULE)).cuda()
    c = ops.clip_scale(noisy)
    kw = {'noise': noise} if supplied else {'seed': 5, 'c2': 1, 'c3': 2}
    good = torch.tensor([3, 20, 49, 0]).cuda()
    want = TD.diffusion_noise(clean, noisy, c, coef, good, **kw)
    t = good.clone()
    t[1] = bad
    got = TD.diffusion_noise(clean, noisy, c, coef, t, **kw)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert float(g[1].abs().max()) == 0.0
        assert torch.equal(g[[0, 2, 3]], w[[0, 2, 3]])


def test_wrapper_rejects_what_the_kernel_cannot_take(TD):
    from speech_enhancement_amd import _lib
    x = torch.zeros(2, 8).cuda()
    c, t = torch.ones(2).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    coef = torch.from_numpy(TD.noise_coefficients(FAST)).cuda()
    E = _lib.SeHipError
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c, coef, t)                                        # neither noise nor seed
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c, coef, t, noise=x, seed=1)                       # both
    with pytest.raises(E):
        TD.diffusion_noise(x, x[:, :4].contiguous(), c, coef, t, seed=1)            # shapes
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c, coef[:, :4].contiguous(), t, seed=1)
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c[:1], coef, t, seed=1)
    with pytest.raises(E):
        TD.diffusion_noise(x, torch.zeros(8, 2).cuda().t(), c, coef, t, seed=1)     # not contiguous
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c, coef, t.int(), seed=1)                          # t must be int64
    with pytest.raises(E):
        TD.diffusion_noise(x, x, c, coef, t, noise=x.cpu())


def _train_model():
    import speech_enhancement_amd as S
    from speech_enhancement_amd import optim
    m = S.TSCNetDiffusion(64, 201, NOISE_SCHEDULE)
    m.load_state_dict(formula.tsc_state())
    m.cuda().train()
    m.set_dropout(0.0, 0.0)
    args = types.SimpleNamespace(optimizer='sgd', lr=0.01, weight_decay=0.01, momentum=0.9, max_norm=0.0)
    return m, optim.build_optimizer(args, m)


def test_seeded_step_is_the_supplied_noise_step(TD, gtt):
    """tsc_diffusion_step(seed=7, counter=(3, 0)) against tsc_diffusion_step(t=T, noise=Z) with T, Z regenerated from the counters the
    seeded step uses: the noise from (c2, c3) = (3, 0), the steps from (3, 0 | STEP_STREAM).  The losses agree within
    1e-5 loss + 3 |step_f32_loss - step_f64_loss| of the golden: the reference loop's own fp32-vs-fp64 spread at this shape."""
    from speech_enhancement_amd import _lib, sampler
    clean, noisy = torch.from_numpy(gtt['clean']).cuda(), torch.from_numpy(gtt['noisy']).cuda()
    B, Ls = clean.shape
    m, opt = _train_model()
    names = [f[len('step_f64_upd:'):] for f in gtt.files if f.startswith('step_f64_upd:')]
    P = dict(m.named_parameters())
    seeded = TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, seed=7, counter=(3, 0), step=False)
    g_seeded = {k: P[k].grad.detach().double().clone() for k in names}
    T = TD.draw_steps(7, 3, 0 | TD.STEP_STREAM, B, len(NOISE_SCHEDULE))
    Z = sampler.philox_normal(7, 3, 0, 0, -(-B * Ls // 4))[1][:B * Ls].view(B, Ls).contiguous()
    w0 = sampler_words(7, 3, TD.STEP_STREAM, 0, B).reshape(B, 4)[:, 0].astype(np.uint64)
    assert T.tolist() == ((w0 * np.uint64(50)) >> np.uint64(32)).tolist()
    supplied = TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, t=T, noise=Z, step=False)
    torch.cuda.synchronize()
    a, b = float(seeded), float(supplied)
    spread = abs(float(gtt['step_f32_loss'][0]) - float(gtt['step_f64_loss'][0]))
    worst = max(float((g_seeded[k] - P[k].grad.detach().double()).abs().max()) / float(P[k].grad.detach().double().abs().max())
                for k in names)
    print(f'seeded loss {a:.9f} supplied loss {b:.9f} |diff| {abs(a - b):.3e} bar {1e-5 * b + 3 * spread:.3e}; '
          f'largest relative gradient difference over {len(names)} tensors {worst:.3e}; T {T.tolist()}')
    assert math.isfinite(a) and abs(a - b) <= 1e-5 * b + 3 * spread, (a, b)
    # a second seeded call repeats the draw; another counter does not; the validation loss takes the same keywords
    again = TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, seed=7, counter=(3, 0), step=False)
    other = TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, seed=7, counter=(4, 0), step=False)
    assert abs(float(again) - a) <= 1e-6 * a and abs(float(other) - a) > 1e-4 * a
    with pytest.raises(_lib.SeHipError):
        TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, seed=7, t=T, step=False)
    with pytest.raises(_lib.SeHipError):
        TD.tsc_diffusion_step(m, opt, clean, noisy, NOISE_SCHEDULE, counter=(3, 0), step=False)
    m.eval()
    v_seeded = float(TD.tsc_diffusion_validation_loss(m, clean, noisy, NOISE_SCHEDULE, seed=7, counter=(3, 0)))
    v_supplied = float(TD.tsc_diffusion_validation_loss(m, clean, noisy, NOISE_SCHEDULE, t=T, noise=Z))
    assert abs(v_seeded - v_supplied) <= 1e-5 * v_supplied + 3 * spread, (v_seeded, v_supplied)


# ------------------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------------------
SIX_KEYS = {'epoch', 'arch', 'state_dict', 'optimizer', 'scaler', 'best_loss'}


def _losses(caplog):
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Train Loss:')]
    return [[float(v) for v in re.findall(r'Loss: (\S+)', l)] for l in lines]


def test_main_diffuse_round_trip(TD, tmp_path, caplog):
    from speech_enhancement_amd import inference_diffuse, main_diffuse
    out = str(tmp_path / 'out')
    caplog.set_level(logging.INFO)
    argv = ['--cfg', '/dev/null', '-a', 'tsc-diffuse', '-b', '2', '--epochs', '1', '--optimizer', 'adamw', '--lr', '5e-4',
            '--crop-len', '1', '--synthetic', '2', '--seed', '1', '--output', out]
    main_diffuse.main(argv)
    folder = os.path.join(out, 'tsc-diffuse', 'default')
    path = os.path.join(folder, 'checkpoint_0000.pth.tar')
    ck = torch.load(path, map_location='cpu')
    assert set(ck) == SIX_KEYS and ck['epoch'] == 1 and ck['arch'] == 'tsc-diffuse' and math.isfinite(ck['best_loss'])
    spec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tsc_state_spec.json')))
    assert sorted(ck['state_dict']) == sorted('module.' + e[0] for e in spec)
    assert all(tuple(ck['state_dict']['module.' + e[0]].shape) == tuple(e[1]) for e in spec)
    assert all(torch.isfinite(v).all() for v in ck['state_dict'].values() if v.is_floating_point())
    assert ck['scaler'] == torch.cuda.amp.GradScaler().state_dict() and ck['optimizer']['param_groups']
    losses = _losses(caplog)
    assert len(losses) == 1 and len(losses[0]) == 2 and all(math.isfinite(v) for v in losses[0]), losses
    assert any(r.getMessage() == 'start_epoch == 0' for r in caplog.records)
    assert len([r for r in caplog.records if r.getMessage().startswith('Train: [0/1]')]) == 1      # two iterations, print_freq 10
    # its own inference CLI loads the file
    a, c = inference_diffuse.parse_option(['-a', 'tsc-diffuse', '-o', out, '-m', path, '--cfg', '/dev/null'])
    model = inference_diffuse.load_model(path, a, c)
    assert not model.training and all(torch.equal(v.cpu(), ck['state_dict']['module.' + k]) for k, v in model.state_dict().items())
    # --resume runs epoch 1 and nothing else
    caplog.clear()
    argv[argv.index('--epochs') + 1] = '2'
    main_diffuse.main(argv + ['--resume', path])
    assert any(r.getMessage() == 'start_epoch == 1' for r in caplog.records)
    assert [r.getMessage() for r in caplog.records if r.getMessage().startswith('Train: [')][0].startswith('Train: [1/2][0/2]')
    losses = _losses(caplog)
    assert len(losses) == 1 and all(math.isfinite(v) for v in losses[0]), losses
    ck1 = torch.load(os.path.join(folder, 'checkpoint_0001.pth.tar'), map_location='cpu')
    assert set(ck1) == SIX_KEYS and ck1['epoch'] == 2 and ck1['best_loss'] <= ck['best_loss']
    assert not os.path.exists(os.path.join(folder, 'checkpoint_0002.pth.tar'))


def _write_wav(path, x, sr=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(np.round(x * 20000).clip(-32768, 32767), dtype='<i2').tobytes())


def test_main_diffuse_trains_from_wav_folders_with_a_noise_folder(TD, tmp_path, caplog):
    from speech_enhancement_amd import main_diffuse
    rs = np.random.RandomState(3)
    dirs = {k: tmp_path / k for k in ('train_clean', 'train_noisy', 'test_clean', 'test_noisy', 'noise')}
    for d in dirs.values():
        os.makedirs(d)
    tone = lambda n: 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 16000 + 6 * rs.rand()) * (0.6 + 0.4 * np.sin(np.arange(n) / 900.0))
    for split, lengths in (('train', (30000, 18000, 26000, 20000)), ('test', (22000, 17000))):
        for k, n in enumerate(lengths):
            x = tone(n) + 0.01 * rs.randn(n)
            _write_wav(dirs[split + '_clean'] / f's{k}.wav', x)
            _write_wav(dirs[split + '_noisy'] / f's{k}.wav', x + 0.08 * rs.randn(n))
    for k, n in enumerate((21000, 9000)):
        _write_wav(dirs['noise'] / f'n{k}.wav', 0.15 * rs.randn(n))
    out = str(tmp_path / 'out')
    caplog.set_level(logging.INFO)
    main_diffuse.main(['--cfg', '/dev/null', '-a', 'tsc-diffuse', '-b', '2', '--epochs', '1', '--optimizer', 'adamw', '--lr', '5e-4',
                       '--crop-len', '1', '--seed', '1', '--output', out, '--gpu', '0', '-p', '1', '--noise-dir', str(dirs['noise']),
                       '--noise-snr', '0', '15', '--opts', 'DATA.TRAIN_CLEAN_DIR', str(dirs['train_clean']), 'DATA.TRAIN_NOISY_DIR',
                       str(dirs['train_noisy']), 'DATA.TEST_CLEAN_DIR', str(dirs['test_clean']), 'DATA.TEST_NOISY_DIR',
                       str(dirs['test_noisy'])])
    losses = _losses(caplog)
    assert len(losses) == 1 and len(losses[0]) == 2 and all(math.isfinite(v) for v in losses[0]), losses
    assert len([r for r in caplog.records if r.getMessage().startswith('Train: [0/1]')]) == 2      # 4 files, batches of 2
    tests = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Test: [')]
    assert tests and all(math.isfinite(float(re.search(r'Loss (\S+)', l).group(1))) for l in tests)
    ck = torch.load(os.path.join(out, 'tsc-diffuse', 'default', 'checkpoint_0000.pth.tar'), map_location='cpu')
    assert set(ck) == SIX_KEYS and all(torch.isfinite(v).all() for v in ck['state_dict'].values() if v.is_floating_point())
    with pytest.raises(RuntimeError, match='--noise-dir'):
        main_diffuse.main(['--cfg', '/dev/null', '-a', 'tsc-diffuse', '--synthetic', '2', '--noise-dir', str(dirs['noise'])])
