"""The graph-replayed TSC-diffusion sampler on the GPU (csrc/se_sampler.hip, sampler.py, inference_diffuse.py): the in-kernel
Philox4x32-10 / Box-Muller generator against the numpy one of test_sampler_host.py, the fused update against its formula in fp64,
the step bookkeeping, and the sampler against the reference's predict_tsc vectors."""
import os
import types

import numpy as np
import pytest
import torch

import formula
from test_sampler_host import FAST, KAT, NOISE_SCHEDULE, box_muller, sampler_words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = types.SimpleNamespace(NOISE_SCHEDULE=NOISE_SCHEDULE, INFERENCE_NOISE_SCHEDULE=FAST, N_FFT=400, HOP_SAMPLES=100, SAMPLE_RATE=16000)
ARGS = types.SimpleNamespace(comp_type='pow')
# seed of the moment test: the fp64 numpy normals of its words pass every bar of that test (checked on the CPU when the test was
# written; the test checks it again before it looks at the kernel's)
MOMENT_SEED = 20240607


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope='module')
def SM():
    from speech_enhancement_amd import sampler
    return sampler


@pytest.fixture(scope='module')
def model():
    import speech_enhancement_amd as S
    m = S.TSCNetDiffusion(64, 201, NOISE_SCHEDULE)
    m.load_state_dict(formula.tsc_state())
    return m.cuda().eval()


@pytest.fixture(scope='module')
def gt():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_tsc.npz'))


# ---- 1. words --------------------------------------------------------------------------------------------------------
def test_words_equal_numpy_philox_bit_for_bit(SM):
    for seed in (0, 0x9E3779B97F4A7C15):
        w, _ = SM.philox_normal(seed, 3, 1, 0, 1024, words=True, normals=False)
        assert np.array_equal(u32(w), sampler_words(seed, 3, 1, 0, 1024)), hex(seed)
    w, _ = SM.philox_normal(0, 0, 0, 0, 1, words=True, normals=False)
    assert u32(w).tolist() == list(KAT[0][2])
    w, _ = SM.philox_normal(2 ** 64 - 1, 0xffffffff, 0xffffffff, 2 ** 64 - 1, 1, words=True, normals=False)
    assert u32(w).tolist() == list(KAT[1][2])
    ctr, key, out = KAT[2]
    w, _ = SM.philox_normal((key[1] << 32) | key[0], ctr[2], ctr[3], (ctr[1] << 32) | ctr[0], 1, words=True, normals=False)
    assert u32(w).tolist() == list(out)


# ---- 2. normals ------------------------------------------------------------------------------------------------------
def test_normals_against_box_muller_in_fp64(SM):
    w, z = SM.philox_normal(5, 2, 0, 0, 2 ** 14, words=True, normals=True)
    words = u32(w)
    assert np.array_equal(words, sampler_words(5, 2, 0, 0, 2 ** 14))
    z64 = box_muller(words, np.float64)
    floor = float(np.abs(box_muller(words, np.float32).astype(np.float64) - z64).max())
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - z64).max())
    print(f'box-muller over {z64.size} draws: kernel max error {err:.3e}, fp32 numpy max error {floor:.3e}')
    assert np.all(np.isfinite(z.cpu().numpy()))
    assert err < 2 * floor


# ---- 3. moments ------------------------------------------------------------------------------------------------------
def _moments(z, z_n4, z_run1):
    z = np.asarray(z, np.float64)
    N = z.size
    m, v = z.mean(), z.var()
    c = z - m
    corr = lambda a, b: float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
    return {'mean': (abs(m), 5 / np.sqrt(N)), 'var': (abs(v - 1), 5 * np.sqrt(2 / N)),
            'kurtosis': (abs(np.mean(c ** 4) / v ** 2 - 3), 5 * np.sqrt(24 / N)),
            'lag1': (abs(corr(z[:-1], z[1:])), 5 / np.sqrt(N)),
            'n3_n4': (abs(corr(z, np.asarray(z_n4, np.float64))), 5 / np.sqrt(N)),
            'run0_run1': (abs(corr(z, np.asarray(z_run1, np.float64))), 5 / np.sqrt(N))}


def test_moments_of_a_million_draws(SM):
    G = 2 ** 18                                          # 2^20 draws
    sets = [(3, 0), (4, 0), (3, 1)]                      # (n, run): the base, the next step, the next utterance
    ref = [box_muller(sampler_words(MOMENT_SEED, n, run, 0, G), np.float64) for n, run in sets]
    for name, (val, bar) in _moments(*ref).items():
        assert val < bar, ('the seed fails in fp64 numpy: pick another', name, val, bar)
    got = [SM.philox_normal(MOMENT_SEED, n, run, 0, G)[1].cpu().numpy() for n, run in sets]
    for name, (val, bar) in _moments(*got).items():
        print(f'{name}: {val:.3e} (bar {bar:.3e})')
        assert val < bar, (name, val, bar)


# ---- 4. geometry -----------------------------------------------------------------------------------------------------
def test_draws_do_not_depend_on_the_launch_geometry(SM):
    _, big = SM.philox_normal(9, 1, 2, 0, 25000)        # 100 000 elements
    _, small = SM.philox_normal(9, 1, 2, 0, 250)         # 1000 elements
    assert np.array_equal(big.cpu().numpy()[:1000].view(np.uint32), small.cpu().numpy().view(np.uint32))
    # and inside the update: the draws of a [1, 1000] and of a [1, 100000] tensor agree on the first 1000 elements
    coef = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], device='cuda')
    n, run = torch.ones(1, device='cuda', dtype=torch.int32), torch.full((1,), 2, device='cuda', dtype=torch.int32)
    seed = torch.full((1,), 9, device='cuda', dtype=torch.int64)
    outs = []
    for Ls in (100000, 1000):
        a = torch.zeros(1, Ls, device='cuda')
        SM.sampler_update(a, torch.zeros_like(a), torch.zeros_like(a), coef, n, seed=seed, run=run)
        outs.append(a.cpu().numpy())
    assert np.array_equal(outs[0][0, :1000].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[1][0].view(np.uint32), small.cpu().numpy().view(np.uint32))       # audio = 0 + 1 * z exactly


# ---- 5. the update with supplied noise against the formula in fp64 ----------------------------------------------------
SHAPES = [(1, 1), (2, 63), (2, 64), (3, 257), (2, 1027)]
GAMMA = 0.2


def _coef():
    import speech_enhancement_amd as S
    from speech_enhancement_amd import sampler
    sched = S.inference_schedule(CFG, fast_sampling=True)
    return sampler.pack_coef(sched[5], sched[6], sched[7], sched[9])


def _reference_update(a, y, e, z, coef, n, clamp, c):
    """(result, elementwise bar) in fp64 from the fp32 inputs and the fp32 coefficient table.  The bar is 8 * 2^-24 times the sum of
    the magnitudes of the terms that are added (at most seven roundings of half an ulp each, every one relative to a partial result
    no larger than that sum): for n > 0 the four terms of the update; for n == 0, where c2 = sigma = 0 and the terms are others,
    (1 - gamma) c1 a, (1 - gamma) c3 e and gamma y; times 1 / c where the de-normalisation applies."""
    a, y, e = a.astype(np.float64), y.astype(np.float64), e.astype(np.float64)
    c1, c2, c3, sg = (float(v) for v in coef[n])
    if n > 0:
        out = c1 * a + c2 * y - c3 * e + sg * z.astype(np.float64)
        mag = np.abs(c1 * a) + np.abs(c2 * y) + np.abs(c3 * e) + np.abs(sg * z)
    else:
        g = float(np.float32(GAMMA))
        out = (1 - g) * (c1 * a - c3 * e) + g * y
        mag = (1 - g) * (np.abs(c1 * a) + np.abs(c3 * e)) + np.abs(g * y)
        if clamp:
            out = np.clip(out, -1.0, 1.0)
        if c is not None:
            out = out / c.astype(np.float64)[:, None]
            mag = mag / c.astype(np.float64)[:, None]
    return out, 8 * 2.0 ** -24 * mag


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('B,Ls', SHAPES)
def test_update_with_supplied_noise_against_fp64(SM, B, Ls, offset):
    coef = _coef()
    steps = coef.shape[0]
    rs = np.random.RandomState(100 * B + Ls)
    a0, y0, e0 = (rs.randn(B, Ls).astype(np.float32) * s for s in (1.2, 1.0, 0.7))     # |a| > 1 on many elements: the clamp acts
    noise = rs.randn(steps - 1, B, Ls).astype(np.float32)
    c = (0.5 + rs.rand(B)).astype(np.float32)

    def dev(x):                                           # offset 1: every buffer starts 4 bytes off a 16-byte boundary
        buf = torch.empty(x.size + offset, device='cuda', dtype=torch.float32)
        v = buf[offset:].view(x.shape)
        v.copy_(torch.from_numpy(x))
        return v
    coef_d, noise_d, c_d = torch.from_numpy(coef).cuda(), dev(noise), torch.from_numpy(c).cuda()
    clamped = 0
    cases = [(5, False, False), (3, False, False), (1, False, False)] + [(0, cl, ci) for cl in (False, True) for ci in (False, True)]
    for n, clamp, use_c in cases:
        a, y, e = dev(a0), dev(y0), dev(e0)
        nd = torch.full((1,), n, device='cuda', dtype=torch.int32)
        SM.sampler_update(a, y, e, coef_d, nd, noise=noise_d, c_inv=c_d if use_c else None, gamma=GAMMA, clamp=clamp)
        z = noise[steps - 1 - n] if n > 0 else None
        want, bar = _reference_update(a0, y0, e0, z, coef, n, clamp, c if use_c else None)
        got = a.cpu().numpy().astype(np.float64)
        worst = float(np.max(np.abs(got - want) / np.maximum(bar, 1e-300)))
        print(f'[{B}, {Ls}] n={n} clamp={clamp} c_inv={use_c}: worst error / bar = {worst:.3f}')
        assert np.all(np.abs(got - want) <= bar), (n, clamp, use_c, worst)
        assert int(nd.item()) == n                                                  # the launch only reads n
        assert np.array_equal(y.cpu().numpy(), y0) and np.array_equal(e.cpu().numpy(), e0)
        if n == 0 and clamp and not use_c:
            clamped += int(np.sum(np.abs(got) == 1.0))
    if B * Ls >= 64:
        assert clamped > 0
    # a step outside the table writes nothing
    a = dev(a0)
    SM.sampler_update(a, dev(y0), dev(e0), coef_d, torch.full((1,), steps, device='cuda', dtype=torch.int32), noise=noise_d)
    assert np.array_equal(a.cpu().numpy(), a0)


def test_update_draws_are_the_generator_at_counter_n_run(SM):
    """noise = NULL: z of element i is draw i of se_philox_normal(seed, n, run)"""
    coef = _coef()
    B, Ls, n, run, seed = 3, 257, 4, 6, 0x123456789ABCDEF
    rs = np.random.RandomState(3)
    a0, y0, e0 = (rs.randn(B, Ls).astype(np.float32) for _ in range(3))
    a = torch.from_numpy(a0).cuda()
    SM.sampler_update(a, torch.from_numpy(y0).cuda(), torch.from_numpy(e0).cuda(), torch.from_numpy(coef).cuda(),
                      torch.full((1,), n, device='cuda', dtype=torch.int32), seed=torch.full((1,), seed, device='cuda', dtype=torch.int64),
                      run=torch.full((1,), run, device='cuda', dtype=torch.int32))
    groups = (B * Ls + 3) // 4
    z = SM.philox_normal(seed, n, run, 0, groups)[1].cpu().numpy()[:B * Ls].reshape(B, Ls)
    want, bar = _reference_update(a0, y0, e0, z, coef, n, False, None)
    assert np.all(np.abs(a.cpu().numpy().astype(np.float64) - want) <= bar)


# ---- 6. advance ------------------------------------------------------------------------------------------------------
def test_advance_walks_the_steps_and_counts_the_utterance(SM):
    steps = 6
    coef = torch.from_numpy(_coef()).cuda()
    emb = torch.randn(steps, 64, device='cuda')
    d = torch.zeros(1, 64, device='cuda')
    n = torch.full((1,), steps - 1, device='cuda', dtype=torch.int32)
    run = torch.full((1,), 7, device='cuda', dtype=torch.int32)
    seed = torch.zeros(1, device='cuda', dtype=torch.int64)
    a, y, e = (torch.randn(2, 63, device='cuda') for _ in range(3))
    seen = []
    for _ in range(steps):
        SM.sampler_update(a, y, e, coef, n, seed=seed, run=run)
        SM.sampler_advance(n, run, emb, d)
        k = int(n.item())
        seen.append(k)
        assert torch.equal(d[0], emb[k])
    assert seen == [4, 3, 2, 1, 0, 5]
    assert int(n.item()) == steps - 1 and int(run.item()) == 8
    assert bool(torch.isfinite(a).all())


# ---- 7. the sampler against the reference ------------------------------------------------------------------------------
def test_graphed_sampler_vs_reference_predict_tsc(model, gt):
    import speech_enhancement_amd as S
    smp = S.GraphedTSCSampler(model, ARGS, CFG, fast=True)
    assert smp.steps == 6
    y = smp(gt['predict_in'], noises=gt['predict_noise'])
    assert y.shape == gt['predict_out'].shape
    sc = float(np.abs(gt['predict_out']).max())
    rms = lambda a, b: float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
    eager = S.predict_tsc(model, ARGS, CFG, gt['predict_in'], *S.inference_schedule(CFG, fast_sampling=True), noises=gt['predict_noise'])
    print(f'graphed sampler vs reference: rms {rms(y, gt["predict_out"]) / sc:.3e} of the maximum; '
          f'vs eager predict_tsc: {rms(y, eager) / sc:.3e}; eager vs reference: {rms(eager, gt["predict_out"]) / sc:.3e}')
    assert rms(y, gt['predict_out']) < 3e-4 * sc
    assert int(smp.n.item()) == smp.steps - 1 and int(smp.run.item()) == 1


# ---- 8. re-entrancy ----------------------------------------------------------------------------------------------------
def test_bucket_reuse_is_bitwise_reproducible(model):
    import speech_enhancement_amd as S
    frames, hop = 16, 100
    rs = np.random.RandomState(8)
    A = (0.1 * rs.randn(frames * hop - 37)).astype(np.float32)          # the wrap-pad repeats the first 37 samples
    Bc = (0.2 * rs.randn(frames * hop - 5)).astype(np.float32)           # another length, the same frame bucket
    nzA, nzB = (rs.randn(5, 1, frames * hop).astype(np.float32) for _ in range(2))
    smp = S.GraphedTSCSampler(model, ARGS, CFG, fast=True)
    yA1 = smp(A, noises=nzA)
    yB = smp(Bc, noises=nzB)
    yA2 = smp(A, noises=nzA)
    assert len(smp.buckets) == 1 and yA1.shape == A.shape and yB.shape == Bc.shape
    assert np.all(np.isfinite(yA1)) and np.all(np.isfinite(yB)) and not np.array_equal(yA1, yB[:A.size])
    assert np.array_equal(yA1.view(np.uint32), yA2.view(np.uint32))
    fresh = S.GraphedTSCSampler(model, ARGS, CFG, fast=True)(A, noises=nzA)
    assert np.array_equal(yA1.view(np.uint32), fresh.view(np.uint32))
    # the wrap-pad and the clip scale are predict_tsc's: the eager path on the same inputs is as close as in test 7
    eager = S.predict_tsc(model, ARGS, CFG, A, *S.inference_schedule(CFG, fast_sampling=True), noises=nzA)
    assert float(np.sqrt(np.mean((yA1.astype(np.float64) - eager) ** 2))) < 3e-4 * float(np.abs(eager).max())


# ---- 9. seeds ----------------------------------------------------------------------------------------------------------
def test_in_kernel_noise_is_reproducible_per_seed(model):
    import speech_enhancement_amd as S
    x = (0.1 * np.random.RandomState(9).randn(1600 - 37)).astype(np.float32)
    s1 = S.GraphedTSCSampler(model, ARGS, CFG, fast=True, seed=123)
    s2 = S.GraphedTSCSampler(model, ARGS, CFG, fast=True, seed=123)
    y1, y2 = s1(x), s2(x)
    assert np.all(np.isfinite(y1)) and np.array_equal(y1.view(np.uint32), y2.view(np.uint32))
    y1b = s1(x)                                           # the second utterance: run advanced
    assert int(s1.run.item()) == 2 and not np.array_equal(y1, y1b)
    s2.set_seed(124)
    y3 = s2(x)
    assert not np.array_equal(y1, y3)
    s2.set_seed(123)                                      # the seed names the sequence: back to its first utterance
    assert np.array_equal(s2(x).view(np.uint32), y1.view(np.uint32))


# ---- 10. command line ----------------------------------------------------------------------------------------------------
def test_inference_diffuse_cli(tmp_path, capsys):
    from scipy.io import wavfile
    import speech_enhancement_amd as S
    from speech_enhancement_amd import inference_diffuse as ID
    noisy_dir, clean_dir, out_dir = tmp_path / 'noisy', tmp_path / 'clean', tmp_path / 'out'
    noisy_dir.mkdir()
    clean_dir.mkdir()
    rs = np.random.RandomState(10)
    lengths = {'p1_001.wav': 8000, 'p1_002.wav': 7963}
    for name, Ls in lengths.items():
        t = np.arange(Ls) / 16000.0
        clean = 0.3 * np.sin(2 * np.pi * 440 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 5 * t)) + 0.02 * rs.randn(Ls)
        noisy = clean + 0.05 * rs.randn(Ls)
        wavfile.write(str(clean_dir / name), 16000, np.round(clean * 32767).astype(np.int16))
        wavfile.write(str(noisy_dir / name), 16000, np.round(noisy * 32767).astype(np.int16))
    cfg = tmp_path / 'cfg.yaml'
    cfg.write_text(f'DATA:\n  TEST_NOISY_DIR: {noisy_dir}\n  TEST_CLEAN_DIR: {clean_dir}\n')
    torch.manual_seed(0)
    m = S.TSCNetDiffusion(64, 201, NOISE_SCHEDULE)
    ckpt = tmp_path / 'checkpoint_0000.pth.tar'
    torch.save({'epoch': 0, 'state_dict': {'module.' + k: v for k, v in m.state_dict().items()}}, str(ckpt))
    ID.main(['-a', 'tsc', '--fast', '--save', '--output', str(out_dir), '--model_path', str(ckpt), '--cfg', str(cfg), '--seed', '3'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('pesq:')]
    assert len(line) == 1
    vals = dict(f.strip().split(': ') for f in line[0].split('\t'))
    assert list(vals) == ['pesq', 'csig', 'cbak', 'covl', 'ssnr', 'stoi']
    assert np.isfinite(float(vals['ssnr'])) and np.isfinite(float(vals['stoi']))
    for name, Ls in lengths.items():
        sr, y = wavfile.read(str(out_dir / name))
        assert sr == 16000 and y.shape == (Ls,) and np.all(np.isfinite(y))
