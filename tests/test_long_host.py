"""CPU-only tests of chunked enhancement of long recordings: the chunk plan (inference.chunk_plan), its refusals, the new
inference_gan flags and the C ABI of the two kernels."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = [(16, 4), (16, 5), (12, 4), (30, 10), (32, 8), (9, 3)]


@pytest.fixture(scope='module')
def I():
    from speech_enhancement_amd import inference
    return inference


@pytest.mark.parametrize('S,V', SWEEP)
def test_chunk_plan_properties(I, S, V):
    """every property the crossfade rule relies on, for every length from one sample more than a chunk to seven chunks (hop = 1)"""
    for L in range(S + 1, 7 * S + 1):
        s = I.chunk_plan(L, S, V, hop=1)
        K = len(s)
        assert K == max(2, -(-(L - V) // (S - V))), (L, s)
        assert s[0] == 0 and s[-1] == L - S, (L, s)                       # full of real audio, the last chunk ends at L
        strides = [b - a for a, b in zip(s, s[1:])]
        assert all(1 <= d <= S - V for d in strides), (L, s)              # ascending, neighbours overlap by at least V
        if K >= 3:
            assert all(d >= V for d in strides), (L, s)                   # a fade-in is over before the next chunk starts
        # every sample is covered, and inside a fade the previous chunk still reaches it
        for k in range(1, K):
            assert s[k - 1] + S >= s[k] + V


def test_chunk_plan_scales_with_the_hop(I):
    assert I.chunk_plan(4137, 1600, 400) == [0, 845, 1691, 2537]            # (k * 2537) // 3, K = ceil(3737 / 1200) = 4
    assert I.chunk_plan(1601, 1600, 400) == [0, 1]
    assert I.chunk_plan(2 * 1600 - 400, 1600, 400) == [0, 1200]
    assert I.chunk_plan(2 * 1600 - 400 + 1, 1600, 400) == [0, 600, 1201]
    n = 3600 * 16000
    s = I.chunk_plan(n, 64000, 8000)
    assert s[0] == 0 and s[-1] == n - 64000 and len(s) == -(-(n - 8000) // 56000)


def test_short_recordings_take_one_whole_forward(I):
    for L in (1, 201, 1599, 1600):
        assert I.chunk_plan(L, 1600, 400) == [0]
    assert I.chunk_plan(16, 16, 4, hop=1) == [0]


@pytest.mark.parametrize('S,V,hop', [(1650, 400, 100), (200, 50, 100), (100, 10, 100), (1600, 0, 100), (1600, -3, 100),
                                     (1600, 534, 100), (1600, 1600, 100), (2, 0, 1), (8, 3, 1)])
def test_chunk_plan_refuses_bad_sizes(I, S, V, hop):
    with pytest.raises(ValueError):
        I.chunk_plan(10 * S, S, V, hop=hop)


def test_chunk_plan_edge_sizes_pass(I):
    assert I.chunk_plan(2000, 300, 100) == I.chunk_plan(2000, 300, 100, hop=100)          # S = 3 V and S = 3 hops are legal
    assert len(I.chunk_plan(2000, 300, 100)) == -(-1900 // 200)
    with pytest.raises(ValueError):
        I.chunk_plan(0, 1600, 400)


def _argv(tmp_path):
    cfg = tmp_path / 'c.yaml'
    cfg.write_text('DATA:\n  TEST_NOISY_DIR: n\n  TEST_CLEAN_DIR: c\n')
    return ['-o', 'out', '-m', 'ck.pth.tar', '--cfg', str(cfg)]


def test_cli_flags_parse_and_default_to_whole_utterances(tmp_path):
    from speech_enhancement_amd import inference_gan as IG
    base, _ = IG.parse_option(_argv(tmp_path))
    assert (base.chunk_len, base.chunk_overlap, base.chunk_batch) == (0.0, 0.5, 8)
    assert IG.long_enhancer(base, None, None, None) is None                             # nothing is built, the model is not touched
    zero, _ = IG.parse_option(_argv(tmp_path) + ['--chunk-len', '0'])
    assert vars(zero) == vars(base)
    a, _ = IG.parse_option(_argv(tmp_path) + ['--chunk-len', '4', '--chunk-overlap', '0.25', '--chunk-batch', '3', '--save'])
    assert (a.chunk_len, a.chunk_overlap, a.chunk_batch, a.save) == (4.0, 0.25, 3, True)
    rest = {k: v for k, v in vars(a).items() if not k.startswith('chunk_') and k != 'save'}
    assert rest == {k: v for k, v in vars(base).items() if not k.startswith('chunk_') and k != 'save'}
    # an overlap that would be refused with chunking on is not looked at with chunking off
    off, _ = IG.parse_option(_argv(tmp_path) + ['--chunk-overlap', '9'])
    assert off.chunk_len == 0.0


@pytest.mark.parametrize('extra', [['--chunk-len', '-1'], ['--chunk-len', '4', '--chunk-overlap', '2'],
                                   ['--chunk-len', '4', '--chunk-overlap', '0'], ['--chunk-len', '0.01'],
                                   ['--chunk-len', '4.001'], ['--chunk-len', '4', '--chunk-batch', '0']])
def test_cli_refuses_bad_combinations_before_any_gpu_work(tmp_path, monkeypatch, extra):
    import torch
    from speech_enhancement_amd import inference_gan as IG
    monkeypatch.setattr(IG, 'load_model', lambda *a, **k: pytest.fail('the model was loaded'))
    monkeypatch.setattr(torch.cuda, 'init', lambda *a, **k: pytest.fail('the GPU was initialised'))
    with pytest.raises(ValueError):
        IG.main(_argv(tmp_path) + extra)


def test_long_enhancer_refuses_a_training_model_and_bad_sizes(I):
    import types
    cfg = types.SimpleNamespace(N_FFT=400, HOP_SAMPLES=100)
    with pytest.raises(RuntimeError, match='eval'):
        I.LongEnhancer(types.SimpleNamespace(training=True), cfg, 0.1, 0.025)
    ok = types.SimpleNamespace(training=False)
    e = I.LongEnhancer(ok, cfg)
    assert (e.S, e.V, e.batch) == (64000, 8000, 8)
    assert (I.LongEnhancer(ok, cfg, 0.1, 0.025, batch=3).S, I.LongEnhancer(ok, cfg, 0.1, 0.025).V) == (1600, 400)
    for kw in ({'chunk_seconds': 0.1, 'overlap_seconds': 0.05}, {'chunk_seconds': 0.1031}, {'batch': 0}):
        with pytest.raises(ValueError):
            I.LongEnhancer(ok, cfg, **kw)
    ok.training = True                                   # switched back to training after construction: refused at the call
    with pytest.raises(RuntimeError, match='eval'):
        e.enhance_device([0.0] * 10)


def test_abi_declares_and_exports_the_chunk_kernels():
    import ctypes
    hdr = open(os.path.join(ROOT, 'include', 'se_hip.h')).read()
    lib = ctypes.CDLL(os.path.join(ROOT, 'speech-enhancement_amd', 'libse_hip.so'))
    for name in ('se_chunk_gather', 'se_chunk_assemble'):
        assert re.search(r'\bint ' + name + r'\s*\(', hdr), name
        assert hasattr(lib, name), name


def test_chunk_wrappers_have_no_cpu_fallback():
    import torch
    from speech_enhancement_amd import _lib, ops
    with pytest.raises(_lib.SeHipError):
        ops.chunk_gather(torch.zeros(4000), torch.tensor([0, 2400]), 1600)
    with pytest.raises(_lib.SeHipError):
        ops.chunk_assemble(torch.zeros(2, 1600), torch.ones(2), torch.zeros(2, dtype=torch.uint8), torch.tensor([0, 2400]), 400, 4000)
