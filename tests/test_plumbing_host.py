"""CPU-only tests of what the enhancers and the inference command lines share: the bucket cache (inference.LRU), the 'module.' prefix
strip (utils.strip_module_prefix) and the loop of the two command lines (inference_gan.run_cli) with everything behind it stubbed."""
import os
import re
import types
from collections import OrderedDict

import numpy as np
import pytest


def test_lru_builds_once_and_drops_the_least_recently_used():
    from speech_enhancement_amd.inference import LRU
    built = []

    def build(key):
        return lambda: built.append(key) or {'key': key}
    c = LRU()
    assert isinstance(c, OrderedDict) and len(c) == 0
    a = c.lookup('a', build('a'), 2)
    b = c.lookup('b', build('b'), 2)
    assert a == {'key': 'a'} and list(c) == ['a', 'b'] and built == ['a', 'b']
    assert c.lookup('b', build('b'), 2) is b and built == ['a', 'b'] and list(c) == ['a', 'b']       # a hit on the last key
    assert c.lookup('a', build('a'), 2) is a and built == ['a', 'b'] and list(c) == ['b', 'a']       # a hit moves its key to the end
    c.lookup('c', build('c'), 2)                                # 'b' leaves: the least recently used, not 'a', the oldest inserted
    assert list(c) == ['a', 'c'] and built == ['a', 'b', 'c'] and c['a'] is a and 'b' not in c
    assert c.lookup('b', build('b'), 2) is not b and built == ['a', 'b', 'c', 'b'] and list(c.keys()) == ['c', 'b']
    # the keys the two enhancers use: frame counts and (frames, supplied noise)
    c.lookup((16, False), build(3), 3)
    assert sorted(c, key=str) == [(16, False), 'b', 'c'] and len(c) == 3 and list(c.items())[-1] == ((16, False), {'key': 3})
    c.clear()
    assert len(c) == 0 and c.lookup(49, build(49), 1) == {'key': 49} and sorted(c) == [49]


def test_strip_module_prefix():
    from speech_enhancement_amd.utils import strip_module_prefix
    sd = OrderedDict([('module.a.weight', 1), ('b.module.bias', 2), ('module.module.x', 3), ('modules.y', 4), ('module.', 5)])
    out = strip_module_prefix(sd)
    assert list(out.items()) == [('a.weight', 1), ('b.module.bias', 2), ('module.x', 3), ('modules.y', 4), ('', 5)]
    for k, s in zip(sd, out):
        assert len(k) - len(s) == (7 if k.startswith('module.') else 0)
    assert list(sd) == ['module.a.weight', 'b.module.bias', 'module.module.x', 'modules.y', 'module.']       # the input is left alone


PESQ_OF = {3: 2.1, 4: 2.9, 5: 2.4}


@pytest.fixture
def cli(tmp_path, monkeypatch):
    """run_cli's surroundings, none of which touches the GPU: two wav names in a noisy and a clean folder, a `build` that returns
    the epoch of the checkpoint name as the model, metrics.evaluate replaced by fixed sums per epoch"""
    import torch
    from speech_enhancement_amd import inference_gan as IG
    monkeypatch.setattr(torch.cuda, 'init', lambda *a, **k: pytest.fail('the GPU was initialised'))
    noisy, clean = tmp_path / 'noisy', tmp_path / 'clean'
    for d in (noisy, clean):
        d.mkdir()
        for name in ('a.wav', 'b.wav'):
            (d / name).write_bytes(b'')
    seen = types.SimpleNamespace(built=[], scored=[], enhanced=[], noisy=noisy, clean=clean)

    def build(model_path):
        seen.built.append(os.path.basename(model_path))
        m = re.search(r'checkpoint_(\d{4})', model_path)
        return (int(m.group(1)) if m else 4), 'the enhancer'

    def evaluate(model, config, pairs, on_enhanced=None, enhancer=None):
        seen.scored.append((model, enhancer, on_enhanced))
        return np.array([PESQ_OF[model], 3.0, 3.0, 3.0, 8.0, 0.9]) * 2           # sums over the two files

    def enhance(model, enhancer, x):
        seen.enhanced.append((model, enhancer, x))
        return x
    monkeypatch.setattr(IG.metrics, 'evaluate', evaluate)
    monkeypatch.setattr(IG, '_read', lambda path, config: os.path.basename(path))
    monkeypatch.setattr(IG, '_save', lambda *a: pytest.fail('saved without --save'))
    seen.config = types.SimpleNamespace(DATA=types.SimpleNamespace(TEST_NOISY_DIR=str(noisy), TEST_CLEAN_DIR=str(clean)), SAMPLE_RATE=16000)
    seen.args = types.SimpleNamespace(output=str(tmp_path / 'out'), model_path=str(tmp_path / 'ckpts'), save=False,
                                      validate_epochs=False, start=None, end=None)
    seen.run = lambda: IG.run_cli(seen.args, seen.config, build, enhance)
    return seen


def test_run_cli_validate_epochs(cli, capsys):
    cli.args.validate_epochs, cli.args.start, cli.args.end = True, 3, 6
    cli.run()
    assert capsys.readouterr().out.split('\n') == [
        'Epoch: 3', 'pesq: 2.100\t csig: 3.000\t cbak: 3.000\t covl: 3.000\t ssnr: 8.000\t stoi: 0.900',
        'Epoch: 4', 'pesq: 2.900\t csig: 3.000\t cbak: 3.000\t covl: 3.000\t ssnr: 8.000\t stoi: 0.900',
        'Epoch: 5', 'pesq: 2.400\t csig: 3.000\t cbak: 3.000\t covl: 3.000\t ssnr: 8.000\t stoi: 0.900',
        'Best epoch: 4\t best PESQ: 2.9', '']
    assert cli.built == ['checkpoint_0003.pth.tar', 'checkpoint_0004.pth.tar', 'checkpoint_0005.pth.tar']
    assert cli.scored == [(3, 'the enhancer', None), (4, 'the enhancer', None), (5, 'the enhancer', None)] and not cli.enhanced
    assert os.path.isdir(cli.args.output)


def test_run_cli_one_checkpoint(cli, capsys):
    cli.args.model_path = 'ck.pth.tar'
    cli.run()
    assert capsys.readouterr().out == 'pesq: 2.900\t csig: 3.000\t cbak: 3.000\t covl: 3.000\t ssnr: 8.000\t stoi: 0.900\n'
    assert cli.built == ['ck.pth.tar'] and len(cli.scored) == 1


def test_run_cli_without_clean_files_only_enhances(cli, capsys):
    for name in ('a.wav', 'b.wav'):
        os.remove(cli.clean / name)
    os.rmdir(cli.clean)
    cli.args.model_path = 'ck.pth.tar'
    cli.args.validate_epochs, cli.args.start, cli.args.end = True, 3, 6          # not looked at without clean files
    cli.run()
    assert capsys.readouterr().out == f'no clean signals under DATA.TEST_CLEAN_DIR ({cli.clean}): enhancing only, no metrics\n'
    assert cli.built == ['ck.pth.tar'] and not cli.scored
    assert cli.enhanced == [(4, 'the enhancer', 'a.wav'), (4, 'the enhancer', 'b.wav')]
