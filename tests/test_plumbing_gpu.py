"""inference.capture on the GPU without a model behind it: a step that counts its own runs shows what the sequence runs, undoes and
records.  The call inside `torch.cuda.graph` is recorded, not run (tests/test_stream_model_gpu.py relies on the same: a captured
stream has received nothing), so the counts below are those of the two warm-up runs, the restore and the replays."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def counting_step():
    acc, out = torch.zeros(4, device='cuda'), torch.zeros(4, device='cuda')

    def step():
        acc.add_(1)
        out.copy_(acc * 2)
        return out
    return acc, out, step


@pytest.mark.parametrize('device', [torch.device('cuda'), torch.device('cuda', 0)], ids=['current', 'cuda0'])
def test_capture_restores_once_and_replays_one_step(device):
    from speech_enhancement_amd.inference import capture
    acc, out, step = counting_step()
    restored = []

    def restore():
        acc.zero_()
        restored.append(acc.data_ptr())
    graph, got = capture(step, device, restore)
    print('after capture: restores', len(restored), 'acc', acc.tolist(), 'out', out.tolist())
    assert len(restored) == 1                            # once, between the warm-up and the capture
    assert acc.tolist() == [0.0] * 4                     # the two warm-up runs were undone, the captured call has not run
    assert out.tolist() == [4.0] * 4                     # what the second warm-up run left: restore does not know `out`
    assert got is out and got.data_ptr() == out.data_ptr()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    print('after three replays: acc', acc.tolist(), 'out', out.tolist())
    assert acc.tolist() == [3.0] * 4 and out.tolist() == [6.0] * 4
    assert len(restored) == 1                            # a replay does not call back into Python


def test_capture_without_restore_keeps_the_warm_up():
    from speech_enhancement_amd.inference import capture
    acc, out, step = counting_step()
    graph, got = capture(step, torch.device('cuda', 0))
    print('after capture: acc', acc.tolist(), 'out', out.tolist())
    assert acc.tolist() == [2.0] * 4 and got is out      # the two warm-up runs
    graph.replay()
    torch.cuda.synchronize()
    assert acc.tolist() == [3.0] * 4 and out.tolist() == [6.0] * 4
    assert torch.is_grad_enabled()                       # no_grad covered the sequence only
