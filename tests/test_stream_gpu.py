"""GPU tests of the two streaming kernels (csrc/se_stream.hip) alone, no model, against their definition in include/se_hip.h restated
in numpy / fp64 here.

Small shapes, B = 3 rows: (W, H) = (1200, 400): H divides W; (1200, 208): it does not, so blocks straddle the ring's end;
(1300, 52): less than one wave's worth of quads per row trip.  Every run takes ceil(2 W / H) + 1 steps, so the ring wraps twice.
The elementwise bar of the emit kernel, 8 * 2^-24 * (|e| + |tail|) + 1e-12, is the one tests/test_long_gpu.py holds
se_chunk_assemble to: the handful of fp32 roundings is the same (a division, the weight, its complement, two products, a sum)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 8 * 2.0 ** -24
B_ = 3
WINDOWS = [(1200, 400), (1200, 208), (1300, 52)]
FADES = {(1200, 400): (200, 100), (1200, 208): (100, 8), (1300, 52): (48, 52)}          # (A, V) of the identity test
EMITS = [(1200, 400, 200, 100), (1200, 200, 0, 1), (1200, 400, 400, 400), (1300, 52, 48, 52)]


@pytest.fixture(scope='module')
def O():
    from speech_enhancement_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def steps_of(W, H):
    return -(-2 * W // H) + 1


def noise(seed, W, H, steps=None):
    return (0.1 * np.random.RandomState(seed).randn(steps or steps_of(W, H), B_, H)).astype(np.float32)


def windows64(blocks, W):
    """the definition: after step k the window of a row is the last W samples of its history, zeros on the left -> (windows
    [steps, B, W] fp32, c [steps, B] fp64 (1 where silent), silent [steps, B])"""
    steps, B, H = blocks.shape
    hist = np.concatenate([np.zeros((B, W), np.float32), blocks.transpose(1, 0, 2).reshape(B, steps * H)], axis=1)
    win = np.stack([hist[:, (k + 1) * H:(k + 1) * H + W] for k in range(steps)])
    P = np.sum(win.astype(np.float64) ** 2, axis=-1)
    r = np.minimum((np.arange(steps) + 1) * H, W)[:, None]
    silent = P == 0
    return win, np.where(silent, 1.0, np.sqrt(r / np.where(silent, 1.0, P))), silent


def run_window(O, blocks, W, reset=None):
    """the kernel over all steps; pos is advanced here (the emit kernel's job).  reset = (step, row): that row's counter and ring
    row are zeroed before the step -> (windows, c, silent) as numpy, stacked over the steps"""
    steps, B, H = blocks.shape
    ring, pos = torch.zeros(B, W, device='cuda'), torch.zeros(B, dtype=torch.int64, device='cuda')
    d = dev(blocks)
    got = []
    for k in range(steps):
        if reset is not None and reset[0] == k:
            pos[reset[1]] = 0
            ring[reset[1]] = 0
        before = pos.clone()
        got.append(O.stream_window(d[k], ring, pos))
        assert torch.equal(pos, before)                       # the window kernel leaves the counter alone
        pos += H
    return [torch.stack([g[i] for g in got]).cpu().numpy() for i in range(3)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_c(c, c64, silent):
    rel = np.abs(c.astype(np.float64) - c64) / c64
    print('c relative error', rel.max())
    assert rel.max() <= 1e-6 and (c[silent] == 1.0).all()


@pytest.mark.parametrize('W,H', WINDOWS)
def test_window_is_the_sliding_window_bit_for_bit(O, W, H):
    blocks = noise(1, W, H)
    steps = blocks.shape[0]
    assert steps * H > 2 * W and (W % H == 0 or any(((k * H) % W) + H > W for k in range(steps)))
    win, c, silent = run_window(O, blocks, W)
    want, c64, quiet = windows64(blocks, W)
    fill = -(-W // H)                                         # steps whose window still has zeros on the left (the last of them has
    assert not want[:fill - 1, :, 0].any() and want[fill, :, 0].all()        # none if H divides W)
    assert win.dtype == np.float32 and same_bits(win, want)
    assert_c(c, c64, quiet)
    assert silent.dtype == np.uint8 and not silent.any()


def test_window_flags_silence_per_row(O):
    W, H = 1200, 400
    blocks = noise(2, W, H)
    quiet_steps = -(-W // H) + 1
    live = blocks.copy()
    blocks[:quiet_steps, 1] = 0.0
    win, c, silent = run_window(O, blocks, W)
    want, c64, quiet = windows64(blocks, W)
    assert silent[:, 1].tolist() == [1] * quiet_steps + [0] * (blocks.shape[0] - quiet_steps)
    assert not silent[:, [0, 2]].any() and np.array_equal(silent.astype(bool), quiet)
    assert (c[:quiet_steps, 1] == 1.0).all() and not win[:quiet_steps, 1].any()
    assert same_bits(win, want)
    assert_c(c, c64, quiet)
    # the other rows are what they are when row 1 carries noise all along, bit for bit
    win2, c2, _ = run_window(O, live, W)
    assert same_bits(win[:, [0, 2]], win2[:, [0, 2]]) and same_bits(c[:, [0, 2]], c2[:, [0, 2]])


def test_window_after_a_row_reset(O):
    """definition 5: a row whose counter and ring row are zeroed is a fresh stream; here after four steps of H = 208, with the ring
    write position at 832 of 1200"""
    W, H = 1200, 208
    blocks = noise(3, W, H)
    win, c, silent = run_window(O, blocks, W, reset=(4, 1))
    base, cb, _ = run_window(O, blocks, W)
    fresh, cf, _ = run_window(O, blocks[4:], W)
    assert same_bits(win[:, [0, 2]], base[:, [0, 2]]) and same_bits(c[:, [0, 2]], cb[:, [0, 2]])
    assert same_bits(win[:4, 1], base[:4, 1]) and same_bits(win[4:, 1], fresh[:, 1]) and same_bits(c[4:, 1], cf[:, 1])
    assert not same_bits(win[4:, 1], base[4:, 1])
    want, c64, quiet = windows64(blocks[4:], W)
    assert same_bits(win[4:, 1], want[:, 1])
    assert_c(c[4:, 1], c64[:, 1], quiet[:, 1])
    assert not silent.any()


def test_window_with_counters_the_library_does_not_produce(O):
    """a caller that writes pos itself: counters that are no multiple of 4 (a quad may then straddle the ring's end: 4-byte accesses)
    follow the same definition; a negative counter gets a zero window, flagged silent, and its ring row is left alone"""
    W, H = 1200, 400
    rs = np.random.RandomState(5)
    ring = (0.1 * rs.randn(4, W)).astype(np.float32)
    block = (0.1 * rs.randn(4, H)).astype(np.float32)
    pos = np.array([6, 1198, 2 * W + 802, -5], np.int64)
    want_ring, want = ring.copy(), np.zeros((4, W), np.float32)
    for b in range(3):
        want_ring[b, (pos[b] + np.arange(H)) % W] = block[b]
        g = pos[b] + H - W + np.arange(W)
        want[b] = np.where(g >= 0, want_ring[b, g % W], 0.0)
    assert (pos[1] % W) + H > W and (pos[2] % W) + H > W and not want[0, :W - 406].any()
    dr, dp = dev(ring), dev(pos)
    win, c, silent = O.stream_window(dev(block), dr, dp)
    assert same_bits(win.cpu().numpy(), want) and same_bits(dr.cpu().numpy(), want_ring) and dp.cpu().tolist() == pos.tolist()
    assert silent.cpu().tolist() == [0, 0, 0, 1] and float(c[3]) == 1.0
    r = np.minimum(pos[:3] + H, W)
    c64 = np.sqrt(r / np.sum(want[:3].astype(np.float64) ** 2, axis=1))
    assert_c(c.cpu().numpy()[:3], c64, np.zeros(3, bool))


def emit64(y, c, silent, tail, pos, H, A, V):
    """step 3 in fp64 on the same fp32 inputs -> (out [B, H], new tail [B, D], magnitude of the bar [B, H], g < 0 [B, H])"""
    y, c, tail = np.asarray(y, np.float64), np.asarray(c, np.float64), np.asarray(tail, np.float64)
    B, W = y.shape
    D = A + V
    with np.errstate(invalid='ignore'):
        e = np.where(np.asarray(silent).astype(bool)[:, None], 0.0, y / c[:, None])
    j = np.arange(H)
    v = e[:, W - H - D + j]
    w = np.where(j < V, (j + 0.5) / V, 1.0)
    old = np.zeros((B, H))
    m = min(V, H)
    old[:, :m] = tail[:, :m]
    before = (np.asarray(pos, np.int64)[:, None] - D + j) < 0           # g = n - H - D + j with n = pos + H
    out = np.where(before, 0.0, w * v + (1.0 - w) * old)
    return out, e[:, W - D:], np.abs(v) + np.abs(old), before


@pytest.mark.parametrize('W,H,A,V', EMITS)
def test_emit_against_fp64(O, W, H, A, V):
    D, B = A + V, 4
    rs = np.random.RandomState(W + H + A + V)
    y = rs.randn(B, W).astype(np.float32)
    c = rs.uniform(0.5, 2.0, B).astype(np.float32)
    tail = rs.randn(B, D).astype(np.float32)
    pos = np.array([0, max(D - H // 2, 0), 10 * H, 10 * H], np.int64)   # g < 0 (where D >= H) or straddling, straddling, g > 0
    silent = np.array([0, 0, 0, 1], np.uint8)
    y[3], c[3] = np.nan, 1.0                                            # a silent row: its y must not be used, whatever it holds
    ref, new_tail, mag, before = emit64(y, c, silent, tail, pos, H, A, V)
    assert before.any() and (~before[:2]).any() and not before[2:].any() and (D < H or before[0].all())
    dt, dp = dev(tail), dev(pos)
    out = O.stream_emit(dev(y), dev(c), dev(silent), dt, dp, H, A, V).cpu().numpy()
    assert out.shape == (B, H) and np.isfinite(out).all()
    err, tol = np.abs(out.astype(np.float64) - ref), EPS * mag + 1e-12
    print(f'max |err| {err.max():.3e}  worst err - tol {(err - tol).max():.3e}')
    assert (err <= tol).all()
    assert (out[before] == 0.0).all()
    got_tail = dt.cpu().numpy()
    assert (np.abs(got_tail.astype(np.float64) - new_tail) <= 2.0 ** -23 * np.abs(new_tail)).all()
    assert dp.cpu().tolist() == (pos + H).tolist()
    # the silent row: nothing of its NaN y comes out -- past the fade exact zeros, inside it only what the old tail still holds
    # (under the bar above); its new tail is exact zeros, so its next step is exact zeros throughout
    assert not out[3, V:].any() and not got_tail[3].any() and np.abs(out[2]).max() > 0
    again = O.stream_emit(dev(y), dev(c), dev(silent), dt, dp, H, A, V).cpu().numpy()
    assert not again[3].any() and not dt[3].any() and dp.cpu().tolist() == (pos + 2 * H).tolist()


@pytest.mark.parametrize('W,H', WINDOWS)
def test_emit_of_window_is_the_identity(O, W, H):
    """no model: y = c * window.  The pushed outputs, then the flush, without the first D samples are the input; a shift by a
    single sample anywhere would show as an error of order one.  Bar: the product and the division round once each, then the blend."""
    A, V = FADES[(W, H)]
    D = A + V
    blocks = noise(4, W, H)
    steps = blocks.shape[0]
    ring, tail = torch.zeros(B_, W, device='cuda'), torch.zeros(B_, D, device='cuda')
    pos = torch.zeros(B_, dtype=torch.int64, device='cuda')
    d, outs = dev(blocks), []
    for k in range(steps):
        win, c, silent = O.stream_window(d[k], ring, pos)
        outs.append(O.stream_emit(win * c[:, None], c, silent, tail, pos, H, A, V))
    assert pos.cpu().tolist() == [steps * H] * B_
    got = torch.cat(outs + [tail], dim=1).cpu().numpy().astype(np.float64)
    x = blocks.transpose(1, 0, 2).reshape(B_, steps * H).astype(np.float64)
    assert got.shape == (B_, steps * H + D) and not got[:, :D].any()
    err = np.abs(got[:, D:] - x)
    print('max |err|', err.max())
    assert (err <= 2 * EPS * np.abs(x) + 1e-12).all()


def test_launchers_refuse_bad_operands_and_launch_nothing(O):
    from speech_enhancement_amd._lib import SeHipError
    W, H, A, V = 1200, 400, 200, 100
    z = lambda *s, **k: torch.zeros(*s, device='cuda', **k)                         # noqa: E731
    pos = torch.full((B_,), 7 * H, dtype=torch.int64, device='cuda')
    ring, win, out = z(B_, W), torch.full((B_, W), 5.0, device='cuda'), torch.full((B_, H), 5.0, device='cuda')
    tail = torch.full((B_, A + V), 3.0, device='cuda')
    y, c, silent = torch.ones(B_, W, device='cuda'), torch.ones(B_, device='cuda'), z(B_, dtype=torch.uint8)
    bad = (SeHipError, ValueError)
    with pytest.raises(bad):                                                        # H % 4 != 0
        O.stream_window(torch.ones(B_, 402, device='cuda'), ring, pos, win)
    with pytest.raises(bad):
        O.stream_emit(y, c, silent, tail, pos, 402, A, V, torch.full((B_, 402), 5.0, device='cuda'))
    with pytest.raises(bad):                                                        # V > H
        O.stream_emit(y, c, silent, z(B_, 401), pos, H, 0, 401, out)
    with pytest.raises(bad):                                                        # H + D > W
        O.stream_emit(y, c, silent, z(B_, 801), pos, H, 701, 100, out)
    with pytest.raises(bad):                                                        # the tail is not [B, D]
        O.stream_emit(y, c, silent, tail, pos, H, A, V + 4, out)
    with pytest.raises(bad):                                                        # a CPU tensor
        O.stream_window(torch.ones(B_, H), ring, pos, win)
    with pytest.raises(bad):
        O.stream_emit(y, c.cpu(), silent, tail, pos, H, A, V, out)
    with pytest.raises(bad):
        O.stream_emit(y, c, silent, tail, pos.cpu(), H, A, V, out)
    with pytest.raises(bad):                                                        # a non-contiguous operand
        O.stream_window(torch.ones(B_, 2 * H, device='cuda')[:, ::2], ring, pos, win)
    with pytest.raises(bad):
        O.stream_window(torch.ones(B_, H, device='cuda'), z(B_, 2 * W)[:, ::2], pos, win)
    with pytest.raises(bad):
        O.stream_emit(torch.ones(B_, 2 * W, device='cuda')[:, ::2], c, silent, tail, pos, H, A, V, out)
    with pytest.raises(bad):                                                        # not the counter's type
        O.stream_emit(y, c, silent, tail, pos.int(), H, A, V, out)
    torch.cuda.synchronize()
    assert pos.cpu().tolist() == [7 * H] * B_ and not ring.any()
    assert bool((win == 5.0).all()) and bool((out == 5.0).all()) and bool((tail == 3.0).all())
