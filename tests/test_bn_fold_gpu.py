"""GPU parity of the Conformer BatchNorm + Swish backward whose apply pass runs inside the fused depthwise backward (round 7:
se_dwconv31_bn_bwd_fused after norm_prelu_bwd's reduce pass) against fp64 autograd and against the two-pass form (norm_prelu_bwd
reduce + apply, then se_dwconv31_bwd_fused)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).cuda()


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def relerr_paths(new, old, k):
    """the depthwise bias gradient of a conv in front of a train-mode BatchNorm is sum_tokens dH = 0 up to rounding: measured against
    the scale of the weight gradient instead of its own"""
    if k == 'dbw':
        return float((new[k].double() - old[k].double()).abs().max() / float(old['dw'].abs().max()))
    return relerr(new[k], old[k])


def _bn_stats(h):
    """(mean, rstd) [1][128][2] of the BatchNorm batch statistics (biased variance, eps 1e-5) -- norm_finalize's layout"""
    hd = h.double()
    mean, var = hd.mean(0), hd.var(0, unbiased=False)
    return torch.stack([mean, (var + 1e-5).rsqrt()], -1).float().view(1, 128, 2).contiguous()


def _grads():
    return dict(dg=torch.full((128,), 0.5, device='cuda'), db=torch.full((128,), -0.25, device='cuda'),
                dw=torch.zeros(128, 31, device='cuda'), dbw=torch.zeros(128, device='cuda'), amax=torch.zeros(1, device='cuda'))


def _new_path(dact, h, mr, g, b, w, u, gate, geom, sync=False):
    from speech_enhancement_amd import ops as O
    M = dact.shape[0]
    r = _grads()
    red = O.bn_swish_bwd_sums(h, mr, g, b, dact, r['dg'], r['db'], float(M), allreduce=(lambda t: None) if sync else None)
    kw = {} if sync else dict(dg=r['dg'], dbeta=r['db'])
    r['dz'] = O.dwconv31_bn_bwd_fused(dact, h, mr, g, b, red, float(M), w, u, gate, r['dw'], r['dbw'], geom, amax=r['amax'], **kw)
    return r


def _old_path(dact, h, mr, g, b, w, u, gate, geom):
    from speech_enhancement_amd import ops as O
    M = dact.shape[0]
    r = _grads()
    dh = torch.empty(M, 128, device='cuda')
    O.norm_prelu_bwd(h, 128, 0, mr, g, b, None, dact, 128, 0, dh, 128, 0, r['dg'], r['db'], None, 1, M, 128, per_batch=False, act=1,
                     count=float(M))
    r['dz'] = O.dwconv31_bwd_fused(dh, w, u, gate, r['dw'], r['dbw'], geom, amax=r['amax'])
    return r


def _operands(B, T, Fq, seed=0):
    M = B * T * Fq
    g, b = rnd(128, seed=seed + 2, scale=0.3, shift=1.0), rnd(128, seed=seed + 3, scale=0.3)
    w = rnd(128, 31, seed=seed + 4, scale=0.2)
    z = rnd(B, T, Fq, 256, seed=seed + 5)
    dact = rnd(M, 128, seed=seed + 6)
    return M, g, b, w, z, dact


@pytest.mark.parametrize('axis,B,T,Fq', [('time', 2, 37, 5), ('freq', 2, 7, 101), ('time', 1, 321, 9), ('freq', 3, 5, 113),
                                         ('time', 2, 112, 3), ('freq', 1, 300, 16), ('time', 1, 16, 2), ('time', 1, 1601, 3)])
def test_folded_conv_module_backward_against_fp64(axis, B, T, Fq):
    """reduce pass + se_dwconv31_bn_bwd_fused against fp64 autograd of BatchNorm-Swish (batch statistics) -> depthwise -> GLU behind a
    given output gradient: dZ, max |dZ|, dgamma, dbeta (accumulated), dW / db of the depthwise conv; tile boundaries 112 / 113, both
    axes, a 10 s clip (T = 1601)"""
    from speech_enhancement_amd import attention as A
    M, g, b, w, z, dact = _operands(B, T, Fq)
    geom = A.seq_geometry(B, T, Fq, axis)
    z64 = z.double().requires_grad_(True)
    w64 = w.double().view(128, 1, 31).requires_grad_(True)
    bw64 = rnd(128, seed=9, scale=0.1).double().requires_grad_(True)
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    u64 = z64[..., :128] * torch.sigmoid(z64[..., 128:])
    sq = u64.permute(0, 2, 3, 1) if axis == 'time' else u64.permute(0, 1, 3, 2)
    rr = F.conv1d(F.pad(sq.reshape(-1, 128, sq.shape[-1]), (15, 15)), w64, bw64, groups=128).reshape(sq.shape)
    h64 = (rr.permute(0, 3, 1, 2) if axis == 'time' else rr.permute(0, 1, 3, 2)).reshape(M, 128)
    F.silu(F.batch_norm(h64, None, None, g64, b64, training=True, eps=1e-5)).backward(dact.double())
    h = h64.detach().float().contiguous()
    u = u64.detach().float().contiguous().view(M, 128)
    gate = z[..., 128:].contiguous().view(M, 128)
    for sync in (False, True):
        r = _new_path(dact, h, _bn_stats(h), g, b, w, u, gate, geom, sync=sync)
        assert relerr(r['dz'].view(B, T, Fq, 256), z64.grad) < 1e-4
        assert abs(float(r['amax']) - float(r['dz'].abs().max())) <= 1e-6 * float(r['amax'])
        assert relerr(r['dg'] - 0.5, g64.grad) < 1e-4 and relerr(r['db'] + 0.25, b64.grad) < 1e-4
        assert relerr(r['dw'], w64.grad.view(128, 31)) < 1e-4
        # the depthwise bias gradient is sum_tokens dH = 0 exactly (the batch statistics are over the same tokens): fp32 noise only
        assert float((r['dbw'].double() - bw64.grad).abs().max()) <= 1e-5 * float(w64.grad.abs().max())


@pytest.mark.parametrize('axis', ['time', 'freq'])
def test_folded_path_matches_two_pass_path_at_bench_shape(axis):
    """the new path against the two-pass path at the train step's shape (M = 16 x 321 x 101 = 518 736 tokens): the same statistics
    (the reduce pass is shared) and the apply pass's arithmetic -- dZ and the BatchNorm parameter gradients agree to the last bits"""
    from speech_enhancement_amd import attention as A
    M, g, b, w, z, dact = _operands(16, 321, 101, seed=20)
    u = (z[..., :128] * torch.sigmoid(z[..., 128:])).contiguous().view(M, 128)
    gate = z[..., 128:].contiguous().view(M, 128)
    h = rnd(M, 128, seed=27, scale=2.0, shift=0.5)
    geom = A.seq_geometry(16, 321, 101, axis)
    mr = _bn_stats(h)
    old = _old_path(dact, h, mr, g, b, w, u, gate, geom)
    for sync in (False, True):
        new = _new_path(dact, h, mr, g, b, w, u, gate, geom, sync=sync)
        assert torch.equal(new['dg'], old['dg']) and torch.equal(new['db'], old['db'])
        for k, tol in (('dz', 1e-6), ('amax', 1e-6), ('dw', 1e-5), ('dbw', 1e-5)):
            assert relerr_paths(new, old, k) < tol, k
