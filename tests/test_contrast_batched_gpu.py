"""Both contrastive problems of the ContraD D-step per launch (contrad_contrast_{fwd,bwd}_batched, contrad_l2norm_{fwd,bwd}_
batched) against two single calls: bitwise equal, forward and backward; and against the oracle at test_contrast_gpu.py's
tolerance."""
import pytest
import torch
import torch.nn.functional as F

from contrad_amd import ops
from oracle import contrad_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-3          # tests/test_contrast_gpu.py


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _single(u1, u2, N, temp, gs):
    z1, inv1 = ops.l2norm_fwd(u1[:2 * N])
    z2, inv2 = ops.l2norm_fwd(u2)
    l1, lse1 = ops.contrast_fwd(z1, N, 0, temp)
    l2, lse2 = ops.contrast_fwd(z2, N, 1, temp)
    dz1 = ops.contrast_bwd(z1, lse1, N, 0, temp, gs[0])
    dz2 = ops.contrast_bwd(z2, lse2, N, 1, temp, gs[1])
    g1 = torch.zeros_like(u1)
    ops.l2norm_bwd(dz1, z1, inv1, out=g1[:2 * N])
    g2 = ops.l2norm_bwd(dz2, z2, inv2)
    return dict(z1=z1, inv1=inv1, z2=z2, inv2=inv2, l1=l1, lse1=lse1, l2=l2, lse2=lse2, dz1=dz1, dz2=dz2, g1=g1, g2=g2)


def _batched(u1, u2, N, temp, gs):
    z1, inv1, z2, inv2 = ops.l2norm_fwd_pair(u1[:2 * N], u2)
    l1, lse1, l2, lse2 = ops.contrast_fwd_pair(z1, N, 0, z2, N, 1, temp)
    dz1, dz2 = ops.contrast_bwd_pair(z1, lse1, N, 0, gs[0], z2, lse2, N, 1, gs[1], temp)
    g1 = torch.full_like(u1, float('nan'))          # rows 2N: must come back as zeros
    g2 = torch.full_like(u2, float('nan'))
    ops.l2norm_bwd_pair(((dz1, z1, inv1, g1[:2 * N], u1.shape[0] - 2 * N), (dz2, z2, inv2, g2, 0)))
    return dict(z1=z1, inv1=inv1, z2=z2, inv2=inv2, l1=l1, lse1=lse1, l2=l2, lse2=lse2, dz1=dz1, dz2=dz2, g1=g1, g2=g2)


@pytest.mark.parametrize('scaled', [False, True], ids=['unit', 'grad_scale'])
@pytest.mark.parametrize('N,D', [(512, 128), (64, 128), (33, 96), (2, 128), (1200, 64)])
def test_batched_equals_two_single_calls(N, D, scaled):
    g = torch.Generator().manual_seed(N + D)
    u1, u2 = torch.randn(3 * N, D, generator=g).to(DEV), torch.randn(3 * N, D, generator=g).to(DEV)
    gs = (torch.tensor([0.7], device=DEV), torch.tensor([1.3], device=DEV)) if scaled else (None, None)
    a, b = _single(u1, u2, N, 0.1, gs), _batched(u1, u2, N, 0.1, gs)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_different_feature_widths_run_one_after_the_other():
    """Two problems whose D fall into different kernel instances: still the results of the single calls."""
    N = 40
    g = torch.Generator().manual_seed(3)
    z1 = F.normalize(torch.randn(2 * N, 48, generator=g)).to(DEV)
    z2 = F.normalize(torch.randn(3 * N, 200, generator=g)).to(DEV)
    l1, lse1, l2, lse2 = ops.contrast_fwd_pair(z1, N, 0, z2, N, 1, 0.2)
    r1, rl1 = ops.contrast_fwd(z1, N, 0, 0.2)
    r2, rl2 = ops.contrast_fwd(z2, N, 1, 0.2)
    assert torch.equal(l1, r1) and torch.equal(lse1, rl1) and torch.equal(l2, r2) and torch.equal(lse2, rl2)
    dz1, dz2 = ops.contrast_bwd_pair(z1, lse1, N, 0, None, z2, lse2, N, 1, None, 0.2)
    assert torch.equal(dz1, ops.contrast_bwd(z1, rl1, N, 0, 0.2)) and torch.equal(dz2, ops.contrast_bwd(z2, rl2, N, 1, 0.2))


@pytest.mark.parametrize('N,D,temp', [(512, 128, 0.1), (64, 128, 0.1), (100, 96, 0.2)])
def test_batched_against_oracle(N, D, temp):
    g = torch.Generator().manual_seed(N)
    u1 = torch.randn(3 * N, D, generator=g)
    u2 = torch.randn(3 * N, D, generator=g)
    o1, o2 = u1.clone().requires_grad_(), u2.clone().requires_grad_()
    v, r = F.normalize(o1), F.normalize(o2)
    r1 = O.nt_xent(v[:N], v[N:2 * N], temp)
    r2 = O.supcon_fake(r[:N], r[N:2 * N], r[2 * N:], temp)
    (r1 + r2).backward()
    b = _batched(u1.to(DEV), u2.to(DEV), N, temp, (None, None))
    assert abs(b['l1'].item() - r1.item()) < TOL * abs(r1.item())
    assert abs(b['l2'].item() - r2.item()) < TOL * abs(r2.item())
    assert rel(b['g1'].cpu(), o1.grad) < TOL
    assert rel(b['g2'].cpu(), o2.grad) < TOL


@pytest.mark.parametrize('N', [64, 512])
def test_loss_node_equals_separate_calls(N):
    """_ContraDContrastive (the node of the D-step) on the batched launches against the single calls, through autograd."""
    from contrad_amd.training.gan.contrad import _ContraDContrastive
    g = torch.Generator().manual_seed(N)
    p1 = torch.randn(3 * N, 128, generator=g).to(DEV).requires_grad_()
    p2 = torch.randn(3 * N, 128, generator=g).to(DEV).requires_grad_()
    s, c = _ContraDContrastive.apply(p1, p2, N, 0.1, False)
    (s + 0.5 * c).backward()
    one, half = torch.tensor([1.0], device=DEV), torch.tensor([0.5], device=DEV)
    a = _single(p1.detach(), p2.detach(), N, 0.1, (one, half))
    assert torch.equal(s.detach().reshape(1), a['l1']) and torch.equal(c.detach().reshape(1), a['l2'])
    assert torch.equal(p1.grad, a['g1']) and torch.equal(p2.grad, a['g2'])
