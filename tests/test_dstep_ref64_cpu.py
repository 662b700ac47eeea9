"""The float64 references of tests/dstep_ref64.py against CPU float64 autograd (through the oracle's own definitions
where it has one) and torch.optim.Adam: they must agree to ~1e-12, or the GPU parity tests measure the wrong thing."""
import math

import pytest
import torch
import torch.nn.functional as F

import dstep_ref64 as R
from oracle import contrad_oracle as O

f64 = torch.float64
TOL = 1e-12


def close(a, b, tol=TOL):
    a, b = torch.as_tensor(a, dtype=f64), torch.as_tensor(b, dtype=f64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()
    assert err < tol, err


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('mode,N,D', [(0, 5, 3), (0, 1, 8), (1, 2, 4), (1, 7, 16)])
def test_contrast(mode, N, D):
    g = gen(N * 10 + mode)
    R_ = (2 if mode == 0 else 3) * N
    z = F.normalize(torch.randn(R_, D, generator=g, dtype=f64)).requires_grad_()
    temp = 0.1
    if mode == 0:
        ref = O.nt_xent(z[:N], z[N:], temp)
    else:
        ref = O.supcon_fake(z[:N], z[N:2 * N], z[2 * N:], temp)
    ref.backward()
    loss, lse, dz = R.contrast(z.detach(), N, mode, temp)
    close(loss, ref.detach())
    close(dz, z.grad)
    S = z.detach() @ z.detach().t() / temp
    S.fill_diagonal_(-5e4)
    close(lse, torch.logsumexp(S, 1))


def test_l2norm():
    u = (torch.randn(6, 5, generator=gen(1), dtype=f64) * 3).requires_grad_()
    dz = torch.randn(6, 5, generator=gen(2), dtype=f64)
    z = F.normalize(u, eps=1e-12)
    (z * dz).sum().backward()
    rz, inv = R.l2norm(u.detach())
    close(rz, z.detach())
    close(inv, 1 / u.detach().norm(dim=1))
    close(R.l2norm_bwd(dz, u.detach()), u.grad)


@pytest.mark.parametrize('training', [True, False])
def test_spectral_norm(training):
    K, C, T = 5, 3, 4
    g = gen(3)
    w = torch.randn(K, C, 2, 2, generator=g, dtype=f64)
    u, v = F.normalize(torch.randn(K, generator=g, dtype=f64), dim=0), F.normalize(torch.randn(C * T, generator=g, dtype=f64), dim=0)
    sd = {'l.weight_orig': w.clone().requires_grad_(), 'l.weight_u': u.clone(), 'l.weight_v': v.clone()}
    w_eff = O.spectral_norm_weight(sd, 'l', training=training)
    ge = torch.randn(w_eff.shape, generator=g, dtype=f64)
    (w_eff * ge).sum().backward()
    weff, u2, v2, sigma = R.sn_prep(w.reshape(K, -1), u, v, training)
    close(weff, w_eff.detach().reshape(K, -1))
    close(u2, sd['l.weight_u'])
    close(v2, sd['l.weight_v'])
    close(R.sn_grad(ge.reshape(K, -1), w.reshape(K, -1), u2, v2), sd['l.weight_orig'].grad.reshape(K, -1))
    # packed layout: row tap * C + c, column k
    wp = R.pack(w.reshape(K, -1), C, T)
    assert torch.equal(wp, w.permute(2, 3, 1, 0).reshape(T * C, K))
    assert torch.equal(R.unpack(torch.cat([wp, torch.zeros(T * C, 3, dtype=f64)], 1), K, C, T), w.reshape(K, -1))
    ws, _, _, s = R.sn_prep(w.reshape(K, -1), None, None, training, fixed_scale=0.25)
    close(ws, w.reshape(K, -1) * 0.25)
    close(R.sn_grad(ge.reshape(K, -1), w.reshape(K, -1), None, None, fixed_scale=0.25), ge.reshape(K, -1) * 0.25)


@pytest.mark.parametrize('k', [1, 3])
def test_rgb_convs(k):
    g = gen(k)
    N, H, W, K = 2, 5, 6, 8
    img = torch.rand(N, 3, H, W, generator=g, dtype=f64).requires_grad_()
    w = (torch.randn(K, 3, k, k, generator=g, dtype=f64) * 0.3).requires_grad_()
    b = torch.randn(K, generator=g, dtype=f64).requires_grad_()
    y_lin = F.conv2d(img * 2 - 1, w, b, padding=k // 2)
    close(R.rgb_fwd(img.detach(), w.detach(), b.detach(), 2.0, -1.0, 0.2, 1.5),
          (F.leaky_relu(y_lin, 0.2) * 1.5).detach().permute(0, 2, 3, 1))
    gy = torch.randn(y_lin.shape, generator=g, dtype=f64)
    gi, gw, gb = torch.autograd.grad(y_lin, (img, w, b), gy)
    dw, db = R.rgb_wgrad(img.detach(), gy.permute(0, 2, 3, 1), k, 2.0, -1.0)
    close(dw, gw)
    close(db, gb)
    close(R.rgb_dgrad(gy.permute(0, 2, 3, 1), w.detach(), None, out_scale=2.0), gi)
    # generator / ToRGB form: modulation, residual, bias, tanh, affine output
    mod = torch.rand(N, K, generator=g, dtype=f64) + 0.5
    res = torch.randn(N, 3, H, W, generator=g, dtype=f64)
    bb = torch.randn(3, generator=g, dtype=f64)
    ws = w.detach()[None] * mod[:, :, None, None, None]              # per-sample modulated weights
    ref = torch.stack([F.conv_transpose2d(gy[i:i + 1], ws[i], bb, padding=k // 2)[0] for i in range(N)])
    close(R.rgb_dgrad(gy.permute(0, 2, 3, 1), w.detach(), bb, 1, 0.5, 0.5, mod, res), torch.tanh(ref + res) * 0.5 + 0.5)


def test_colstats_and_bn():
    g = gen(5)
    M, K, P = 12, 8, 4
    x = (torch.randn(M, K, generator=g, dtype=f64) + 3).requires_grad_()
    close(R.colstats(x.detach()), torch.stack([x.detach().sum(0), (x.detach() ** 2).sum(0)]))
    gamma, beta = torch.rand(K, generator=g, dtype=f64) + 0.5, torch.randn(K, generator=g, dtype=f64) * 0.3
    gm, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rm, rv = torch.randn(K, generator=g, dtype=f64), torch.rand(K, generator=g, dtype=f64) + 0.5
    cb = torch.randn(K, generator=g, dtype=f64)
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.relu(F.batch_norm((x + cb)[:, :, None], rm2, rv2, gm, bt, True, 0.1, 1e-5))[:, :, 0]
    close(R.bn_relu(x.detach(), gamma, beta, 1e-5), y.detach())
    nrm, nrv = R.bn_running(rm, rv, x.detach(), cb, 0.1)
    close(nrm, rm2)
    close(nrv, rv2)
    dy = torch.randn(M, K, generator=g, dtype=f64)
    gx, ggm, gbt = torch.autograd.grad(y, (x, gm, bt), dy)
    dx, dgm, dbt = R.bn_relu_bwd(dy, x.detach(), gamma, beta, 1e-5)
    close(dx, gx)
    close(dgm, ggm)
    close(dbt, gbt)
    dx2, _, _ = R.bn_relu_bwd(dy, x.detach(), gamma, beta, 1e-5, mask=y.detach() > 0)
    close(dx2, gx)
    # perm_hw: column c * P + hw of the input lands at NHWC position (hw, c)
    yp = R.bn_relu(x.detach(), gamma, beta, 1e-5, perm_hw=P)
    assert torch.equal(yp.reshape(M, P, K // P).permute(0, 2, 1).reshape(M, K), R.bn_relu(x.detach(), gamma, beta, 1e-5))


@pytest.mark.parametrize('kind', ['nonsat', 'wgan', 'hinge', 'lsgan'])
def test_gan_losses(kind):
    g = gen(6)
    d = (torch.randn(2, 9, generator=g, dtype=f64) * 4).requires_grad_()
    ref = O.gan_d_loss(d[0], d[1], kind)
    ref.backward()
    loss, gr, gg = R.gan_d(d.detach()[0], d.detach()[1], kind)
    close(loss, ref.detach())
    close(gr, d.grad[0])
    close(gg, d.grad[1])
    dg = d.detach()[0].clone().requires_grad_()
    refg = (F.softplus(-dg).mean() if kind == 'nonsat' else
            (0.5 * ((dg - 1.0) ** 2).mean() if kind == 'lsgan' else -dg.mean()))
    refg.backward()
    lg, gg2 = R.gan_g(dg.detach(), kind)
    close(lg, refg.detach())
    close(gg2, dg.grad)


@pytest.mark.parametrize('grad_scale', [1.0, 0.25])
def test_adam_matches_torch_optim(grad_scale):
    g = gen(7)
    p0 = torch.randn(37, generator=g, dtype=f64)
    grads = [torch.randn(37, generator=g, dtype=f64) for _ in range(5)]
    lr, b1, b2, eps = 2e-3, 0.5, 0.999, 1e-8
    p = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    q, m, v = p0.clone(), torch.zeros(37, dtype=f64), torch.zeros(37, dtype=f64)
    for t, gr in enumerate(grads, 1):
        p.grad = gr * grad_scale
        opt.step()
        q, m, v = R.adam(q, gr, m, v, t, lr, b1, b2, eps, grad_scale)
        close(q, p.detach())
        close(m, opt.state[p]['exp_avg'])
        close(v, opt.state[p]['exp_avg_sq'])
    assert math.isfinite(q.sum().item())
