"""Latent recovery on the GPU (contrad_amd/recover.py; csrc/cddls.hip: the recovery forms of the energy and image-end
kernels, the Adam form of the latent update): every form alone against float64, one step and a three-step trajectory
against tests/recover_ref64.py, a planted target, descent, eager against ``--graph``, the invariants, the CLI.

Tolerances (each recorded through ``margin``); u = 2^-24, the unit roundoff of fp32:
  loss form    |err| <= 1e-5 * (sum of |terms|), the energy bound of test_cddls_gpu.py (its header has the derivation: at most
               8192 + 3072 fp32 terms per sample, a strided partial per lane, then a tree); every term here is positive, so
               the sum of |terms| is the reference value itself
  residual     r = ((2 lam) / F) * (phi - phi*): one rounding each in the quotient, the difference and the product, 3 u
               relative; held to RTOL_U = 4 u times the largest |r| of the case (absolute, as KTOL is)
  image end    g_lin = fma(2 / P, o - x, g) * (0.5 * (1 - t * t)), t = 2 o - 1: seven roundings (o - x, the fma, t, t t, 1 - t t,
               the product; the factor 2 / P itself) on magnitudes <= 2.5 (|g| <= 2.3 by construction, the rest <= 1):
               IETOL = 8 u * 2.5 = 1.2e-6 absolute
  Adam form    m, v: two roundings of products and one of the fma, held to 4 u of (b1 |m| + (1 - b1) |g|) resp.
               (b2 v + (1 - b2) g^2) per element; z: u = (m / c1) / (sqrt(v / c2) + eps) carries <= 8 roundings (5e-7
               relative), |u| <= (1 - b1) / sqrt(1 - b2) / min(c1 / sqrt(c2)) <= 4.5 at the betas used, lr = 0.3:
               0.3 * 4.5 * 5e-7 + u = 7.4e-7; AZTOL = 2e-6 absolute
  step         rel L2 1e-3 on the same linear region (TOL), 1e-2 raw (FLIP_TOL): the project's existing values
"""
import os
import shutil

import numpy as np
import pytest
import torch

import cddls_ref64 as R
import cddls_snresnet_ref64 as RS
import recover_ref64 as V
from conftest import ROOT
from png_reader import read_png

pytestmark = pytest.mark.gpu
TOL, FLIP_TOL = 1e-3, 1e-2
U = 2.0 ** -24
RTOL_U, IETOL, AZTOL, MV_U = 4 * U, 8 * U * 2.5, 2e-6, 4 * U
LAM = 2.5                                   # the kernels alone; the steps use V.LAMBDA_FEAT (see recover_ref64.py)
SENTINEL, GUARD = -7.25, 64


def dev():
    return torch.device('cuda', 0)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def unaligned(t):
    """A device copy of ``t`` (flat) that starts 4 bytes past a 16-byte boundary: the kernels' scalar form."""
    buf = torch.empty(t.numel() + 1, device=dev())
    v = buf[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def guarded(*shape):
    """A device tensor of ``shape`` inside a buffer of sentinels -> (view, check that the guards are intact)."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), SENTINEL, device=dev())

    def intact():
        return bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all())
    return big[GUARD:GUARD + n].view(*shape), intact


# ---------------------------------------------------------------------------------------------------------
# the three forms alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,F', [(1, 12, 4), (7, 27, 8), (5, 768, 2048), (3, 3072, 8192), (4, 3072, None)])
def test_loss_form(margin, N, P, F):
    from contrad_amd import ops
    g = gen(N + P)
    gout, xt = torch.rand(N, P, generator=g), torch.rand(N, P, generator=g)
    out, out_ok = guarded(3, N)
    kw, resid_ok = {}, None
    if F is not None:
        phi, phit = torch.randn(N, F, generator=g).relu(), torch.randn(N, F, generator=g).relu()
        resid, resid_ok = guarded(N, F)
        kw = dict(phi=phi.to(dev()), phi_target=phit.to(dev()), resid=resid)
    pix, feat, loss = ops.cddls_recover_loss(gout.to(dev()), xt.to(dev()), LAM if F else 0.0, out=out, **kw)
    rp, rf, rl, rr = V.loss_form(gout.double(), xt.double(), LAM, *((phi.double(), phit.double()) if F else ()))
    tag = 'recover loss N=%d P=%d F=%s ' % (N, P, F)
    margin(tag + 'pix', relmax(pix, rp), 1e-5)
    margin(tag + 'loss', relmax(loss, rl), 1e-5)                # positive terms: the sum of |terms| is the value
    if F is not None:
        margin(tag + 'feat', relmax(feat, rf), 1e-5)
        margin(tag + 'resid', maxabs(resid, rr), RTOL_U * float(rr.abs().max()))
        assert resid_ok() and float(rf.min()) > 0
        assert abs(float(rl[0]) - float(rp[0])) > 0.1 * float(rl[0])        # the feature term carries weight
    else:
        assert float(feat.abs().max()) == 0.0 and torch.equal(loss, pix)
    assert out_ok()
    out2, _ = guarded(3, N)
    if F is not None:
        kw['resid'] = torch.empty(N, F, device=dev())
    ops.cddls_recover_loss(gout.to(dev()), xt.to(dev()), LAM if F else 0.0, out=out2, **kw)
    assert torch.equal(out, out2) and (F is None or torch.equal(kw['resid'], resid))        # two calls: the same bits


@pytest.mark.parametrize('n', [3 * 32 * 32, 3 * 3 * 16 * 16, 1, 7, 4 * (4096 + 3) + 1])
@pytest.mark.parametrize('with_gx', [True, False], ids=['gx', 'nogx'])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'unaligned'])
def test_image_end_form(margin, n, with_gx, aligned):
    """The recovery form takes no z2: there is none in its arguments; P = 12 makes the pixel term as large as g_x."""
    from contrad_amd import ops
    g = gen(n)
    gout, xt, gx = torch.rand(n, generator=g), torch.rand(n, generator=g), (0.5 * torch.randn(n, generator=g)).clamp(-2.3, 2.3)
    put = (lambda t: t.to(dev())) if aligned else unaligned
    if aligned:
        glin, ok = guarded(n)
    else:
        big = torch.full((n + 2 * GUARD + 1,), SENTINEL, device=dev())
        glin = big[GUARD + 1:GUARD + 1 + n]
        assert glin.data_ptr() % 16 == 4
        ok = lambda: bool((big[:GUARD + 1] == SENTINEL).all()) and bool((big[GUARD + 1 + n:] == SENTINEL).all())     # noqa: E731
    P = 12
    ops.cddls_recover_image_end(put(gout), put(xt), glin, P, gx=put(gx) if with_gx else None)
    ref = V.image_end_form(gout.double(), xt.double(), P, gx.double() if with_gx else None)
    margin('recover image_end n=%d gx=%d aligned=%d' % (n, with_gx, aligned), maxabs(glin, ref), IETOL)
    assert ok()
    if n > 100:         # both terms carry weight
        pixel_only = V.image_end_form(gout.double(), xt.double(), P)
        assert float(pixel_only.abs().max()) > 100 * IETOL and (not with_gx or float((ref - pixel_only).abs().max()) > 100 * IETOL)


def _adam_inputs(n, seed, eps):
    g = gen(seed)
    z = torch.rand(n, generator=g) * 2 - 1
    mag = eps * 10.0 ** (torch.rand(n, generator=g) * 6 - 3)             # |g| from 1e-3 eps to 1e3 eps
    gz = mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    gz[torch.rand(n, generator=g) < 0.1] = 0.0
    return z, gz


@pytest.mark.parametrize('n,aligned', [(128, True), (5 * 128, True), (7, False), (4 * (4096 + 3) + 1, True)])
@pytest.mark.parametrize('launches', [1, 4])
def test_adam_form(margin, n, aligned, launches):
    from contrad_amd import ops
    eps, first = V.ADAM_EPS, 41 if launches == 1 else 0
    put = (lambda t: t.to(dev())) if aligned else unaligned
    z, gz = _adam_inputs(n, n + launches, eps)
    g = gen(n)
    m, v = (torch.zeros(n), torch.zeros(n)) if first == 0 else (eps * torch.randn(n, generator=g), (eps * torch.randn(n, generator=g)) ** 2)
    z[0], z[n - 1] = 0.99, -0.99                        # driven into both clamps (n == 1 would keep the second only)
    zd, md, vd = put(z), put(m), put(v)
    state = torch.tensor([first, 0, 0, 0], dtype=torch.int32, device=dev())
    tag = 'recover adam n=%d aligned=%d launches=%d ' % (n, aligned, launches)
    for k in range(launches):
        # every launch against the yardstick's step from the state the launch itself read: the bounds in the header are
        # per launch (over consecutive launches m can cancel to far below the scale its rounding error was made at)
        zr, mr, vr = zd.cpu().double(), md.cpu().double(), vd.cpu().double()
        if k:
            _, gz = _adam_inputs(n, 1000 * k + n, eps)
        gz[0], gz[n - 1] = -1e3 * eps, 1e3 * eps
        b1, b2 = (float(np.float32(b)) for b in V.BETAS)
        scale_m = b1 * mr.abs() + (1 - b1) * gz.double().abs()
        scale_v = b2 * vr + (1 - b2) * gz.double() ** 2
        ops.cddls_recover_update(zd, put(gz), md, vd, V.LR, V.BETAS, eps, state)
        zr, mr, vr = V.adam_form(zr, gz.double(), mr, vr, V.LR, V.BETAS, eps, first + k)
        margin(tag + 'z launch %d' % k, maxabs(zd, zr), AZTOL)
        ok = scale_m > 0
        margin(tag + 'm launch %d' % k, float(((md.cpu().double() - mr).abs()[ok] / scale_m[ok]).max()), MV_U)
        margin(tag + 'v launch %d' % k, float(((vd.cpu().double() - vr).abs()[ok] / scale_v[ok]).max()), MV_U)
        assert bool((md.cpu()[~ok] == 0).all()) and bool((vd.cpu()[~ok] == 0).all())
        assert state.tolist() == [first + k + 1, 0, 0, 0]
    assert float(zd[n - 1]) == -1.0 and float(zd[0]) == 1.0
    assert float(zd.min()) >= -1.0 and float(zd.max()) <= 1.0


@pytest.mark.parametrize('n,aligned', [(5 * 128, True), (7, False)])
def test_adam_form_zero_gradient_leaves_z_bitwise(n, aligned):
    from contrad_amd import ops
    put = (lambda t: t.to(dev())) if aligned else unaligned
    z = torch.rand(n, generator=gen(n)) * 2 - 1
    zd, md, vd = put(z), put(torch.zeros(n)), put(torch.zeros(n))
    state = torch.tensor([3, 0, 0, 0], dtype=torch.int32, device=dev())
    ops.cddls_recover_update(zd, put(torch.zeros(n)), md, vd, V.LR, V.BETAS, 1e-8, state)
    assert torch.equal(zd.cpu(), z) and float(md.abs().max()) == 0.0 and float(vd.abs().max()) == 0.0
    assert state.tolist() == [4, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------
# the recovery
# ---------------------------------------------------------------------------------------------------------
_NETS = {}


def _modules(arch, hw, gsd, dsd):
    from contrad_amd.models.gan import get_architecture
    G, D = get_architecture(arch, (hw, hw, 3))
    full = dict(G.state_dict())
    full.update({k: v.float() for k, v in gsd.items()})
    G.load_state_dict(full)
    D.load_state_dict({k: v.float() for k, v in dsd.items()})
    G.to(dev()).eval(); D.to(dev()).eval()
    for p in list(G.parameters()) + list(D.parameters()):
        p.requires_grad_(False)
    return G, D


def nets(kind):
    """'fixture' (32 x 32), 'trained' (R.trained_like_networks at 16 x 16), 'snresnet18' (32 x 32): float64 state dicts on the
    host and the eval-mode float32 modules on the device, made once per session."""
    if kind not in _NETS:
        if kind == 'fixture':
            gsd, dsd = R.fixture_networks()
            _NETS[kind] = (gsd, dsd) + _modules('sndcgan', 32, gsd, dsd) + (32, 'sndcgan')
        elif kind == 'trained':
            gsd, dsd = R.trained_like_networks(1.0, 16)
            _NETS[kind] = (gsd, dsd) + _modules('sndcgan', 16, gsd, dsd) + (16, 'sndcgan')
        else:
            gsd, dsd = RS.fixture_networks()
            _NETS[kind] = (gsd, dsd) + _modules('snresnet18', 32, gsd, dsd) + (32, 'snresnet18')
    return _NETS[kind]


def cpu_region(region):
    return {'g': [m.cpu() for m in region['g']], 'd': [m.cpu() for m in region['d']]}


@pytest.mark.parametrize('kind,N,feature', [('fixture', 4, False), ('fixture', 4, True), ('trained', 3, False),
                                            ('trained', 3, True), ('snresnet18', 3, True)])
def test_one_step(margin, kind, N, feature):
    """g_z, the losses and the increment of z of one step against the yardstick.  adam_eps is the float64 median |g_z| of
    the case (recover_ref64.median_gradient), so that the increment is a smooth function of the gradient."""
    from contrad_amd.recover import LatentRecovery
    gsd, dsd, G, D, hw, d_type = nets(kind)
    lam = V.LAMBDA_FEAT if feature else 0.0
    z0, target = V.case(N, hw, 500 + N + hw)
    args = dict(image_hw=hw, lam=lam, dsd=dsd if feature else None, d_type=d_type if feature else None)
    eps = V.median_gradient(gsd, z0, target, hw, lam, args['dsd'], args['d_type'])
    S = LatentRecovery(G, N, D=D if feature else None, lambda_feat=lam, lr=V.LR, betas=V.BETAS, adam_eps=eps)
    S.set_targets(target.to(dev()))
    S.start(z0.to(dev()))
    pix, feat, loss = S.losses()
    S.step()
    region = cpu_region(S.linear_region())
    zero = torch.zeros(N, 128, dtype=torch.float64)
    same = V.recovery_step(gsd, z0.double(), zero, zero, target.double(), 0, V.LR, V.BETAS, eps, region=region, **args)
    raw = V.recovery_step(gsd, z0.double(), zero, zero, target.double(), 0, V.LR, V.BETAS, eps, **args)
    tag = 'recover step %s N=%d feature=%d ' % (kind, N, feature)
    for name, ref, tol in (('same region', same, TOL), ('raw', raw, FLIP_TOL)):
        margin(tag + 'g_z ' + name, rel_l2(S.g_z, ref['g_z']), tol)
        margin(tag + 'pix ' + name, relmax(pix, ref['pix']), tol)
        margin(tag + 'loss ' + name, relmax(loss, ref['loss']), tol)
        if feature:
            margin(tag + 'feat ' + name, relmax(feat, ref['feat']), tol)
            margin(tag + 'g_x ' + name, rel_l2(S.g_x, ref['g_x']), tol)
    margin(tag + 'dz same region', rel_l2(S.z.cpu().double() - z0.double(), same['z'] - z0.double()), TOL)
    assert float((same['z'] - z0.double()).abs().max()) > 0.01
    assert S.state.tolist()[:2] == [1, 0]
    assert (feature and float(feat.min()) > 0) or (not feature and float(feat.abs().max()) == 0 and torch.equal(pix, loss))


def test_trajectory(margin):
    """Three steps at N = 4 (pixels only, the fixture networks): the increments of z and the final pix on the kernel's own
    regions, under the condition test_recover_ref64_cpu.py::test_the_trajectory_case_is_well_conditioned asserts."""
    from contrad_amd.recover import LatentRecovery
    gsd, dsd, G, D, hw, _ = nets('fixture')
    z0, target, eps = V.trajectory_case(gsd)
    S = LatentRecovery(G, V.TRAJ_N, lr=V.LR, betas=V.BETAS, adam_eps=eps)
    S.set_targets(target.to(dev()))
    S.start(z0.to(dev()))
    zs, regions = [S.z.cpu().double()], []
    for _ in range(V.TRAJ_STEPS):
        S.step()
        regions.append(cpu_region(S.linear_region()))
        zs.append(S.z.cpu().double())
    pix, _, _ = S.losses()
    steps, ref_pix = V.trajectory(gsd, z0.double(), target.double(), V.TRAJ_STEPS, V.LR, V.BETAS, eps, regions=regions)
    for k, st in enumerate(steps):
        margin('recover trajectory dz same region step %d' % k, rel_l2(zs[k + 1] - zs[k], st['z'] - st['z_prev']), TOL)
    margin('recover trajectory final pix', relmax(pix, ref_pix), TOL)
    assert S.state.tolist()[:2] == [V.TRAJ_STEPS, 0]


@pytest.mark.parametrize('feature', [False, True])
def test_planted_target(feature):
    """x* = G(z*): pix, feat and g_z are exactly 0 at z*, and three steps leave z bitwise where it is."""
    from contrad_amd.recover import LatentRecovery
    gsd, dsd, G, D, hw, _ = nets('fixture')
    N = 4
    zstar = (torch.rand(N, 128, generator=gen(77)) * 2 - 1).to(dev())
    S = LatentRecovery(G, N, D=D if feature else None, lambda_feat=V.LAMBDA_FEAT if feature else 0.0, lr=V.LR, betas=V.BETAS)
    S.start(zstar)
    S.set_targets(S.images())
    S.start(zstar)
    for t in S.losses():
        assert float(t.abs().max()) == 0.0
    for _ in range(3):
        S.step()
        assert float(S.g_z.abs().max()) == 0.0
    assert torch.equal(S.z, zstar) and S.state.tolist()[:2] == [3, 0]
    assert float(S.images().std()) > 0


def test_descent():
    from contrad_amd.recover import LatentRecovery
    gsd, dsd, G, D, hw, _ = nets('fixture')
    N, g = 4, gen(78)
    zstar = (torch.rand(N, 128, generator=g) * 1.6 - 0.8)
    S = LatentRecovery(G, N, lr=0.01)
    S.start(zstar.to(dev()))
    S.set_targets(S.images())
    S.start((zstar + 0.05 * (torch.rand(N, 128, generator=g) * 2 - 1)).to(dev()))
    before = S.losses()[2]
    for _ in range(20):
        S.step()
    after = S.losses()[2]
    assert float(before.min()) > 0 and bool((after < before).all()), (before.tolist(), after.tolist())


def _run(G, D, lam, z0, target, graph, steps=5):
    from contrad_amd.recover import LatentRecovery
    S = LatentRecovery(G, z0.shape[0], D=D, lambda_feat=lam, lr=V.LR, betas=V.BETAS, adam_eps=1e-6, graph=graph)
    S.set_targets(target)
    S.start(z0)
    for _ in range(steps):
        S.step()
    return S, S.z.clone(), S.m.clone(), S.v.clone(), S.images(), torch.stack(S.losses())


@pytest.mark.parametrize('feature', [False, True])
def test_invariants(feature):
    """Eager and --graph runs are bitwise equal over 5 steps, so are two runs; both state dicts stay bit-identical."""
    gsd, dsd, G, D, hw, _ = nets('fixture')
    z0, target = V.case(8, 32, 9)
    z0, target = z0.to(dev()), target.to(dev())
    lam, Dm = (V.LAMBDA_FEAT, D) if feature else (0.0, None)
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in (G, D)]
    S, *a = _run(G, Dm, lam, z0, target, False)
    assert S.state.tolist()[:2] == [5, 0] and bool(torch.isfinite(a[3]).all()) and not torch.equal(a[0], z0)
    for m, sd in zip((G, D), before):
        now = m.state_dict()
        assert list(now) == list(sd) and all(torch.equal(now[k], sd[k]) for k in sd)
    Sg, *b = _run(G, Dm, lam, z0, target, True)                     # eager first step, capture, replays
    assert Sg.graph is not None and all(torch.equal(x, y) for x, y in zip(a, b))
    _, *c = _run(G, Dm, lam, z0, target, False)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    for m, sd in zip((G, D), before):
        now = m.state_dict()
        assert all(torch.equal(now[k], sd[k]) for k in sd)


# ---------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------
def test_cli(tmp_path):
    from contrad_amd import recover
    from contrad_amd.train_gan import main as train_main
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    run = str(tmp_path / 'run')
    train_main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
                '--seed', '5', '--logdir', run])
    if not [f for f in os.listdir(run) if f.endswith('.gin')]:
        shutil.copy(gin, os.path.join(run, 'c10_b64.gin'))
    gen_pt, dis_pt = os.path.join(run, 'gen.pt'), os.path.join(run, 'dis.pt')
    argv = [gen_pt, 'sndcgan', '--synthetic', '--n', '8', '--steps', '3', '--holdout', '--rows', '2', '--seed', '6',
            '--batch_size', '5']
    out = recover.main(argv)
    assert out == os.path.join(run, 'recover_6.json')
    import json
    with open(out) as f:
        js = json.load(f)
    for k in ('model_path', 'architecture', 'data', 'synthetic', 'n', 'holdout', 'steps', 'lr', 'betas', 'adam_eps', 'restarts',
              'lambda_feat', 'dis', 'batch_size', 'seed', 'graph', 'rows', 'image_size', 'train', 'test', 'auc', 'z_score',
              'median_gap', 'note'):
        assert k in js, k
    assert js['n'] == 8 and js['steps'] == 3 and js['lr'] == recover.DEFAULT_LR and js['train']['n'] == js['test']['n'] == 8
    assert set(js['train']) == {'n', 'mean', 'median', 'p10', 'p90', 'psnr_median'} and 0 <= js['auc'] <= 1
    with np.load(os.path.join(run, 'recover_6.npz')) as z:
        assert z['z'].shape == (16, 128) and z['z'].dtype == np.float32 and np.abs(z['z']).max() <= 1
        assert z['pix'].shape == z['feat'].shape == z['index'].shape == z['split'].shape == (16,)
        assert z['index'].tolist() == list(range(8)) * 2 and z['split'].tolist() == [0] * 8 + [1] * 8
        assert (z['pix'] > 0).all() and (z['feat'] == 0).all()
        assert abs(float(np.median(z['pix'][:8].astype(np.float64))) - js['train']['median']) < 1e-12
    png = read_png(os.path.join(run, 'recover_6.png'))
    assert png.shape == recover.figure_shape(2, 32, 32) == (36, 274, 3)
    first = {n: open(os.path.join(run, n), 'rb').read() for n in ('recover_6.json', 'recover_6.npz')}
    recover.main(argv)
    for n, data in first.items():
        assert open(os.path.join(run, n), 'rb').read() == data, n
    # the feature term through the command line, replayed from a graph
    recover.main([gen_pt, 'sndcgan', '--synthetic', '--n', '4', '--steps', '3', '--rows', '0', '--seed', '7', '--lambda_feat', '1',
                  '--dis', dis_pt, '--graph'])
    with np.load(os.path.join(run, 'recover_7.npz')) as z:
        assert z['z'].shape == (4, 128) and (z['feat'] > 0).all()
    assert not os.path.exists(os.path.join(run, 'recover_7.png'))
    with pytest.raises(ValueError, match='--dis'):
        recover.main([gen_pt, 'sndcgan', '--synthetic', '--n', '4', '--lambda_feat', '1'])
