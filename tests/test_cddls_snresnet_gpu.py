"""cDDLS sampling with D_SNResNet18 on the GPU (contrad_amd/cddls.py's snresnet18 D half, the pooled-seed and join forms
of cddls_feature_seed_kernel): the two forms alone against float64, the D half alone, one Langevin step and the three-step
trajectory of tests/golden/cddls_snresnet18.npz against tests/cddls_snresnet_ref64.py, the sampler's invariants, the CLI.

Tolerances: those of tests/test_cddls_gpu.py (each recorded through ``margin``).
  kernels   abs 1e-5: every output is one fp32 sum and at most two fp32 products of magnitude <= ~6 (a few ulp there)
  D half / step / trajectory   rel L2 1e-3 on the sampler's own linear region, 1e-2 raw
"""
import os
import shutil

import numpy as np
import pytest
import torch

import cddls_snresnet_ref64 as RS
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL, FLIP_TOL, KTOL = 1e-3, 1e-2, 1e-5
EPS, SIGMA_N, LBD = RS.EPS, RS.SIGMA_N, RS.LBD
GUARD = 64                   # floats of NaN on either side of an output


def dev():
    return torch.device('cuda', 0)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def maxabs(a, b):
    return float((a.detach().double().cpu().reshape(-1) - b.detach().double().cpu().reshape(-1)).abs().max())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(n):
    """(whole buffer, 16-byte aligned view of n floats with GUARD NaNs on either side)."""
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev())
    v = buf[GUARD:GUARD + n]
    assert v.data_ptr() % 16 == 0
    return buf, v


def guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def with_zeros(act):
    """Exact zeros and negative zeros among the activations: both belong to the region `slope`."""
    flat = act.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    return act


# ---------------------------------------------------------------------------------------------------------
# the two new forms of the kernel alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,T,C', [(1, 16, 512), (3, 16, 512), (5, 1, 4), (2, 4, 8), (7, 16, 64)])
def test_pooled_seed(margin, N, T, C):
    from contrad_amd import ops
    g = gen(N * 1000 + T * 10 + C)
    h, c = torch.randn(N, C, generator=g), -LBD * 0.5 * torch.randn(C, generator=g)
    act = with_zeros(torch.randn(N, T, C, generator=g))
    ref = RS.pooled_form(h, c, act)
    buf, out = guarded(N * T * C)
    ops.cddls_pooled_seed(h.to(dev()), c.to(dev()), act.to(dev()), 0.1, out=out)
    margin('cddls pooled_seed N=%d T=%d C=%d' % (N, T, C), maxabs(out, ref), KTOL)
    assert guards_intact(buf, N * T * C)
    zero = (act == 0).view(-1)
    assert bool(zero.any()) and maxabs(out.cpu()[zero], ref.view(-1)[zero]) < KTOL
    fresh = ops.cddls_pooled_seed(h.to(dev()), c.to(dev()), act.to(dev()), 0.1)          # its own allocation
    assert tuple(fresh.shape) == (N, T, C) and torch.equal(fresh.view(-1), out)


@pytest.mark.parametrize('n', [4, 3 * 16 * 16 * 64, 33 * 32 * 32 * 64])
def test_join_bwd(margin, n):
    """The last size is 540 672 quads: more than one pass of the 2048 x 256-thread grid."""
    from contrad_amd import ops
    g = gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    act = with_zeros(torch.randn(n, generator=g))
    ref = RS.join_form(a, b, act)
    buf, out = guarded(n)
    ad, bd, xd = a.to(dev()), b.to(dev()), act.to(dev())
    ops.cddls_join_bwd(ad, bd, xd, 0.1, out=out)
    margin('cddls join_bwd n=%d' % n, maxabs(out, ref), KTOL)
    assert guards_intact(buf, n)
    assert float(act[0]) == 0.0 and float(out[0]) == float((a[0] + b[0]) * torch.tensor(0.1))      # zero: region `slope`
    ibuf, inplace = guarded(n)                             # in place on the first operand, as the sampler calls it
    inplace.copy_(ad)
    ops.cddls_join_bwd(inplace, bd, xd, 0.1, out=inplace)
    assert torch.equal(inplace, out) and guards_intact(ibuf, n)


def test_feature_seed_is_the_pooled_form_at_one_pixel():
    from contrad_amd import ops
    g = gen(58192)
    gh, a = torch.randn(5, 8192, generator=g).to(dev()), with_zeros(torch.randn(5, 8192, generator=g)).to(dev())
    c = (-LBD * 0.5 * torch.randn(8192, generator=g)).to(dev())
    seed = ops.cddls_feature_seed(gh, c, a, 0.1)
    pooled = ops.cddls_pooled_seed(gh, c, a.view(5, 1, 8192), 0.1)
    assert torch.equal(seed, pooled.view(5, 8192))
    assert maxabs(seed, RS.seed_form(gh.cpu(), c.cpu(), a.cpu())) < KTOL


# ---------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nets():
    """Fixture networks: float64 state dicts on the host, the float32 modules in eval mode on the device."""
    from contrad_amd.models.gan import get_architecture
    gsd, dsd = RS.fixture_networks()
    G, D = get_architecture('snresnet18', (32, 32, 3))
    full = dict(G.state_dict())
    full.update({k: v.float() for k, v in gsd.items()})
    G.load_state_dict(full)
    D.load_state_dict({k: v.float() for k, v in dsd.items()})
    G.to(dev()).eval(); D.to(dev()).eval()
    for p in list(G.parameters()) + list(D.parameters()):
        p.requires_grad_(False)
    return gsd, dsd, G, D


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'cddls_snresnet18.npz'))


def cpu_region(region):
    return {'g': [m.cpu() for m in region['g']], 'd': [m.cpu() for m in region['d']], 'hidden': region['hidden'].cpu()}


def test_d_half_alone(margin, nets):
    """Logit, pooled features and g_x of one forward + backward of the D half on given images."""
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = nets
    W, x = RS.d_half_case()
    N, y = RS.DHALF_N, RS.STEP_CLASS
    S = CDDLSSampler(G, D, W.to(dev()), torch.zeros(10, device=dev()), N, lbd=LBD)
    S.set_class(y)
    with torch.no_grad():
        S.x.copy_(x)
        S._d_forward()
        S._d_backward()
    region = cpu_region(S.linear_region())
    assert len(region['d']) == 17 and tuple(region['d'][0].shape) == (N, 64, 32, 32) and tuple(region['d'][-1].shape) == (N, 512, 4, 4)
    same, raw = RS.d_half(dsd, W[y].double(), x.double(), LBD, region=region), RS.d_half(dsd, W[y].double(), x.double(), LBD)
    for name, ref, tol in (('same region', same, TOL), ('raw', raw, FLIP_TOL)):
        margin('cddls snresnet18 D half logit ' + name, rel_l2(S.logits.view(N, 1), ref[0]), tol)
        margin('cddls snresnet18 D half features ' + name, rel_l2(S.d_feats, ref[1]), tol)
        margin('cddls snresnet18 D half g_x ' + name, rel_l2(S.g_x, ref[2]), tol)


@pytest.mark.parametrize('N', RS.STEP_SIZES)
def test_one_step(margin, nets, N):
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = nets
    W, b, z0, z2_0, n, n2 = RS.one_step_case(N)
    y = RS.STEP_CLASS
    S = CDDLSSampler(G, D, W.to(dev()), b.to(dev()), N, lbd=LBD, eps=EPS, sigma_n=SIGMA_N, energy=True)
    S.set_class(y)
    S.start(z0.to(dev()), z2=z2_0.to(dev()))
    S.step(noise=n.to(dev()), noise2=n2.to(dev()))
    region = cpu_region(S.linear_region())
    args = (gsd, dsd, W[y].double(), b[y].double(), z0.double(), z2_0.double(), n.double(), n2.double(), EPS, LBD, SIGMA_N)
    same, raw = RS.langevin_step(*args, region=region), RS.langevin_step(*args)
    tag = 'cddls snresnet18 step N=%d ' % N
    e = S.energy.double().cpu()
    margin(tag + 'g_z same region', rel_l2(S.g_z, same['g_z']), TOL)
    margin(tag + 'g_x same region', rel_l2(S.g_x, same['g_x']), TOL)
    margin(tag + 'energy same region', float(((e - same['e']).abs() / same['e'].abs()).max()), TOL)
    margin(tag + 'g_z raw', rel_l2(S.g_z, raw['g_z']), FLIP_TOL)
    margin(tag + 'g_x raw', rel_l2(S.g_x, raw['g_x']), FLIP_TOL)
    margin(tag + 'energy raw', float(((e - raw['e']).abs() / raw['e'].abs()).max()), TOL)
    margin(tag + 'dz same region', rel_l2(S.z.cpu().double() - z0.double(), same['z'] - z0.double()), TOL)
    margin(tag + 'dz2 same region', rel_l2(S.z2.cpu().double() - z2_0.double(), same['z2'] - z2_0.double()), TOL)
    assert int(S.state[0]) == 1 and int(S.state[1]) == 0


@pytest.mark.parametrize('yi', [0, 1])
def test_trajectory_against_reference(margin, nets, fx, yi):
    """Three steps on the reference's recorded draws: increments of z and z2 and the final images against the yardstick on
    the sampler's own linear regions (1e-3) and against the reference's raw run (1e-2); what the raw criterion sees of z2
    is what the fixture stores (tests/test_cddls_gpu.py::test_trajectory_against_reference)."""
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = nets
    y = int(fx['classes'][yi])
    W, b = RS.fixture_head(fx)
    S = CDDLSSampler(G, D, W.float().to(dev()), b.float().to(dev()), 4, lbd=float(fx['lbd']), eps=float(fx['eps']),
                     sigma_n=float(fx['sigma_n']))
    S.set_class(y)
    S.start(torch.from_numpy(fx['z0']).to(dev()), z2=torch.from_numpy(fx['z2_0']).to(dev()))
    zs, z2s, regions = [S.z.cpu().double()], [S.z2.cpu().double()], []
    for k in range(fx['n'].shape[0]):
        S.step(noise=torch.from_numpy(fx['n'][k]).to(dev()), noise2=torch.from_numpy(fx['n2'][k]).to(dev()))
        regions.append(cpu_region(S.linear_region()))
        zs.append(S.z.cpu().double()); z2s.append(S.z2.cpu().double())
    images = S.images().cpu().double()
    steps, ref_images = RS.ref_trajectory(fx, y, regions=regions, nets=(gsd, dsd))
    tag = 'cddls snresnet18 trajectory y=%d ' % y
    fz = [torch.from_numpy(fx['z0'].astype(np.float64))] + [torch.from_numpy(t) for t in fx['y%d.z' % y]]
    fsum = torch.from_numpy(fx['y%d.z2_sums' % y])
    for k, st in enumerate(steps):
        margin(tag + 'dz same region step %d' % k, rel_l2(zs[k + 1] - zs[k], st['z'] - st['z_prev']), TOL)
        margin(tag + 'dz2 same region step %d' % k, rel_l2(z2s[k + 1] - z2s[k], st['z2'] - st['z2_prev']), TOL)
        margin(tag + 'dz raw step %d' % k, rel_l2(zs[k + 1] - zs[k], fz[k + 1] - fz[k]), FLIP_TOL)
        margin(tag + 'd(sum z2) raw step %d' % k,
               rel_l2((z2s[k + 1] - z2s[k]).reshape(4, -1).sum(1), fsum[k + 1] - fsum[k]), FLIP_TOL)
    margin(tag + 'z2 total increment raw', rel_l2(z2s[-1] - z2s[0], torch.from_numpy(fx['y%d.z2_last' % y]) - z2s[0]), FLIP_TOL)
    margin(tag + 'images same region', rel_l2(images, ref_images), TOL)
    margin(tag + 'images raw', rel_l2(images, torch.from_numpy(fx['y%d.images' % y])), FLIP_TOL)


def _run(G, D, W, b, z0, seed, graph, steps=5, y=1, first_step=0):
    from contrad_amd.cddls import CDDLSSampler
    S = CDDLSSampler(G, D, W, b, z0.shape[0], seed=seed, graph=graph)
    S.set_class(y)
    S.start(z0, first_step)
    for _ in range(steps):
        S.step()
    return S, S.z.clone(), S.z2.clone(), S.images()


def _prepared(S):
    return [t.data_ptr() for t in S.d_wps + S.g_wps] + [f.buf.data_ptr() for f in (S.d_filters, S.g_filters) if f and f.buf is not None]


def test_invariants(nets):
    gsd, dsd, G, D = nets
    g = gen(8)
    W, b = (0.05 * torch.randn(10, 512, generator=g)).to(dev()), (0.1 * torch.randn(10, generator=g)).to(dev())
    z0 = (torch.rand(8, 128, generator=g) * 2 - 1).to(dev())
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in (G, D)]
    S, z_a, z2_a, im_a = _run(G, D, W, b, z0, 11, False)
    assert int(S.state[0]) == 5 and bool(torch.isfinite(im_a).all())
    assert len(S.d_wps) == 22                   # stem, 8 x (conv1, conv2), 3 shortcut convs, the two logit-head layers
    for m, sd in zip((G, D), before):           # both state dicts bit-identical: u, v, running statistics, counters
        now = m.state_dict()
        assert list(now) == list(sd) and all(torch.equal(now[k], sd[k]) for k in sd)
    _, z_g, z2_g, im_g = _run(G, D, W, b, z0, 11, True)          # eager first step, capture, replays
    assert torch.equal(z_a, z_g) and torch.equal(z2_a, z2_g) and torch.equal(im_a, im_g)
    _, z_b, z2_b, im_b = _run(G, D, W, b, z0, 11, False)         # same seed: the same bits
    assert torch.equal(z_a, z_b) and torch.equal(z2_a, z2_b) and torch.equal(im_a, im_b)
    _, z_c, z2_c, _ = _run(G, D, W, b, z0, 12, False)            # another seed
    assert not torch.equal(z_a, z_c) and not torch.equal(z2_a, z2_c)
    _, z_d, z2_d, _ = _run(G, D, W, b, z0, 11, False, first_step=6)      # another step range of the same seed
    assert not torch.equal(z_a, z_d) and not torch.equal(z2_a, z2_d)
    # a second class on the same sampler reuses everything prepared
    ptrs, c_before = _prepared(S), S.c_row.clone()
    S.set_class(2); S.start(z0); S.step()
    assert ptrs == _prepared(S)
    assert not torch.equal(S.c_row, c_before)
    assert torch.equal(S.c_row, W[2] * -1.0)                     # pooled features: the row as it comes, no permutation


def test_cli(tmp_path):
    from contrad_amd import cddls, lineval
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(3)
    G, D = get_architecture('snresnet18', (32, 32, 3))
    G.to(dev()); D.to(dev())
    with torch.no_grad():           # fresh modules carry random u, v: a few train-mode passes make them what a checkpoint holds
        D.train()
        for _ in range(5):
            D(torch.rand(4, 3, 32, 32, device=dev()))
    logdir = tmp_path / 'run'
    logdir.mkdir()
    torch.save({k: v.cpu() for k, v in G.state_dict().items()}, str(logdir / 'gen_best.pt'))
    torch.save({k: v.cpu() for k, v in D.state_dict().items()}, str(logdir / 'dis_best.pt'))
    shutil.copy(os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin'), str(logdir / 'c10_b64.gin'))
    head = lineval.install_head(D, 2)
    assert tuple(head.weight.shape) == (2, 512)
    lin = str(logdir / 'lin_eval_1.pth.tar')
    lineval.save_checkpoint(D, 1, lin)
    argv = [str(logdir), lin, 'snresnet18', '--n_samples', '12', '--n_classes', '2', '--batch_size', '4', '--n_steps', '3']
    out = cddls.main(argv + ['--seed', '1', '--log_energy'])
    assert os.path.basename(out) == 'samples_cDDLS_1'
    assert sorted(os.listdir(os.path.join(out, '0'))) == sorted('%d.png' % i for i in range(6))
    assert sorted(os.listdir(os.path.join(out, '1'))) == sorted('%d.png' % i for i in range(6, 12))
    with np.load(os.path.join(out, 'samples.npz')) as z:
        assert z['images'].shape == (12, 32, 32, 3) and z['images'].dtype == np.uint8
        assert z['labels'].tolist() == [0] * 6 + [1] * 6
        assert z['images'].min() >= 0 and z['images'].max() <= 255 and z['images'].std() > 0
    data = open(os.path.join(out, '0', '0.png'), 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and len(data) > 100
    pngs = {(c, f): open(os.path.join(out, c, f), 'rb').read() for c in ('0', '1') for f in os.listdir(os.path.join(out, c))}
    shutil.rmtree(out)
    out2 = cddls.main(argv + ['--seed', '1', '--graph'])            # the same seed replayed from a captured graph
    assert out2 == out
    assert pngs == {(c, f): open(os.path.join(out2, c, f), 'rb').read() for c in ('0', '1') for f in os.listdir(os.path.join(out2, c))}
    with pytest.raises(RuntimeError, match=r'linear.weight is \(2, 512\), expected \(3, 512\)'):
        cddls.main(argv[:5] + ['--n_classes', '3', '--batch_size', '4', '--n_steps', '1', '--seed', '1'])
    with pytest.raises(NotImplementedError, match='sndcgan'):
        cddls.main([str(logdir), lin, 'stylegan2', '--n_samples', '2'])
