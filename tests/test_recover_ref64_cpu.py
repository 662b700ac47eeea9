"""The float64 yardstick of latent recovery (tests/recover_ref64.py) against float64 autograd of the definition, its
statistics against brute force, the host refusals of contrad_amd/recover.py and the -EINVAL cases of the three entry
points, and the condition of the trajectory case of test_recover_gpu.py.  No GPU."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import cddls_ref64 as R
import cddls_snresnet_ref64 as RS
import recover_ref64 as V
from conftest import ROOT

TOL = 1e-3          # test_recover_gpu.py's same-region tolerance


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope='module')
def nets16():
    return R.fixture_networks(16)


@pytest.fixture(scope='module')
def nets32():
    return R.fixture_networks(32)


# ---- the yardstick against autograd of the definition ----
def _autograd_gz(gsd, z, target, hw, lam, dsd, d_type):
    z = z.clone().requires_grad_()
    pix, feat, loss = V.definition_loss(gsd, z, target, hw, lam, dsd, d_type)
    g, = torch.autograd.grad(loss.sum(), z)
    return g, pix.detach(), feat.detach(), loss.detach()


@pytest.mark.parametrize('lam,d_type', [(0.0, None), (V.LAMBDA_FEAT, 'sndcgan'), (V.LAMBDA_FEAT, 'snresnet18')])
def test_the_forms_give_the_gradient_of_the_definition(nets16, lam, d_type):
    hw = 32 if d_type == 'snresnet18' else 16
    gsd, dsd = RS.fixture_networks() if d_type == 'snresnet18' else nets16
    z0, target = V.case(2, hw, 11)
    z, t = z0.double(), target.double()
    out = V.recovery_step(gsd, z, torch.zeros_like(z), torch.zeros_like(z), t, 0, V.LR, V.BETAS, V.ADAM_EPS, hw, lam, dsd, d_type)
    g, pix, feat, loss = _autograd_gz(gsd, z, t, hw, lam, dsd, d_type)
    assert float(g.abs().max()) > 0
    assert rel_l2(out['g_z'], g) <= 1e-12
    for a, b in ((out['pix'], pix), (out['feat'], feat), (out['loss'], loss)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert (lam == 0) == (float(out['feat'].abs().max()) == 0.0)
    if lam:             # the feature term carries weight in the gradient: dropping it would show
        g0, _, _, _ = _autograd_gz(gsd, z, t, hw, 0.0, None, None)
        share = rel_l2(g0, g)
        want = {'sndcgan': 0.2666, 'snresnet18': 0.9822}[d_type]         # float64 on fixed inputs: the figures DESIGN.md quotes
        assert abs(share - want) < 0.01 * want, (d_type, share)


def test_adam_form_is_adam_with_the_clamp():
    g = torch.Generator().manual_seed(5)
    z, gr = torch.rand(64, generator=g).double() * 2 - 1, (torch.randn(64, generator=g) * 1e-3).double()
    m, v = torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    p = z.clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=0.01, betas=(0.5, 0.75), eps=1e-4)
    for step in range(3):
        z, m, v = V.adam_form(z, gr, m, v, 0.01, (0.5, 0.75), 1e-4, step)
        p.grad = gr.clone()
        opt.step()
        # the betas 0.5 / 0.75 are float32 numbers; lr and eps are not, and the corrections are rounded to float32
        assert float((z - p.detach().clamp(-1, 1)).abs().max()) < 1e-7
    c1, c2 = V.bias_corrections((0.9, 0.999), 0)
    assert c1 == float(np.float32(1.0 - float(np.float32(0.9)))) and abs(c2 - 1e-3) < 1e-6
    # zero gradient on zero moments: z is bitwise what it was
    z0 = torch.rand(16, generator=g) * 2 - 1
    z1, _, _ = V.adam_form(z0, torch.zeros(16), torch.zeros(16), torch.zeros(16), 0.3, (0.7, 0.95), 1e-8, 0)
    assert torch.equal(z0, z1)


# ---- the statistics ----
def test_auc_is_the_pair_count_with_ties():
    from contrad_amd import recover
    rng = np.random.RandomState(3)
    for n, m, levels in ((1, 1, 2), (7, 5, 3), (40, 33, 6), (25, 60, 1000)):
        a, b = rng.randint(0, levels, n) / 8.0, rng.randint(0, levels, m) / 8.0 + (0.125 if levels == 6 else 0.0)
        auc, z = recover.auc_train_below_test(a, b)
        assert abs(auc - V.auc_brute(list(a), list(b))) < 1e-12
        assert abs(z - V.z_score(list(a), list(b))) < 1e-9
    assert recover.auc_train_below_test([1.0, 2.0], [3.0, 4.0]) [0] == 1.0
    assert recover.auc_train_below_test([3.0], [3.0]) == (0.5, 0.0)


def test_statistics_against_the_restatement():
    from contrad_amd import recover
    rng = np.random.RandomState(4)
    tr, te = rng.rand(101) * 0.02, rng.rand(57) * 0.03
    out = recover.statistics(tr, te)
    for name, p in (('train', tr), ('test', te)):
        ref = V.split_stats(p)
        assert set(out[name]) == set(ref) == {'n', 'mean', 'median', 'p10', 'p90', 'psnr_median'}
        for k in ref:
            assert abs(out[name][k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (name, k)
    mt, mr = V.split_stats(te)['median'], V.split_stats(tr)['median']
    assert abs(out['median_gap'] - (mt - mr) / mt) < 1e-12
    assert abs(out['auc'] - V.auc_brute(list(tr), list(te))) < 1e-12
    assert 'no sign of memorisation' in out['note'] and 'equal settings' in out['note']
    alone = recover.statistics(tr)
    assert set(alone) == {'train', 'note'}


# ---- refusals ----
def _cpu_networks(arch='sndcgan', hw=32):
    from contrad_amd.models.gan import get_architecture
    G, D = get_architecture(arch, (hw, hw, 3))
    return G.eval(), D.eval()


def test_host_refusals_touch_no_gpu(tmp_path):
    from contrad_amd import recover
    was = torch.cuda.is_initialized()
    G, D = _cpu_networks()
    with pytest.raises(NotImplementedError, match='sndcgan'):
        recover.LatentRecovery(torch.nn.Linear(2, 2).eval(), 4)
    with pytest.raises(NotImplementedError, match='sndcgan'):
        recover.LatentRecovery(G, 4, D=torch.nn.Linear(2, 2).eval(), lambda_feat=1.0)
    with pytest.raises(ValueError, match='needs D'):
        recover.LatentRecovery(G, 4, lambda_feat=1.0)
    G.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        recover.LatentRecovery(G, 4)
    G.eval(); D.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        recover.LatentRecovery(G, 4, D=D, lambda_feat=1.0)
    D.eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        recover.LatentRecovery(G, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        recover.LatentRecovery(G, 4, D=D, lambda_feat=1.0)
    G16, _ = _cpu_networks('sndcgan', 16)
    _, DR = _cpu_networks('snresnet18', 32)
    with pytest.raises(NotImplementedError, match='32x32'):
        recover.LatentRecovery(G16, 4, D=DR, lambda_feat=1.0)
    with pytest.raises(ValueError):
        recover.LatentRecovery(G, 4, lr=-1.0)

    # the command line: every argument refusal before any CUDA call
    run = tmp_path / 'run'
    run.mkdir()
    shutil.copy(os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin'), str(run / 'c10_b64.gin'))
    gen = str(run / 'gen.pt')
    rng = np.random.RandomState(0)
    np.savez(str(tmp_path / 'set.npz'), x_train=rng.randint(0, 255, (4, 32, 32, 3)).astype(np.uint8))
    data = ['--data', str(tmp_path / 'set.npz')]
    with pytest.raises(ValueError, match='--dis'):
        recover.main([gen, 'sndcgan', '--lambda_feat', '1'] + data)
    with pytest.raises(ValueError, match='--steps'):
        recover.main([gen, 'sndcgan', '--steps', '0'] + data)
    with pytest.raises(ValueError, match='beyond the 4 images'):
        recover.main([gen, 'sndcgan', '--n', '8'] + data)
    with pytest.raises(ValueError, match='x_test'):
        recover.main([gen, 'sndcgan', '--n', '2', '--holdout'] + data)
    with pytest.raises(NotImplementedError, match='sndcgan'):
        recover.main([gen, 'stylegan2', '--n', '2'] + data)
    assert torch.cuda.is_initialized() == was


@pytest.fixture(scope='module')
def built():
    from contrad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_without_gpu(built):
    """-EINVAL before any GPU call, on host pointers."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    LL = ctypes.c_longlong
    fn = built.raw('contrad_cddls_recover_loss')
    #       gout target phi phi* resid pix feat loss N  F  P      lambda stream
    good = [p, p, p, p, p, p, p, p, 2, 4, LL(8), 1.0, None]
    for i, bad in ((0, None), (1, None), (5, None), (6, None), (7, None), (8, 0), (10, LL(0)), (3, None), (4, None), (9, 0)):
        args = list(good)
        args[i] = bad
        assert fn(*args) == -22, ('loss', i)
    for phi_t, resid in ((p, None), (None, p), (p, p)):          # a target or residual pointer without the feature pointer
        assert fn(p, p, None, phi_t, resid, p, p, p, 2, 4, LL(8), 1.0, None) == -22
    fn = built.raw('contrad_cddls_recover_image_end')
    good = [p, p, p, p, LL(8), LL(4), None]
    for i, bad in ((1, None), (2, None), (3, None), (4, LL(0)), (5, LL(0))):
        args = list(good)
        args[i] = bad
        assert fn(*args) == -22, ('image_end', i)
    fn = built.raw('contrad_cddls_recover_update')
    good = [p, p, p, p, LL(8), 0.1, 0.9, 0.999, 1e-8, p, None]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (9, None), (4, LL(0)), (5, -0.1), (6, 1.0), (6, -0.1), (7, 1.0),
                   (8, -1.0)):
        args = list(good)
        args[i] = bad
        assert fn(*args) == -22, ('update', i)


# ---- the condition of the GPU trajectory case ----
def test_the_trajectory_case_is_well_conditioned(nets32):
    """On the trajectory inputs a float32 torch-CPU run of the same arithmetic stays within TOL / 2 of the float64 run on
    the increments of z (both on the float64 run's own regions): the acceptance habit of the gp step's fixture.  adam_eps
    is the float64 median |g_z| of the first step."""
    gsd, _ = nets32
    z0, target, eps = V.trajectory_case(gsd)
    assert eps > 0
    z = z0.double()
    regions = []
    m = v = torch.zeros_like(z)
    for i in range(V.TRAJ_STEPS):                       # the float64 run's own regions, step by step
        regions.append({'g': V.g_region(gsd, z, 32), 'd': []})
        out = V.recovery_step(gsd, z, m, v, target.double(), i, V.LR, V.BETAS, eps, region=regions[-1])
        z, m, v = out['z'], out['m'], out['v']
    s64, pix64 = V.trajectory(gsd, z0.double(), target.double(), V.TRAJ_STEPS, V.LR, V.BETAS, eps, regions=regions)
    free, _ = V.trajectory(gsd, z0.double(), target.double(), V.TRAJ_STEPS, V.LR, V.BETAS, eps)
    gsd32 = {k: t.float() for k, t in gsd.items()}
    s32, pix32 = V.trajectory(gsd32, z0, target, V.TRAJ_STEPS, V.LR, V.BETAS, eps, regions=regions)
    for a, b, c in zip(s32, s64, free):
        assert a['z'].dtype == torch.float32
        assert torch.equal(b['z'], c['z'])               # imposing its own regions changes nothing
        d64 = b['z'] - b['z_prev']
        assert float(d64.abs().max()) > 0.01             # the increments are not noise
        assert rel_l2(a['z'] - a['z_prev'], d64) <= TOL / 2
        interior = (b['z'].abs() < 1).double().mean()
        assert float(interior) > 0.5                     # most entries move freely; some may sit in the clamp
    assert rel_l2(pix32, pix64) <= TOL / 2
