"""cDDLS sampling with D_SNResNet18 without a GPU: the float64 yardstick (tests/cddls_snresnet_ref64.py) against the
reference's own ``_sample_cddls`` on its snresnet18 pair (tests/golden/cddls_snresnet18.npz), the conditions the GPU
comparisons rest on, the restated forms of the join kernel, the two new C entry points' argument checks, the host refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cddls_snresnet_ref64 as RS
from conftest import GOLDEN


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'cddls_snresnet18.npz'))


@pytest.fixture(scope='module')
def nets():
    return RS.fixture_networks()


@pytest.fixture(scope='module')
def trajectories(fx, nets):
    return {int(y): RS.ref_trajectory(fx, int(y), nets=nets) for y in fx['classes']}


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize('y', [3, 7])
def test_yardstick_reproduces_reference(fx, trajectories, y):
    """Increments, not states (the states are dominated by z0), to relative 1e-10: the bound of test_cddls_ref64_cpu.py."""
    steps, images = trajectories[y]
    zs, prev = torch.from_numpy(fx['y%d.z' % y]), t64(fx['z0'])
    s_ref = torch.from_numpy(fx['y%d.z2_sums' % y])
    for k, st in enumerate(steps):
        assert relmax(st['z'] - st['z_prev'], zs[k] - prev) < 1e-10, k
        prev = zs[k]
        assert abs(st['e'].sum().item() - fx['y%d.e_sum' % y][k]) < 1e-10 * abs(fx['y%d.e_sum' % y][k])
        assert relmax(st['z2'].reshape(4, -1).sum(1) - st['z2_prev'].reshape(4, -1).sum(1), s_ref[k + 1] - s_ref[k]) < 1e-10
    z2_first = t64(fx['z2_0'])
    assert relmax(steps[-1]['z2'] - z2_first, torch.from_numpy(fx['y%d.z2_last' % y]) - z2_first) < 1e-10
    assert relmax(images, torch.from_numpy(fx['y%d.images' % y])) < 1e-10
    assert os.path.getsize(os.path.join(GOLDEN, 'cddls_snresnet18.npz')) < os.path.getsize(os.path.join(GOLDEN, 'cddls.npz'))


@pytest.mark.parametrize('y', [3, 7])
def test_fixture_checks_gradient_and_noise_alike(trajectories, y):
    """At every step the drift 0.5 eps g_z and the noise sigma_n sqrt(eps) n are within a factor 10 of each other, and no
    entry of z sits on the clamp: an increment comparison sees both terms, undistorted."""
    for st in trajectories[y][0]:
        ratio = float(st['drift'].norm() / st['noise'].norm())
        assert 0.1 < ratio < 10.0, ratio
        assert int((st['z'].abs() == 1).sum()) == 0


def test_classes_differ(trajectories):
    """The class row reaches z: the two classes' drifts are not the same vector (relative difference far above round-off)."""
    a, b = trajectories[3][0][0]['g_z'], trajectories[7][0][0]['g_z']
    assert float((a - b).norm() / a.norm()) > 1e-2


def test_restated_kernel_forms_equal_a_loop():
    g = torch.Generator().manual_seed(5)
    N, T, C = 3, 4, 8
    h, c = torch.randn(N, C, generator=g), torch.randn(C, generator=g)
    act = torch.randn(N, T, C, generator=g)
    act[0, 0, 0], act[1, 2, 3] = 0.0, -0.0
    out = RS.pooled_form(h, c, act)
    inv_t = float(np.float32(1.0) / np.float32(T))
    for n in range(N):
        for t in range(T):
            for k in range(C):
                d = 1.0 if float(act[n, t, k]) > 0 else RS.SLOPE
                assert float(out[n, t, k]) == ((float(h[n, k]) + float(c[k])) * inv_t) * d
    assert float(out[0, 0, 0]) == ((float(h[0, 0]) + float(c[0])) * inv_t) * RS.SLOPE           # zero: region `slope`
    a, b, x = torch.randn(24, generator=g), torch.randn(24, generator=g), torch.randn(24, generator=g)
    x[5] = 0.0
    out = RS.join_form(a, b, x)
    for i in range(24):
        assert float(out[i]) == (float(a[i]) + float(b[i])) * (1.0 if float(x[i]) > 0 else RS.SLOPE)
    gh, a2 = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    out = RS.seed_form(gh, c, a2)
    for n in range(N):
        for k in range(C):
            assert float(out[n, k]) == (float(gh[n, k]) + float(c[k])) * (1.0 if float(a2[n, k]) > 0 else RS.SLOPE)
    assert torch.equal(RS.pooled_form(gh, c, a2.view(N, 1, C)).view(N, C), out)                  # T = 1 is the seed form


def test_imposing_own_regions_changes_nothing(fx, nets, trajectories):
    gsd, dsd = nets
    W, b = RS.fixture_head(fx)
    st = trajectories[3][0][0]
    region = RS.own_region(gsd, dsd, st['z_prev'], st['z2_prev'], float(fx['eps']))
    assert len(region['g']) == 4 and len(region['d']) == 17 and tuple(region['hidden'].shape) == (4, 1024)
    again = RS.langevin_step(gsd, dsd, W[3], b[3], st['z_prev'], st['z2_prev'], t64(fx['n'][0]), t64(fx['n2'][0]),
                             float(fx['eps']), float(fx['lbd']), float(fx['sigma_n']), region=region)
    for key in ('z', 'z2', 'g_z', 'g_x', 'e', 'd', 'f'):
        assert relmax(again[key], st[key]) < 1e-12, key


def _images_of(gsd, z, z2, eps):
    with torch.no_grad():
        return RS.R.g_eval_forward(gsd, z, 32) + eps * z2


def test_same_region_comparisons_are_well_conditioned(fx, nets, trajectories):
    """In the float64 runs of the fixture and of the GPU tests' one-step and D-half cases, per layer at most 1e-4 of the
    pre-activations lie within 1e-5 of the layer's largest magnitude of zero: only those can change region in float32."""
    gsd, dsd = nets
    batches = []
    for y in (3, 7):
        batches += [_images_of(gsd, st['z_prev'], st['z2_prev'], float(fx['eps'])) for st in trajectories[y][0]]
    for N in RS.STEP_SIZES:
        W, b, z0, z2_0, n, n2 = RS.one_step_case(N)
        batches.append(_images_of(gsd, z0.double(), z2_0.double(), RS.EPS))
    batches.append(RS.d_half_case()[1].double())
    for x in batches:
        shares = RS.near_zero_share(RS.preactivations(dsd, x))
        assert len(shares) == 18 and max(shares) <= RS.NEAR_ZERO_SHARE, shares


def _aligned(n):
    buf = np.zeros(n + 8, np.float32)
    off = (-buf.ctypes.data % 16) // 4
    v = buf[off:off + n]
    assert v.ctypes.data % 16 == 0
    return v


def test_new_entry_points_refuse_bad_arguments_before_any_gpu_call():
    from contrad_amd._lib import lib
    was = torch.cuda.is_initialized()
    pooled, join = lib().raw('contrad_cddls_pooled_seed'), lib().raw('contrad_cddls_join_bwd')
    N, T, C = 2, 4, 8
    g, c, act, out = _aligned(N * C + 4), _aligned(C + 4), _aligned(N * T * C + 4), _aligned(N * T * C + 4)

    def p(a, shift=0):
        return ctypes.c_void_p(a.ctypes.data + 4 * shift)
    LL = ctypes.c_longlong
    good = [p(g), p(c), p(act), p(out)]
    for i in range(4):                                              # a null pointer, a misaligned pointer
        for bad in (ctypes.c_void_p(0), p([g, c, act, out][i], 1)):
            args = list(good)
            args[i] = bad
            assert pooled(*args, LL(N), T, C, 0.1, None) == -22, i
    assert pooled(p(g), p(c), p(act), p(g), LL(N), 1, C, 0.1, None) == -22           # not in place: g and out differ in shape
    for n_, t_, c_ in ((0, T, C), (-1, T, C), (N, 0, C), (N, T, 0), (N, T, 2), (N, T, 6), (N, T, 9)):
        assert pooled(*good, LL(n_), t_, c_, 0.1, None) == -22, (n_, t_, c_)
    n = 16
    a, b, x, o = _aligned(n + 4), _aligned(n + 4), _aligned(n + 4), _aligned(n + 4)
    good = [p(a), p(b), p(x), p(o)]
    for i in range(4):
        for bad in (ctypes.c_void_p(0), p([a, b, x, o][i], 1)):
            args = list(good)
            args[i] = bad
            assert join(*args, LL(n), 0.1, None) == -22, i
    for n_ in (0, -4, 3, 6, 17):
        assert join(*good, LL(n_), 0.1, None) == -22, n_
    assert torch.cuda.is_initialized() == was


def test_host_refusals():
    """Raised from host state alone (the modules stay on the CPU): a D in train mode, a head of another width, stylegan2."""
    from contrad_amd import cddls
    from contrad_amd.models.gan import get_architecture
    was = torch.cuda.is_initialized()
    G, D = get_architecture('snresnet18', (32, 32, 3))
    W, b = torch.zeros(10, 512), torch.zeros(10)
    G.eval(); D.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        cddls.CDDLSSampler(G, D, W, b, 4)
    D.eval()
    with pytest.raises(RuntimeError, match='reads 8192 features, D has 512'):
        cddls.CDDLSSampler(G, D, torch.zeros(10, 8192), b, 4)
    assert cddls.IMPLEMENTED == ('sndcgan', 'snresnet18')
    with pytest.raises(NotImplementedError, match='sndcgan'):
        cddls.main(['logdir', 'lin.pth.tar', 'stylegan2', '--n_samples', '2'])
    assert torch.cuda.is_initialized() == was
