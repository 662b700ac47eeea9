"""cDDLS sampling on the GPU (contrad_amd/cddls.py, csrc/cddls.hip): every new kernel alone against float64 with
explicit noise, the generator against the numpy Philox / float64 Box-Muller, one Langevin step and the three-step
trajectory of tests/golden/cddls.npz against tests/cddls_ref64.py, the sampler's invariants, the CLI.

Tolerances (each recorded through ``margin``):
  kernels      abs 1e-5: every output is a sum of at most four fp32 products of magnitude <= ~6 (8 ulp there)
  normals      abs 1.6e-5 against float64 Box-Muller of the same words: 32 ulp at 5.9, the largest draw
  energy       |err| < 1e-5 * (sum of |terms|): <= 8192 + 3072 fp32 terms per sample, summed over 256 lanes then a tree
  step         rel L2 1e-3 on the same linear region (TOL of test_gstep_gpu.py / test_sndcgan_gpu.py), 1e-2 raw (FLIP_TOL)
"""
import os
import shutil

import numpy as np
import pytest
import torch

import cddls_ref64 as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL, FLIP_TOL, KTOL = 1e-3, 1e-2, 1e-5
EPS, SIGMA_N, LBD = 0.5, 0.7, 2.5          # far from the defaults: a dropped or mis-scaled term cannot hide
SIZES = [(1, 32), (3, 16), (5, 32)]


def dev():
    return torch.device('cuda', 0)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def unaligned(t):
    """A device copy of ``t`` (flat) that starts 4 bytes past a 16-byte boundary: the kernels' scalar form."""
    buf = torch.empty(t.numel() + 1, device=dev())
    v = buf[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------
# kernels alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,hw', SIZES)
def test_feature_seed(margin, N, hw):
    from contrad_amd import ops
    F = 512 * (hw // 8) ** 2
    g = gen(N)
    gh, a = torch.randn(N, F, generator=g), torch.randn(N, F, generator=g)
    c = -LBD * 0.5 * torch.randn(F, generator=g)
    ref = (gh.double() + c.double()) * torch.where(a > 0, 1.0, 0.1).double()
    out = ops.cddls_feature_seed(gh.to(dev()), c.to(dev()), a.to(dev()), 0.1)
    margin('cddls feature_seed N=%d F=%d' % (N, F), maxabs(out, ref), KTOL)
    buf = gh.to(dev())                                       # in place, as the sampler calls it
    ops.cddls_feature_seed(buf, c.to(dev()), a.to(dev()), 0.1, out=buf)
    assert torch.equal(buf, out)


@pytest.mark.parametrize('M,K,ld,perm', [(3 * 16 * 16, 128, 128, 1), (5, 8192, 8192, 16), (3, 2048, 2048, 4),
                                         (7, 6, 7, 1), (33, 64, 66, 1), (2000, 64, 64, 1)])
def test_bn_relu_bwd_eval(margin, M, K, ld, perm):
    """(M, K) row matrices with row stride ld: the vector form, the permuted form of norm_init (feature rows 8192 / 2048),
    a stride that is no multiple of 4, more than one block."""
    from contrad_amd import ops
    g = gen(M + K)
    dy, y = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)       # in x's column order
    gamma, var = 1 + 0.3 * torch.randn(K, generator=g), 0.5 + torch.rand(K, generator=g)
    ref = dy.double() * (y > 0).double() * (gamma.double() / torch.sqrt(var.double() + 1e-5))

    def lay(t):             # the layout bn_relu_apply wrote: column ch * perm + hw at hw * (K / perm) + ch
        return t.view(M, K // perm, perm).permute(0, 2, 1).reshape(M, K) if perm > 1 else t

    def strided(t):
        buf = torch.zeros(M, ld, device=dev())
        buf[:, :K] = t
        return buf[:, :K]
    dyd, yd, dx = strided(lay(dy)), strided(lay(y)), strided(torch.zeros(M, K))
    ops.bn_relu_bwd_eval(dyd, yd, dx, gamma.to(dev()), var.to(dev()), 1e-5, perm)
    margin('cddls bn_relu_bwd_eval M=%d K=%d ld=%d perm=%d' % (M, K, ld, perm), maxabs(dx, ref), KTOL)
    if perm == 1:           # in place, as the sampler calls it
        ops.bn_relu_bwd_eval(dyd, yd, dyd, gamma.to(dev()), var.to(dev()), 1e-5, 1)
        assert torch.equal(dyd, dx)
        assert ld == K or float(dyd.as_strided((M, ld - K), (ld, 1), dyd.storage_offset() + K).abs().max()) == 0.0


@pytest.mark.parametrize('n,aligned', [(1 * 3 * 32 * 32, True), (3 * 3 * 16 * 16, True), (5 * 3 * 32 * 32, True), (1, True),
                                       (7, True), (4096 + 3, True), (4096 + 3, False), (300 * 3072 + 1, True)])
def test_compose_and_image_end(margin, n, aligned):
    from contrad_amd import ops
    g = gen(n)
    gout, z2, gx, nz = torch.rand(n, generator=g), torch.randn(n, generator=g), 4 * torch.randn(n, generator=g), \
        torch.randn(n, generator=g)
    put = (lambda t: t.to(dev())) if aligned else unaligned
    x = ops.cddls_compose(put(gout), put(z2), EPS, out=put(torch.zeros(n)))
    margin('cddls compose n=%d' % n, maxabs(x, gout.double() + EPS * z2.double()), KTOL)
    xc = ops.cddls_compose(put(gout), put(3 * z2), EPS, out=put(torch.zeros(n)), clamp01=True)
    refc = (gout.double() + EPS * 3 * z2.double()).clamp(0, 1)
    margin('cddls compose clamp n=%d' % n, maxabs(xc, refc), KTOL)
    assert float(xc.min()) >= 0.0 and float(xc.max()) <= 1.0
    if n > 100:
        assert float((xc == 0).sum()) > 0 and float((xc == 1).sum()) > 0

    z2d, glin = put(z2), put(torch.zeros(n))
    ops.cddls_image_end(put(gx), put(gout), z2d, glin, EPS, SIGMA_N, noise=put(nz))
    t = 2 * gout.double() - 1
    margin('cddls image_end g_lin n=%d' % n, maxabs(glin, gx.double() * 0.5 * (1 - t * t)), KTOL)
    ref2 = z2.double() - 0.5 * EPS * (EPS * gx.double() + z2.double()) + SIGMA_N * EPS ** 0.5 * nz.double()
    margin('cddls image_end z2 n=%d' % n, maxabs(z2d, ref2), KTOL)


@pytest.mark.parametrize('n,aligned', [(1 * 128, True), (3 * 128, True), (5 * 128, True), (7, False), (4 * (4096 + 3) + 1, True)])
def test_latent_update(margin, n, aligned):
    """The clamp is hit on both sides by construction; the last block advances the step and leaves the counter at 0."""
    from contrad_amd import ops
    g = gen(n)
    z, gz, nz = torch.rand(n, generator=g) * 2 - 1, torch.randn(n, generator=g), torch.randn(n, generator=g)
    z[0], gz[0], nz[0] = 0.99, -3.0, 1.0            # pushed above +1
    z[n - 1], gz[n - 1], nz[n - 1] = -0.99, 3.0, -1.0     # pushed below -1 (n == 1: this one wins)
    put = (lambda t: t.to(dev())) if aligned else unaligned
    zd = put(z)
    state = torch.tensor([41, 0, 0, 0], dtype=torch.int32, device=dev())
    ops.cddls_latent_update(zd, put(gz), EPS, SIGMA_N, noise=put(nz), state=state)
    raw = z.double() - 0.5 * EPS * gz.double() + SIGMA_N * EPS ** 0.5 * nz.double()
    assert raw[n - 1] < -1 and (n == 1 or raw[0] > 1)
    margin('cddls latent_update n=%d' % n, maxabs(zd, raw.clamp(-1, 1)), KTOL)
    assert float(zd[n - 1]) == -1.0 and (n == 1 or float(zd[0]) == 1.0)
    assert state.tolist() == [42, 0, 0, 0]


@pytest.mark.parametrize('N,hw', SIZES)
def test_energy(margin, N, hw):
    from contrad_amd import ops
    F, P = 512 * (hw // 8) ** 2, 3 * hw * hw
    g = gen(N + hw)
    d, f, c = torch.randn(N, 1, generator=g), torch.randn(N, F, generator=g).relu(), 0.1 * torch.randn(F, generator=g)
    b, z2 = torch.randn(1, generator=g), torch.randn(N, 3, hw, hw, generator=g)
    e = ops.cddls_energy(d.to(dev()), f.to(dev()), c.to(dev()), b.to(dev()), z2.to(dev()))
    ref = -d.double().view(-1) + f.double() @ c.double() + b.double() + 0.5 * (z2.double() ** 2).reshape(N, -1).sum(1)
    scale = d.double().abs().view(-1) + f.double() @ c.double().abs() + b.double().abs() + 0.5 * (z2.double() ** 2).reshape(N, -1).sum(1)
    margin('cddls energy N=%d F=%d' % (N, F), float(((e.double().cpu() - ref).abs() / scale).max()), 1e-5)


# ---------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------
BIG_SEED = (0x299f31d0 << 32) | 0xa4093822


@pytest.mark.parametrize('n', [1, 7, 4096 + 3])
def test_generator_words_and_normals(margin, n):
    from contrad_amd import ops
    for seed, stream, step in ((0, 0, 0), (1, 2, 0), (2024, 1, 999), (BIG_SEED, 0, 123456), (-5, 1, 3)):
        out, words = ops.cddls_normal_fill(n, seed, stream, step=step, device=dev(), want_words=True)
        w = words.cpu().numpy().view(np.uint32)
        assert np.array_equal(w, R.philox_words(n, seed, stream, step)), (seed, stream, step)
        ref = R.normals64(n, seed, stream, step)
        margin('cddls normals n=%d' % n, float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max()), 1.6e-5)
        # the step from device memory, another grid: the same bits
        st = torch.tensor([step, 0], dtype=torch.int32, device=dev())
        for grid in (1, 7):
            o2, _ = ops.cddls_normal_fill(n, seed, stream, step=-1, step_dev=st, device=dev(), grid_blocks=grid)
            assert torch.equal(o2, out)


def test_generator_statistics(margin):
    from contrad_amd import ops
    a, b, c, d = (ops.cddls_normal_fill(R.STAT_N, s, st, step=k, device=dev())[0].cpu().numpy()
                  for (s, st, k) in (R.STAT_A, R.STAT_B, R.STAT_STEP, R.STAT_SEED2))
    for name, x in (('a', a), ('b', b)):
        m1, m2, m4 = R.moments(x)
        margin('cddls generator |mean| ' + name, m1, R.B_MEAN)
        margin('cddls generator |var - 1| ' + name, m2, R.B_VAR)
        margin('cddls generator |m4 - 3| ' + name, m4, R.B_M4)
    margin('cddls generator corr streams', R.corr(a, b), R.B_CORR)
    margin('cddls generator corr steps', R.corr(a, c), R.B_CORR)
    margin('cddls generator corr seeds', R.corr(a, d), R.B_CORR)
    ref = R.normals64(R.STAT_N, *R.STAT_A)
    margin('cddls normals n=2^20', float(np.abs(a.astype(np.float64) - ref).max()), 1.6e-5)
    assert np.isfinite(a).all() and np.abs(a).max() < 5.9


# ---------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nets():
    """Fixture networks: float64 state dicts on the host, the float32 modules in eval mode on the device."""
    from contrad_amd.models.gan import get_architecture
    gsd, dsd = R.fixture_networks()
    G, D = get_architecture('sndcgan', (32, 32, 3))
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
    return np.load(os.path.join(GOLDEN, 'cddls.npz'))


def cpu_region(region):
    return {'g': [m.cpu() for m in region['g']], 'd': [m.cpu() for m in region['d']], 'hidden': region['hidden'].cpu()}


@pytest.mark.parametrize('N', [4, 3])
def test_one_step(margin, nets, N):
    """g_z, g_x and the energy of one step against ref64.  The gradient is checked on g_z and g_x themselves: the fixture
    networks give |g_z| ~ 2e-5 per entry, so at these constants the increment of z is noise to five digits and the two
    `dz` margins only check the update arithmetic (noise scale, clamp, the z2 decay), not the gradient."""
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = nets
    g = gen(100 + N)
    W, b = 0.05 * torch.randn(10, 8192, generator=g), 0.1 * torch.randn(10, generator=g)
    z0, z2_0 = torch.rand(N, 128, generator=g) * 2 - 1, torch.randn(N, 3, 32, 32, generator=g)
    n, n2 = torch.randn(N, 128, generator=g), torch.randn(N, 3, 32, 32, generator=g)
    y = 4
    S = CDDLSSampler(G, D, W.to(dev()), b.to(dev()), N, lbd=LBD, eps=EPS, sigma_n=SIGMA_N, energy=True)
    S.set_class(y)
    S.start(z0.to(dev()), z2=z2_0.to(dev()))
    S.step(noise=n.to(dev()), noise2=n2.to(dev()))
    region = cpu_region(S.linear_region())
    args = (gsd, dsd, W[y].double(), b[y].double(), z0.double(), z2_0.double(), n.double(), n2.double(), EPS, LBD, SIGMA_N)
    same, raw = R.langevin_step(*args, region=region), R.langevin_step(*args)
    tag = 'cddls step N=%d ' % N
    margin(tag + 'g_z same region', rel_l2(S.g_z, same['g_z']), TOL)
    margin(tag + 'g_x same region', rel_l2(S.g_x, same['g_x']), TOL)
    margin(tag + 'energy same region', float(((S.energy.double().cpu() - same['e']).abs() / same['e'].abs()).max()), TOL)
    margin(tag + 'g_z raw', rel_l2(S.g_z, raw['g_z']), FLIP_TOL)
    margin(tag + 'g_x raw', rel_l2(S.g_x, raw['g_x']), FLIP_TOL)
    margin(tag + 'energy raw', float(((S.energy.double().cpu() - raw['e']).abs() / raw['e'].abs()).max()), TOL)
    margin(tag + 'dz same region', rel_l2(S.z.cpu().double() - z0.double(), same['z'] - z0.double()), TOL)
    margin(tag + 'dz2 same region', rel_l2(S.z2.cpu().double() - z2_0.double(), same['z2'] - z2_0.double()), TOL)
    assert int(S.state[0]) == 1 and int(S.state[1]) == 0


_TRAINED_LIKE = {}


def trained_like(shift):
    """R.trained_like_networks(shift) at 16 x 16 images: norm_init with mean^2 / var up to 3.8e3 (shift 1) or 3.3e4 (shift 3)
    and running variances of 3e-4 .. 1e-3, as float64 state dicts and as eval-mode modules on the device."""
    if shift not in _TRAINED_LIKE:
        from contrad_amd.models.gan import get_architecture
        gsd, dsd = R.trained_like_networks(shift, 16)
        G, D = get_architecture('sndcgan', (16, 16, 3))
        full = dict(G.state_dict())
        full.update({k: v.float() for k, v in gsd.items()})
        G.load_state_dict(full)
        D.load_state_dict({k: v.float() for k, v in dsd.items()})
        G.to(dev()).eval(); D.to(dev()).eval()
        for p in list(G.parameters()) + list(D.parameters()):
            p.requires_grad_(False)
        _TRAINED_LIKE[shift] = (gsd, dsd, G, D)
    return _TRAINED_LIKE[shift]


@pytest.mark.parametrize('shift', [1.0, 3.0])
def test_g_forward_on_a_trained_like_state(margin, shift):
    """The sampler's norm_init output at N = 3 against float64, end to end from z and on the kernel's own input (h0), each
    under the rule of test_dstep_kernels_gpu.test_bn_relu_eval: max(FAMILY_TOL['bn_fwd'], 2 x the error of plain fp32 torch
    on the same device tensors)."""
    import torch.nn.functional as F
    import dstep_ref64 as K
    from contrad_amd.cddls import CDDLSSampler
    BN_FWD = (1.3e-6, 7e-7)             # FAMILY_TOL['bn_fwd'] of test_dstep_kernels_gpu.py
    gsd, dsd, G, D = trained_like(shift)
    N, g = 3, gen(int(shift))
    W, b = 0.05 * torch.randn(10, 2048, generator=g), 0.1 * torch.randn(10, generator=g)
    z = (torch.rand(N, 128, generator=g) * 2 - 1).to(dev())
    S = CDDLSSampler(G, D, W.to(dev()), b.to(dev()), N)
    S.set_class(1)
    S.start(z)
    S._g_forward()
    got = S.g_acts[0].permute(0, 3, 1, 2)                    # NHWC -> NCHW
    bn = G.norm_init
    sd32 = {k: v.to(dev()) for k, v in G.state_dict().items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    tag = 'cddls g_forward trained-like state +%g norm_init ' % shift
    # end to end from z
    a64, a32 = [], []
    R.g_eval_forward(sd64, z.double(), 16, acts=a64)
    R.g_eval_forward(sd32, z, 16, acts=a32)
    bound = K.bn_eval_bound(BN_FWD, K.errors(a32[0], a64[0]))
    emax, el2 = K.errors(got, a64[0])
    margin(tag + 'from z max-norm', emax, bound[0])
    margin(tag + 'from z rel-L2', el2, bound[1])
    # the BatchNorm alone, on the fp32 linear output the kernel read
    inp = dict(x=S.h0, cb=None, rm=bn.running_mean, rv=bn.running_var, gamma=bn.weight, beta=bn.bias)
    ref = K.bn_relu_eval(S.h0, None, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, 4)
    bound = K.bn_eval_bound(BN_FWD, K.errors(K.bn_relu_eval_fp32(inp, bn.eps, 4), ref))
    emax, el2 = K.errors(S.g_acts[0].view(N, -1), ref)
    margin(tag + 'from h0 max-norm', emax, bound[0])
    margin(tag + 'from h0 rel-L2', el2, bound[1])
    assert float(ref.max()) > 1.0 and F.relu(ref).count_nonzero() > ref.numel() // 4


def test_one_step_on_a_trained_like_state(margin):
    """test_one_step on the first trained-like state (16 x 16, N = 3): the running variances of 3e-4 .. 1e-3 scale the backward
    by up to 60 x per layer; g_z, g_x and the energy on the kernel's own linear region at the unchanged TOL."""
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = trained_like(1.0)
    N, g = 3, gen(103)
    W, b = 0.05 * torch.randn(10, 2048, generator=g), 0.1 * torch.randn(10, generator=g)
    z0, z2_0 = torch.rand(N, 128, generator=g) * 2 - 1, torch.randn(N, 3, 16, 16, generator=g)
    n, n2 = torch.randn(N, 128, generator=g), torch.randn(N, 3, 16, 16, generator=g)
    y = 4
    S = CDDLSSampler(G, D, W.to(dev()), b.to(dev()), N, lbd=LBD, eps=EPS, sigma_n=SIGMA_N, energy=True)
    S.set_class(y)
    S.start(z0.to(dev()), z2=z2_0.to(dev()))
    S.step(noise=n.to(dev()), noise2=n2.to(dev()))
    region = cpu_region(S.linear_region())
    same = R.langevin_step(gsd, dsd, W[y].double(), b[y].double(), z0.double(), z2_0.double(), n.double(), n2.double(), EPS,
                           LBD, SIGMA_N, image_hw=16, region=region)
    tag = 'cddls step trained-like state N=%d ' % N
    margin(tag + 'g_z same region', rel_l2(S.g_z, same['g_z']), TOL)
    margin(tag + 'g_x same region', rel_l2(S.g_x, same['g_x']), TOL)
    margin(tag + 'energy same region', float(((S.energy.double().cpu() - same['e']).abs() / same['e'].abs()).max()), TOL)
    assert int(S.state[0]) == 1 and float(same['g_z'].abs().max()) > 0


@pytest.mark.parametrize('yi', [0, 1])
def test_trajectory_against_reference(margin, nets, fx, yi):
    """Three steps on the reference's recorded draws: increments of z and z2 and the final images against ref64 on the
    kernel's own linear regions (1e-3) and against the reference's raw run (1e-2).  The raw criterion sees z2 per step only
    through its per-sample sums and in full only as the total increment: that is what the fixture stores under the size limit
    for committed files; the same-region criterion compares the full z2 tensors step by step."""
    from contrad_amd.cddls import CDDLSSampler
    gsd, dsd, G, D = nets
    y = int(fx['classes'][yi])
    W, b = R.fixture_head(fx)
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
    steps, ref_images = R.ref_trajectory(fx, y, regions=regions, nets=(gsd, dsd))
    tag = 'cddls trajectory y=%d ' % y
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


def test_invariants(nets):
    gsd, dsd, G, D = nets
    g = gen(8)
    W, b = (0.05 * torch.randn(10, 8192, generator=g)).to(dev()), (0.1 * torch.randn(10, generator=g)).to(dev())
    z0 = (torch.rand(8, 128, generator=g) * 2 - 1).to(dev())
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in (G, D)]
    S, z_a, z2_a, im_a = _run(G, D, W, b, z0, 11, False)
    assert int(S.state[0]) == 5 and bool(torch.isfinite(im_a).all())
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
    ptrs = [t.data_ptr() for t in S.d_wps + S.g_wps] + [f.buf.data_ptr() for f in (S.d_filters, S.g_filters) if f and f.buf is not None]
    c_before = S.c_row.clone()
    S.set_class(2); S.start(z0); S.step()
    assert ptrs == [t.data_ptr() for t in S.d_wps + S.g_wps] + [f.buf.data_ptr() for f in (S.d_filters, S.g_filters) if f and f.buf is not None]
    assert not torch.equal(S.c_row, c_before)
    from contrad_amd.cddls import permute_class_row
    assert torch.equal(S.c_row, permute_class_row(W[2], 4, 4) * -1.0)


def test_cli(tmp_path):
    from contrad_amd import cddls, lineval
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(3)
    G, D = get_architecture('sndcgan', (32, 32, 3))
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
    lineval.install_head(D, 2)
    lin = str(logdir / 'lin_eval_1.pth.tar')
    lineval.save_checkpoint(D, 1, lin)
    out = cddls.main([str(logdir), lin, 'sndcgan', '--n_samples', '12', '--n_classes', '2', '--batch_size', '4',
                      '--n_steps', '3', '--seed', '1', '--log_energy'])
    assert os.path.basename(out) == 'samples_cDDLS_1'
    assert sorted(os.listdir(os.path.join(out, '0'))) == sorted('%d.png' % i for i in range(6))
    assert sorted(os.listdir(os.path.join(out, '1'))) == sorted('%d.png' % i for i in range(6, 12))
    with np.load(os.path.join(out, 'samples.npz')) as z:
        assert z['images'].shape == (12, 32, 32, 3) and z['images'].dtype == np.uint8
        assert z['labels'].tolist() == [0] * 6 + [1] * 6
        assert z['images'].min() >= 0 and z['images'].max() <= 255 and z['images'].std() > 0
        first = z['images'][0]
    data = open(os.path.join(out, '0', '0.png'), 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and len(data) > 100
    try:
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, '0', '0.png')).convert('RGB')), first)
    except ImportError:
        pass
    with pytest.raises(NotImplementedError, match='sndcgan'):
        cddls.main([str(logdir), lin, 'stylegan2', '--n_samples', '2'])
