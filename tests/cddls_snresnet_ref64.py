"""Float64 restatement of one cDDLS Langevin step with D_SNResNet18 as the discriminator (contrad_amd/cddls.py's
``snresnet18`` D half; the reference's ``_sample_cddls`` on ``get_architecture('snresnet18', ...)``) on the CPU oracle, with
explicit noise and optional imposed linear regions, plus the three index forms of the join kernel
(csrc/cddls.hip: cddls_feature_seed_kernel) in the order of operations the kernel uses.  Shared by the CPU and the GPU
tests; nothing here touches a GPU or a kernel of this project."""
import math

import numpy as np
import torch

import cddls_ref64 as R

O = R.O
SLOPE = 0.1
G_SEED, D_SEED = 4321, 1234


def fixture_networks():
    """Float64 state dicts: O.det_fill of G_SNDCGAN(32) and D_SNResNet18, then R.POWER_ITERATIONS train-mode power
    iterations on every spectral-norm layer of D -- det_fill draws u, v at random, and in eval mode nothing iterates them
    (cddls_ref64.fixture_networks: sigma = u^T W v ~ 0 would blow the normalised weights of 20 stacked layers up)."""
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)          # det_fill draws in the default dtype: the same values everywhere
    try:
        gsd = {k: v.double() for k, v in O.det_fill(O.sndcgan_g_param_shapes(32), seed=G_SEED).items()}
        dsd = {k: v.double() for k, v in O.det_fill(O.snresnet18_param_shapes(), seed=D_SEED).items()}
    finally:
        torch.set_default_dtype(saved)
    for k in list(dsd):
        if k.endswith('.weight_orig'):
            for _ in range(R.POWER_ITERATIONS):
                O.spectral_norm_weight(dsd, k[:-len('.weight_orig')], training=True)
    return gsd, dsd


def d_forward(dsd, x, region=None):
    """-> (logit (N, 1), pooled features (N, 512)) in eval mode; ``region``: {'d': 17 masks, 'hidden': mask} or None."""
    dm = region['d'] if region else None
    hm = (region['hidden'], None, None) if region else None
    d, _, _, f = O.snresnet18_forward(dsd, x, sg_linear=False, training=False, act_masks=dm, hidden_masks=hm)
    return d, f


def energy_terms(gsd, dsd, w_y, b_y, z, z2, eps, lbd, region=None):
    """-> (x, per-sample e (N,), logit, features)."""
    x = R.g_eval_forward(gsd, z, 32, region['g'] if region else None) + eps * z2
    d, f = d_forward(dsd, x, region)
    l = f @ w_y + b_y
    e = -(d.view(-1) + lbd * l) + 0.5 * (z2 ** 2).reshape(z2.size(0), -1).sum(1)
    return x, e, d, f


def langevin_step(gsd, dsd, w_y, b_y, z, z2, n, n2, eps, lbd, sigma_n, region=None):
    """One step in float64 -> dict(z, z2 (the new state), g_z, g_z2, g_x, e, d, f)."""
    z = z.detach().clone().requires_grad_()
    z2 = z2.detach().clone().requires_grad_()
    x, e, d, f = energy_terms(gsd, dsd, w_y, b_y, z, z2, eps, lbd, region)
    g_z, g_z2, g_x = torch.autograd.grad(e.sum(), (z, z2, x))
    s = sigma_n * math.sqrt(eps)
    z_new = torch.clamp(z.detach() - 0.5 * eps * g_z + s * n, -1, 1)
    z2_new = z2.detach() - 0.5 * eps * g_z2 + s * n2
    return {'z': z_new, 'z2': z2_new, 'g_z': g_z, 'g_z2': g_z2, 'g_x': g_x, 'e': e.detach(), 'd': d.detach(),
            'f': f.detach(), 'drift': 0.5 * eps * g_z, 'noise': s * n}


def d_half(dsd, w_y, x, lbd, region=None):
    """The D half alone: logit, pooled features and d(-(D(x) + lbd <f, w_y>)) / dx."""
    x = x.detach().clone().requires_grad_()
    d, f = d_forward(dsd, x, region)
    g_x, = torch.autograd.grad((-(d.view(-1) + lbd * (f @ w_y))).sum(), x)
    return d.detach(), f.detach(), g_x


final_images = R.final_images


def preactivations(dsd, x):
    """The pre-activations of D's 17 trunk LeakyReLUs and of the logit head's hidden layer on images ``x`` (eval mode)."""
    import torch.nn.functional as F
    pres = []

    def conv(pre, h, stride, pad):
        return F.conv2d(h, O.spectral_norm_weight(dsd, pre, False), dsd[pre + '.bias'], stride=stride, padding=pad)

    def act(y):
        pres.append(y)
        return F.leaky_relu(y, SLOPE)
    with torch.no_grad():
        h = act(conv('conv1', x * 2. - 1., 1, 1))
        for pre, inp, planes, s, sc in O.snresnet18_blocks():
            o = conv(pre + '.conv2', act(conv(pre + '.conv1', h, s, 1)), 1, 1)
            h = act(o + (conv(pre + '.shortcut.0', h, s, 0) if sc else h))
        f = F.avg_pool2d(h, 4).reshape(h.size(0), -1)
        pres.append(F.linear(f, O.spectral_norm_weight(dsd, 'linear.l1', False), dsd['linear.l1.bias']))
    return pres


NEAR_ZERO, NEAR_ZERO_SHARE = 1e-5, 1e-4


def near_zero_share(pres):
    """Per layer, the share of pre-activations whose magnitude is below NEAR_ZERO of the layer's largest: the only entries
    a float32 run can put in another linear region."""
    return [float((p.abs() < NEAR_ZERO * p.abs().max()).double().mean()) for p in pres]


# ---- the three index forms of the join kernel, in the kernel's order of operations ----
def _d(act, slope):
    return torch.where(act > 0, torch.ones((), dtype=torch.float64), torch.full((), slope, dtype=torch.float64))


def seed_form(g, c, act, slope=SLOPE):
    """(N, F): (g + c) * d."""
    return (g.double() + c.double()) * _d(act, slope)


def pooled_form(g, c, act, slope=SLOPE):
    """act (N, T, C); g (N, C); c (C,): ((g + c) * inv_T) * d with inv_T the float32 reciprocal of T, as the kernel has it."""
    inv_t = float(np.float32(1.0) / np.float32(act.shape[1]))
    return ((g.double() + c.double()) * inv_t)[:, None, :] * _d(act, slope)


def join_form(a, b, act, slope=SLOPE):
    """flat: (a + b) * d."""
    return (a.double() + b.double()) * _d(act, slope)


# ---- the inputs of the one-step and D-half GPU cases (the CPU test checks their condition) ----
EPS, SIGMA_N, LBD = 0.5, 0.7, 2.5          # test_cddls_gpu.py's: far from the defaults
STEP_SIZES, DHALF_N, STEP_CLASS = (4, 3), 3, 4
# seeds at which the float64 runs keep clear of every LeakyReLU's kink (the first that pass
# test_cddls_snresnet_ref64_cpu.py::test_same_region_comparisons_are_well_conditioned, searched upwards from 204 / 203 / 300)
STEP_SEEDS, DHALF_SEED = {4: 209, 3: 206}, 301


def one_step_case(N):
    """float32-representable (W, b, z0, z2_0, n, n2) of the one-step case at batch N."""
    g = torch.Generator().manual_seed(STEP_SEEDS[N])
    W, b = 0.05 * torch.randn(10, 512, generator=g), 0.1 * torch.randn(10, generator=g)
    z0, z2_0 = torch.rand(N, 128, generator=g) * 2 - 1, torch.randn(N, 3, 32, 32, generator=g)
    n, n2 = torch.randn(N, 128, generator=g), torch.randn(N, 3, 32, 32, generator=g)
    return W, b, z0, z2_0, n, n2


def d_half_case():
    """float32-representable (W, images) of the D-half case."""
    g = torch.Generator().manual_seed(DHALF_SEED)
    return 0.05 * torch.randn(10, 512, generator=g), torch.rand(DHALF_N, 3, 32, 32, generator=g)


# ---- the fixture (tests/golden/cddls_snresnet18.npz) ----
def fixture_head(fx):
    """(10, 512) float64 classifier with the stored rows in place (the others are never read) and its bias."""
    W, b = torch.zeros(10, 512, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    for i, y in enumerate(fx['classes']):
        W[int(y)] = torch.from_numpy(fx['head.weight_rows'][i].astype(np.float64))
        b[int(y)] = float(fx['head.bias_rows'][i])
    return W, b


def ref_trajectory(fx, y, regions=None, nets=None):
    """The yardstick over the fixture's steps for class ``y`` (``regions``: one imposed linear region per step) -> (list of
    langevin_step's dicts, with the state each step started from as z_prev / z2_prev; the final images)."""
    gsd, dsd = nets if nets is not None else fixture_networks()
    W, b = fixture_head(fx)
    eps, lbd, sigma_n = float(fx['eps']), float(fx['lbd']), float(fx['sigma_n'])
    z, z2 = torch.from_numpy(fx['z0'].astype(np.float64)), torch.from_numpy(fx['z2_0'].astype(np.float64))
    steps = []
    for k in range(fx['n'].shape[0]):
        out = langevin_step(gsd, dsd, W[y], b[y], z, z2, torch.from_numpy(fx['n'][k].astype(np.float64)),
                            torch.from_numpy(fx['n2'][k].astype(np.float64)), eps, lbd, sigma_n,
                            region=None if regions is None else regions[k])
        out['z_prev'], out['z2_prev'] = z, z2
        steps.append(out)
        z, z2 = out['z'], out['z2']
    return steps, final_images(gsd, z, z2, eps)


def own_region(gsd, dsd, z, z2, eps):
    """The linear regions the yardstick itself runs on at (z, z2), in linear_region()'s layout."""
    import torch.nn.functional as F
    with torch.no_grad():
        g, h = [], F.linear(z, gsd['linear.weight'], gsd['linear.bias'])

        def bn(prefix, t):
            return F.batch_norm(t, gsd[prefix + '.running_mean'], gsd[prefix + '.running_var'], gsd[prefix + '.weight'],
                                gsd[prefix + '.bias'], False, 0.1, 1e-5)
        h = bn('norm_init', h.view(h.size(0), h.size(1), 1, 1)).view(h.size(0), -1)
        g.append(h > 0)
        h = F.relu(h).view(-1, 512, 4, 4)
        for j, (ci, co, k, s, p) in enumerate(O.SNDCGAN_G_CONVT):
            h = F.conv_transpose2d(h, gsd['main.%d.weight' % (3 * j)], gsd['main.%d.bias' % (3 * j)], stride=s, padding=p)
            if j < 3:
                h = bn('main.%d' % (3 * j + 1), h)
                g.append(h > 0)
                h = F.relu(h)
        x = 0.5 * torch.tanh(h) + 0.5 + eps * z2
        pres = preactivations(dsd, x)
    return {'g': g, 'd': [p > 0 for p in pres[:-1]], 'hidden': pres[-1] > 0}
