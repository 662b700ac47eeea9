"""Float64 yardstick of latent recovery (contrad_amd/recover.py; csrc/cddls.hip: the recovery forms of the energy and
image-end kernels, the Adam form of the latent update), using none of this project's kernels: the three forms restated, one
recovery step and a k-step trajectory on ``cddls_ref64.g_eval_forward`` with the ``region=`` convention of
``langevin_step``, and the statistics by brute force.  Every function computes in the dtype of its tensor inputs, so the
CPU test can run the same arithmetic in float32.  Shared by the CPU and the GPU tests; nothing here touches a GPU."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import cddls_ref64 as R
import cddls_snresnet_ref64 as RS

O = R.O


# ---- the three forms ----
def loss_form(gout, target, lam, phi=None, phi_target=None):
    """-> (pix, feat, loss (N,), resid (N, F) or None): pix = |gout - x*|^2 / P, feat = |phi - phi*|^2 / F (0 without phi),
    loss = pix + lam feat, resid = (2 lam / F)(phi - phi*)."""
    N = gout.shape[0]
    d = (gout - target).reshape(N, -1)
    pix = (d * d).sum(1) / d.shape[1]
    if phi is None:
        return pix, torch.zeros_like(pix), pix.clone(), None
    r = (phi - phi_target).reshape(N, -1)
    feat = (r * r).sum(1) / r.shape[1]
    return pix, feat, pix + lam * feat, (2.0 * lam / r.shape[1]) * r


def image_end_form(gout, target, P, g_x=None):
    """g_lin = ((2 / P)(gout - x*) [+ g_x]) * (1 - t^2) / 2, t = 2 gout - 1."""
    g = (2.0 / P) * (gout - target)
    if g_x is not None:
        g = g + g_x
    t = 2.0 * gout - 1.0
    return g * (0.5 * (1.0 - t * t))


def bias_corrections(betas, step):
    """(1 - b1^t, 1 - b2^t), t = step + 1: float64 pow of the float32 betas, rounded once to float32 (as Python floats)."""
    t = float(step) + 1.0
    return tuple(float(np.float32(1.0 - math.pow(float(np.float32(b)), t))) for b in betas)


def adam_form(z, g, m, v, lr, betas, adam_eps, step):
    """-> (z, m, v) after one step: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2,
    z <- clamp(z - lr (m / c1) / (sqrt(v / c2) + adam_eps), -1, 1) with the float32 values of lr, betas, adam_eps."""
    b1, b2 = (float(np.float32(b)) for b in betas)
    ob1, ob2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    lr, adam_eps = float(np.float32(lr)), float(np.float32(adam_eps))
    c1, c2 = bias_corrections(betas, step)
    m = b1 * m + ob1 * g
    v = b2 * v + ob2 * (g * g)
    u = (m / c1) / (torch.sqrt(v / c2) + adam_eps)
    return torch.clamp(z - lr * u, -1, 1), m, v


# ---- the networks ----
def d_features(dsd, x, d_type, masks=None):
    """phi: the D half's feature tensor as (N, F) rows (sndcgan: the last post-LeakyReLU map, flat; snresnet18: the 512
    pooled features), eval mode."""
    if d_type == 'sndcgan':
        return O.sndcgan_d_features(dsd, x, False, masks)
    if d_type == 'snresnet18':
        return O.snresnet18_features(dsd, x, False, masks)
    raise ValueError(d_type)


def g_forward(gsd, z, image_hw, masks=None):
    """-> (gout, h): G's output and its last pre-activation (gout = 0.5 tanh(h) + 0.5), both in the autograd graph of z."""
    acts = []
    gout = R.g_eval_forward(gsd, z, image_hw, masks, acts=acts)
    ci, co, k, s, p = O.SNDCGAN_G_CONVT[3]
    h = F.conv_transpose2d(acts[3], gsd['main.9.weight'], gsd['main.9.bias'], stride=s, padding=p)
    return gout, h


def g_region(gsd, z, image_hw):
    """The ReLU regions G itself runs on at z, in linear_region()'s layout."""
    acts = []
    with torch.no_grad():
        R.g_eval_forward(gsd, z, image_hw, acts=acts)
    return [(acts[0] > 0).reshape(z.shape[0], -1)] + [a > 0 for a in acts[1:]]


def definition_loss(gsd, z, target, image_hw=32, lam=0.0, dsd=None, d_type=None, region=None, phi_target=None):
    """The definition, plainly: per-sample (pix, feat, loss) of z as differentiable tensors."""
    gout = R.g_eval_forward(gsd, z, image_hw, region['g'] if region else None)
    N = z.shape[0]
    pix = ((gout - target) ** 2).reshape(N, -1).mean(1)
    if not lam:
        return pix, torch.zeros_like(pix), pix
    if phi_target is None:
        with torch.no_grad():
            phi_target = d_features(dsd, target, d_type)
    phi = d_features(dsd, gout, d_type, region['d'] if region else None)
    feat = ((phi - phi_target) ** 2).reshape(N, -1).mean(1)
    return pix, feat, pix + lam * feat


def recovery_step(gsd, z, m, v, target, step, lr, betas, adam_eps, image_hw=32, lam=0.0, dsd=None, d_type=None,
                  region=None, phi_target=None):
    """One recovery step through the three forms -> dict(z, m, v (the new state), g_z, g_x, pix, feat, loss (at the old z)).
    ``region``: {'g': [...], 'd': [...]} imposed instead of the signs of the pre-activations, or None."""
    z = z.detach().clone().requires_grad_()
    gout, h = g_forward(gsd, z, image_hw, region['g'] if region else None)
    P = gout[0].numel()
    g_x = None
    if lam:
        if phi_target is None:
            with torch.no_grad():
                phi_target = d_features(dsd, target, d_type)
        x = gout.detach().clone().requires_grad_()
        phi = d_features(dsd, x, d_type, region['d'] if region else None)
        pix, feat, loss, resid = loss_form(gout.detach(), target, lam, phi.detach(), phi_target)
        g_x, = torch.autograd.grad(phi, x, grad_outputs=resid)          # the D backward seeded from the residual rows
    else:
        pix, feat, loss, _ = loss_form(gout.detach(), target, 0.0)
    g_lin = image_end_form(gout.detach(), target, P, g_x)
    g_z, = torch.autograd.grad(h, z, grad_outputs=g_lin)
    z_new, m_new, v_new = adam_form(z.detach(), g_z, m, v, lr, betas, adam_eps, step)
    return {'z': z_new, 'm': m_new, 'v': v_new, 'g_z': g_z, 'g_x': g_x, 'pix': pix, 'feat': feat, 'loss': loss}


def trajectory(gsd, z0, target, k, lr, betas, adam_eps, image_hw=32, lam=0.0, dsd=None, d_type=None, regions=None):
    """k steps from z0 with zero moments -> (list of recovery_step's dicts with z_prev; the final pix)."""
    z, m, v = z0, torch.zeros_like(z0), torch.zeros_like(z0)
    steps = []
    for i in range(k):
        out = recovery_step(gsd, z, m, v, target, i, lr, betas, adam_eps, image_hw, lam, dsd, d_type,
                            None if regions is None else regions[i])
        out['z_prev'] = z
        steps.append(out)
        z, m, v = out['z'], out['m'], out['v']
    with torch.no_grad():
        pix = definition_loss(gsd, z, target, image_hw)[0]
    return steps, pix


# ---- the inputs of the GPU cases (the CPU test asserts the trajectory's condition) ----
LR, BETAS, ADAM_EPS = 0.3, (0.7, 0.95), 3e-6              # far from the defaults
# the fixture discriminators have small features: at this weight the feature term is a sizeable share of g_z (asserted in
# test_recover_ref64_cpu.py), so dropping or mis-scaling it shows at the step tolerances
LAMBDA_FEAT = 2500.0
TRAJ_N, TRAJ_STEPS, TRAJ_SEED = 4, 3, 401


def case(N, image_hw, seed):
    """float32-representable (z0, targets) of a one-step case: uniform latents, uniform images."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 128, generator=g) * 2 - 1, torch.rand(N, 3, image_hw, image_hw, generator=g)


def median_gradient(gsd, z0, target, image_hw=32, lam=0.0, dsd=None, d_type=None):
    """The float64 median |g_z| of the first step from z0, rounded to float32: the adam_eps of the cases that compare
    increments of z.  The update is then a smooth function of g through zero, and a sign flip of a near-zero gradient entry
    cannot move an increment by 2 lr."""
    z, t = z0.double(), target.double()
    first = recovery_step(gsd, z, torch.zeros_like(z), torch.zeros_like(z), t, 0, LR, BETAS, 1.0, image_hw, lam, dsd, d_type)
    return float(np.float32(first['g_z'].abs().median().item()))


def trajectory_case(gsd):
    """(z0, targets, adam_eps) of the trajectory (pixels only, 32 x 32, the fixture networks)."""
    z0, target = case(TRAJ_N, 32, TRAJ_SEED)
    return z0, target, median_gradient(gsd, z0, target)


# ---- the statistics ----
def percentile(sorted_values, q):
    """Linear interpolation between the order statistics (numpy's default)."""
    pos = (len(sorted_values) - 1) * q / 100.0
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(sorted_values) - 1)
    return sorted_values[lo] + (sorted_values[hi] - sorted_values[lo]) * (pos - lo)


def split_stats(pix):
    s = sorted(float(p) for p in pix)
    med = percentile(s, 50)
    return {'n': len(s), 'mean': math.fsum(s) / len(s), 'median': med, 'p10': percentile(s, 10), 'p90': percentile(s, 90),
            'psnr_median': 10.0 * math.log10(1.0 / med) if med > 0 else float('inf')}


def auc_brute(train, test):
    """P(train < test) + P(equal) / 2 by counting every pair."""
    wins = sum((1.0 if a < b else 0.5 if a == b else 0.0) for a in train for b in test)
    return wins / (len(train) * len(test))


def z_score(train, test):
    """(U - n m / 2) / sigma with the tie-corrected variance of the Mann-Whitney U."""
    n, m = len(train), len(test)
    u = auc_brute(train, test) * n * m
    both = [float(x) for x in train] + [float(x) for x in test]
    N = n + m
    ties = sum(c ** 3 - c for c in (both.count(x) for x in set(both)))
    var = n * m / 12.0 * ((N + 1) - ties / (N * (N - 1.0)))
    return (u - n * m / 2.0) / math.sqrt(var) if var > 0 else 0.0
