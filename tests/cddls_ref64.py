"""Float64 restatement of one cDDLS Langevin step (contrad_amd/cddls.py; the reference's ``_sample_cddls``) on the CPU
oracle, with explicit noise and optional imposed linear regions, plus the noise generator of csrc/cddls.hip in numpy
(Philox4x32-10, Box-Muller in float64).  Shared by the CPU and the GPU tests; nothing here touches a GPU."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import contrad_oracle as O  # noqa: E402

STREAM_Z, STREAM_Z2, STREAM_INIT = 0, 1, 2
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ---- the generator ----
def philox4x32_10(counter, key):
    """counter: (n, 4) uint32, key: (2,) uint32 -> (n, 4) uint32."""
    c = [np.asarray(counter, dtype=np.uint64)[:, i] & 0xffffffff for i in range(4)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(0xffffffff)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(0xffffffff)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xffffffff, (k1 + _W1) & 0xffffffff
    return np.stack(c, 1).astype(np.uint32)


def philox_words(n, seed, stream, step):
    """The raw words of elements 0 .. n - 1: counter (element // 4, step, stream, 0), key = the 64-bit seed."""
    nq = (n + 3) // 4
    ctr = np.zeros((nq, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(nq), step, stream
    seed = int(seed) & 0xffffffffffffffff
    return philox4x32_10(ctr, (seed & 0xffffffff, seed >> 32)).reshape(-1)[:n]


def box_muller64(words):
    """Float64 normals of a word array whose length is the element count: elements 4q, 4q + 1 from words 4q (radius) and
    4q + 1 (angle), elements 4q + 2, 4q + 3 from words 4q + 2, 4q + 3; even elements the cosine, odd ones the sine.
    The length must be even (normals64 generates whole quads and cuts)."""
    w = np.asarray(words, dtype=np.uint32).astype(np.float64)
    u = (np.floor(w / 256.0) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u[0::2]))
    a = 2.0 * np.pi * u[1::2]
    out = np.empty(len(w), np.float64)
    out[0::2], out[1::2] = r * np.cos(a), r * np.sin(a)
    return out


def box_muller32(words):
    """The kernel's float32 arithmetic restated in numpy (csrc/cddls.hip: neg_log_uniform, box_muller4): the radius from
    -ln u without rounding u (2x + 1 is a 24-bit integer below one half, 1 - u is one above, through log1p), the angle from
    the rounded float32 uniform.  numpy's float32 log / log1p / sqrt and a float64 sine / cosine of the float32 angle stand
    in for logf / log1pf / sqrtf / sincospif."""
    f = np.float32
    x = (np.asarray(words, dtype=np.uint32) >> 8).astype(np.int64)
    xr, xa = x[0::2], x[1::2]
    low = np.log(np.minimum(2 * xr + 1, (1 << 24) - 1).astype(f) * f(2.0 ** -25))
    high = np.log1p(-(np.maximum((1 << 25) - 2 * xr - 1, 1)).astype(f) * f(2.0 ** -25))
    r = np.sqrt(f(2) * -np.where(xr < (1 << 23), low, high).astype(f)).astype(f)
    u = ((xa.astype(f) + f(0.5)) * f(2.0 ** -24)).astype(f)
    a = (f(2) * u).astype(np.float64) * np.pi
    out = np.empty(len(x), f)
    out[0::2], out[1::2] = r * np.cos(a).astype(f), r * np.sin(a).astype(f)
    return out


def normals64(n, seed, stream, step):
    """Float64 normals of elements 0 .. n - 1 (whole quads are generated, then cut)."""
    nq = (n + 3) // 4
    return box_muller64(philox_words(4 * nq, seed, stream, step))[:n]


# ---- the networks in eval mode ----
def g_eval_forward(sd, z, image_hw=32, masks=None, acts=None):
    """G_SNDCGAN in eval mode (== O.sndcgan_g_forward(training=False) without masks); ``masks``: four bool tensors, the
    ReLU regions after norm_init ((N, f)) and after the three BatchNorms (NCHW), imposed instead of sign(pre-act).
    ``acts``: a list that receives the four post-ReLU activations (NCHW)."""
    hb = image_hw // 8

    def relu(h, m):
        h = F.relu(h) if m is None else h * m.to(h.dtype)
        if acts is not None:
            acts.append(h.view(h.size(0), 512, hb, hb) if h.dim() == 2 else h)
        return h

    def bn(prefix, h):
        return F.batch_norm(h, sd[prefix + '.running_mean'], sd[prefix + '.running_var'], sd[prefix + '.weight'],
                            sd[prefix + '.bias'], False, 0.1, 1e-5)
    mk = masks if masks is not None else [None] * 4
    h = F.linear(z, sd['linear.weight'], sd['linear.bias'])
    h = bn('norm_init', h.view(h.size(0), h.size(1), 1, 1)).view(h.size(0), -1)
    h = relu(h, mk[0]).view(-1, 512, hb, hb)
    for j, (ci, co, k, s, p) in enumerate(O.SNDCGAN_G_CONVT):
        h = F.conv_transpose2d(h, sd['main.%d.weight' % (3 * j)], sd['main.%d.bias' % (3 * j)], stride=s, padding=p)
        if j < 3:
            h = relu(bn('main.%d' % (3 * j + 1), h), mk[j + 1])
    return 0.5 * torch.tanh(h) + 0.5


def energy_terms(gsd, dsd, w_y, b_y, z, z2, eps, lbd, image_hw=32, region=None):
    """-> (x, per-sample e (N,)) of steps 1 - 4.  ``region``: {'g': [...], 'd': [...], 'hidden': mask} or None."""
    gm = region['g'] if region else None
    dm = region['d'] if region else None
    hm = (region['hidden'], None, None) if region else None
    x = g_eval_forward(gsd, z, image_hw, gm) + eps * z2
    d, _, _, f = O.sndcgan_d_forward(dsd, x, sg_linear=False, training=False, act_masks=dm, hidden_masks=hm)
    l = f @ w_y + b_y
    e = -(d.view(-1) + lbd * l) + 0.5 * (z2 ** 2).reshape(z2.size(0), -1).sum(1)
    return x, e


def langevin_step(gsd, dsd, w_y, b_y, z, z2, n, n2, eps, lbd, sigma_n, image_hw=32, region=None):
    """One step in float64 -> dict(z, z2 (the new state), g_z, g_x, e)."""
    z = z.detach().clone().requires_grad_()
    z2 = z2.detach().clone().requires_grad_()
    x, e = energy_terms(gsd, dsd, w_y, b_y, z, z2, eps, lbd, image_hw, region)
    g_z, g_z2, g_x = torch.autograd.grad(e.sum(), (z, z2, x))
    s = sigma_n * math.sqrt(eps)
    z_new = torch.clamp(z.detach() - 0.5 * eps * g_z + s * n, -1, 1)
    z2_new = z2.detach() - 0.5 * eps * g_z2 + s * n2
    return {'z': z_new, 'z2': z2_new, 'g_z': g_z, 'g_z2': g_z2, 'g_x': g_x, 'e': e.detach()}


def final_images(gsd, z, z2, eps, image_hw=32):
    with torch.no_grad():
        return torch.clamp(g_eval_forward(gsd, z, image_hw) + eps * z2, 0, 1)


POWER_ITERATIONS = 5


def fixture_networks(image_hw=32):
    """The float64 state dicts the fixture was made with: O.det_fill (seeds 4321 / 1234, as the other sndcgan fixtures),
    then POWER_ITERATIONS train-mode power iterations on every spectral-norm layer of D.  det_fill draws u and v at
    random; in eval mode nothing iterates them, sigma = u^T W v would be ~0 and the normalised weights of nine stacked
    layers would blow the logit up to 1e15.  A trained checkpoint carries converged u, v; so does this one."""
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)          # det_fill draws in the default dtype: the same values everywhere
    try:
        gsd = {k: v.double() for k, v in O.det_fill(O.sndcgan_g_param_shapes(image_hw), seed=4321).items()}
        dsd = {k: v.double() for k, v in O.det_fill(O.sndcgan_d_param_shapes(image_hw), seed=1234).items()}
    finally:
        torch.set_default_dtype(saved)
    for k in list(dsd):
        if k.endswith('.weight_orig'):
            for _ in range(POWER_ITERATIONS):
                O.spectral_norm_weight(dsd, k[:-len('.weight_orig')], training=True)
    return gsd, dsd


def trained_like_networks(bias_shift=1.0, image_hw=16, n_latents=64):
    """fixture_networks with a generator whose BatchNorm state looks like a trained one's: linear.weight x 0.2 and
    linear.bias + ``bias_shift`` (channels whose mean is far above their spread), and every running mean / variance set to
    the float64 population statistics of this generator's own pre-BatchNorm activations over ``n_latents`` latents, layer
    by layer, rounded to float32 (what a checkpoint stores).  -> (gsd, dsd), float64 copies of the float32 values."""
    gsd, dsd = fixture_networks(image_hw)
    gsd['linear.weight'] = (gsd['linear.weight'] * 0.2).float().double()
    gsd['linear.bias'] = (gsd['linear.bias'] + bias_shift).float().double()
    z = (torch.rand(n_latents, 128, generator=torch.Generator().manual_seed(64), dtype=torch.float64) * 2 - 1)
    hb = image_hw // 8

    def settle(prefix, h):              # h: pre-BN activation, channels in dim 1
        dims = [d for d in range(h.dim()) if d != 1]
        gsd[prefix + '.running_mean'] = h.mean(dims).float().double()
        gsd[prefix + '.running_var'] = h.var(dims, unbiased=False).float().double()
        return F.relu(F.batch_norm(h, gsd[prefix + '.running_mean'], gsd[prefix + '.running_var'], gsd[prefix + '.weight'],
                                   gsd[prefix + '.bias'], False, 0.1, 1e-5))
    h = settle('norm_init', F.linear(z, gsd['linear.weight'], gsd['linear.bias'])).view(-1, 512, hb, hb)
    for j, (ci, co, k, s, p) in enumerate(O.SNDCGAN_G_CONVT[:3]):
        h = settle('main.%d' % (3 * j + 1),
                   F.conv_transpose2d(h, gsd['main.%d.weight' % (3 * j)], gsd['main.%d.bias' % (3 * j)], stride=s, padding=p))
    return gsd, dsd


def bn_state_ratio(gsd, prefix):
    """max over channels of running_mean^2 / running_var of one BatchNorm of a state dict."""
    return float((gsd[prefix + '.running_mean'] ** 2 / gsd[prefix + '.running_var']).max())


# ---- the fixture (tests/golden/cddls.npz) ----
def fixture_head(fx):
    """(10, 8192) float64 classifier with the stored rows in place (the others are never read) and its bias."""
    W, b = torch.zeros(10, 8192, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    for i, y in enumerate(fx['classes']):
        W[int(y)] = torch.from_numpy(fx['head.weight_rows'][i].astype(np.float64))
        b[int(y)] = float(fx['head.bias_rows'][i])
    return W, b


def ref_trajectory(fx, y, regions=None, nets=None):
    """ref64 over the fixture's steps for class ``y`` (``regions``: one imposed linear region per step) -> (list of
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


# ---- statistical checks of the generator, shared by the CPU test (numpy) and the GPU test (kernel) ----
# (seed, stream, step) of the four samples: a reference one, the other stream, the next step, another seed
STAT_A, STAT_B, STAT_STEP, STAT_SEED2 = (2024, 0, 5), (2024, 1, 5), (2024, 0, 6), (977, 0, 5)
STAT_N = 1 << 20
# five standard errors over 2^20 draws: mean 1 / sqrt(n), variance sqrt(2 / n), fourth moment sqrt(96 / n), correlation 1 / sqrt(n)
B_MEAN, B_VAR, B_M4, B_CORR = 4.9e-3, 6.9e-3, 0.048, 4.9e-3


def moments(x):
    x = np.asarray(x, np.float64)
    return abs(x.mean()), abs(x.var() - 1.0), abs((x ** 4).mean() - 3.0)


def corr(a, b):
    return abs(np.corrcoef(np.asarray(a, np.float64), np.asarray(b, np.float64))[0, 1])
