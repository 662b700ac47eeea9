"""The yardstick of the StyleGAN2 projector (contrad_amd/project.py, csrc/project/project.hip): float64 numpy / torch written
for these tests, literal restatements of DESIGN.md section 25 that use none of this project's kernels, and the error bounds
of the four kernels.  No GPU.

Bounds.  u = 2^-24, gamma(k) = k u / (1 - k u) (Higham): a chain of k fp32 roundings moves a value by at most gamma(k) times
the sum of the magnitudes that went into it.  Each bound below counts the roundings of the kernel's own fixed summation order
(restated from the launch plan: values per workgroup, threads, butterfly steps) and multiplies by float64 magnitudes -- the
pooled ABSOLUTE residual or map where a pooled value may cancel.  Nothing is fitted to what the kernels return.

  image_end        pool_l: 3 adds per level on top of the rounding of x - t: gamma(3 l + 1) pool_l(|r|); squares, the sum chain
                   and the division on top.  The gradient adds L products and one scale.
  noise_grad       gamma(adds + 2) |noise_w| sum_k |g|.
  noise_reg        the pooled maps carry gamma(3 j) A_j (A_j = the pooled |map|), a product twice that, the means a_j, b_j the
                   chain of their sums; reg and the gradient inherit them by the product rule.
  noise_normalize  the mean about the first element, the centred values, the mean square, one division and one square root
                   (both correctly rounded), one product.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def cdiv(a, b):
    return -(-a // b)


# ---- the schedule ----
def schedule(t, rampdown=0.25, rampup=0.05):
    ramp = min(1.0, (1.0 - t) / rampdown)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return ramp * min(1.0, t / rampup)


def perturbation(t, w_std, noise_factor=0.05, noise_ramp=0.75):
    return w_std * noise_factor * max(0.0, 1.0 - t / noise_ramp) ** 2


# ---- image end ----
def pool(x, l):
    """The 2^l x 2^l mean over the last two axes (float64 numpy)."""
    x = np.asarray(x, np.float64)
    k = 1 << l
    s = x.shape
    return x.reshape(s[:-2] + (s[-2] // k, k, s[-1] // k, k)).mean(axis=(-3, -1))


def image_end(x, t, lam):
    """(pix (L, N), gx (N, 3, H, W)): pix_l[n] = mean(pool_l(x - t)^2), gx = d sum_n sum_l lam_l pix_l[n] / d x, hand-derived:
    sum_l lam_l (2 / P_l) 4^-l pool_l(r) spread back over each tile."""
    r = np.asarray(x, np.float64) - np.asarray(t, np.float64)
    N, _, H, W = r.shape
    pix = np.zeros((len(lam), N))
    gx = np.zeros_like(r)
    for l, w in enumerate(lam):
        p = pool(r, l)
        P_l = 3 * (H >> l) * (W >> l)
        pix[l] = (p ** 2).reshape(N, -1).sum(1) / P_l
        k = 1 << l
        gx += w * (2.0 / P_l) * (4.0 ** -l) * np.repeat(np.repeat(p, k, axis=-2), k, axis=-1)
    return pix, gx


def image_end_torch(x, t, lam):
    """The literal formula in float64 torch (avg_pool2d), for autograd: sum_n sum_l lam_l pix_l[n] and the rows."""
    rows = []
    for l in range(len(lam)):
        a, b = (F.avg_pool2d(v, 1 << l) if l else v for v in (x, t))
        rows.append(((a - b) ** 2).flatten(1).mean(1))
    rows = torch.stack(rows)
    return (torch.as_tensor(lam, dtype=torch.float64).view(-1, 1) * rows).sum(), rows


def image_end_rows(L, H, W):
    """Rows of a channel plane per workgroup (the launch plan of contrad_proj_image_end)."""
    rows = 1 << (L - 1)
    while rows * 2 * W <= 4096 and H % (rows * 2) == 0:
        rows *= 2
    return rows


def image_end_bounds(x, t, lam):
    ra = np.abs(np.asarray(x, np.float64) - np.asarray(t, np.float64))
    N, _, H, W = ra.shape
    L = len(lam)
    rows = image_end_rows(L, H, W)
    nb = 3 * (H // rows)
    pix_b = np.zeros((L, N))
    g_abs = np.zeros_like(ra)
    for l, w in enumerate(lam):
        pa = pool(ra, l)
        cnt = (rows >> l) * (W >> l)
        chain = cdiv(cnt, 256) + 6 + 4 + cdiv(nb, 64) + 6
        pix_b[l] = gamma(2 * (3 * l + 1) + 1 + chain + 3) * (pa ** 2).reshape(N, -1).sum(1) / (3 * (H >> l) * (W >> l))
        k = 1 << l
        g_abs += abs(w) * np.repeat(np.repeat(pa, k, axis=-2), k, axis=-1)
    gx_b = gamma(3 * (L - 1) + 1 + 2 * L + 3) * (2.0 / (3 * H * W)) * g_abs
    return pix_b, gx_b


# ---- the noise maps' gradient ----
def noise_grad(g_pre, noise_w):
    """(B, 1, H, W) = noise_w * sum_k g_pre[b, h, w, k]."""
    return float(noise_w) * np.asarray(g_pre, np.float64).sum(-1)[:, None]


def noise_grad_bound(g_pre, noise_w):
    K = g_pre.shape[-1]
    vec = K % 4 == 0
    per = K // 4 if vec else K
    s = 0
    while (1 << s) < per and s < 6:
        s += 1
    adds = cdiv(per, 1 << s) * (4 if vec else 1) + s
    return gamma(adds + 2) * abs(float(noise_w)) * np.abs(np.asarray(g_pre, np.float64)).sum(-1)[:, None]


# ---- the noise regulariser ----
def reg_levels(R):
    J = 1
    while R > 8:
        R //= 2
        J += 1
    return J


def noise_reg_torch(m):
    """The regulariser of the StyleGAN2 projector as its loop: m (N, 1, R, R) float64 torch -> reg (N,)."""
    reg = torch.zeros(m.shape[0], dtype=m.dtype)
    while True:
        reg = reg + (m * torch.roll(m, 1, 3)).flatten(1).mean(1) ** 2 + (m * torch.roll(m, 1, 2)).flatten(1).mean(1) ** 2
        if m.shape[2] <= 8:
            break
        m = F.avg_pool2d(m, 2)
    return reg


def _pyramid(m):
    out = [np.asarray(m, np.float64)]
    while out[-1].shape[-1] > 8:
        out.append(pool(out[-1], 1))
    return out


def noise_reg(m):
    """(reg (N,), d reg[n] / d m (N, 1, R, R)), the gradient hand-derived: (2 / R^2) sum_j a_j (m_j[y][x-1] + m_j[y][x+1]) +
    b_j (m_j[y-1][x] + m_j[y+1][x]) at (y, x) = (h, w) >> j."""
    levels = _pyramid(m)
    N, R = levels[0].shape[0], levels[0].shape[-1]
    reg = np.zeros(N)
    grad = np.zeros_like(levels[0])
    for j, mj in enumerate(levels):
        a = (mj * np.roll(mj, 1, -1)).reshape(N, -1).mean(1)
        b = (mj * np.roll(mj, 1, -2)).reshape(N, -1).mean(1)
        reg += a ** 2 + b ** 2
        gj = a.reshape(N, 1, 1, 1) * (np.roll(mj, 1, -1) + np.roll(mj, -1, -1)) + b.reshape(N, 1, 1, 1) * (np.roll(mj, 1, -2) + np.roll(mj, -1, -2))
        k = 1 << j
        grad += (2.0 / (R * R)) * np.repeat(np.repeat(gj, k, axis=-2), k, axis=-1)
    return reg, grad


def noise_reg_bounds(m, g_acc, scale):
    """(bound of reg (N,), bound of g_acc + scale * grad (N, 1, R, R))."""
    levels = _pyramid(m)
    A = _pyramid(np.abs(np.asarray(m, np.float64)))
    N, R = levels[0].shape[0], levels[0].shape[-1]
    J = len(levels)
    reg_b = np.zeros(N)
    mag = np.zeros(N)
    gerr = np.zeros_like(levels[0])
    gabs = np.zeros_like(levels[0])
    for j, (mj, Aj) in enumerate(zip(levels, A)):
        S = mj.shape[-1]
        nbj = cdiv(S * S, 4096)
        chain = cdiv(min(S * S, 4096), 256) + 6 + 4 + cdiv(nbj, 64) + 6
        g = gamma(6 * j + 1 + chain + 1)
        a = (mj * np.roll(mj, 1, -1)).reshape(N, -1).mean(1)
        b = (mj * np.roll(mj, 1, -2)).reshape(N, -1).mean(1)
        ea = g * (Aj * np.roll(Aj, 1, -1)).reshape(N, -1).mean(1)
        eb = g * (Aj * np.roll(Aj, 1, -2)).reshape(N, -1).mean(1)
        reg_b += 2 * np.abs(a) * ea + ea ** 2 + 2 * np.abs(b) * eb + eb ** 2
        mag += a ** 2 + b ** 2
        SW = np.roll(Aj, 1, -1) + np.roll(Aj, -1, -1)
        SH = np.roll(Aj, 1, -2) + np.roll(Aj, -1, -2)
        g2 = gamma(3 * j + 2 + 2 * J + 3)
        k = 1 << j
        up = lambda v: np.repeat(np.repeat(v, k, axis=-2), k, axis=-1)          # noqa: E731
        r4 = lambda v: v.reshape(N, 1, 1, 1)                                    # noqa: E731
        gerr += up((r4(ea) + r4(np.abs(a)) * g2) * SW + (r4(eb) + r4(np.abs(b)) * g2) * SH)
        gabs += up(r4(np.abs(a)) * SW + r4(np.abs(b)) * SH)
    reg_b += gamma(2 * J + 4) * mag
    c = 2.0 / (R * R)
    g_b = abs(scale) * c * gerr * (1.0 + gamma(4)) + gamma(3) * (np.abs(np.asarray(g_acc, np.float64)) + abs(scale) * c * gabs)
    return reg_b, g_b


# ---- the noise normalisation ----
def noise_normalize(m):
    """Per image: m - mean(m), times rsqrt(mean of its square); all zeros where that mean square is 0."""
    m = np.asarray(m, np.float64)
    c = m - m.mean(axis=(1, 2, 3), keepdims=True)
    ms = (c ** 2).mean(axis=(1, 2, 3), keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(ms > 0, c / np.sqrt(ms), 0.0)


def noise_normalize_bound(m):
    m = np.asarray(m, np.float64)
    n = m.shape[-1] ** 2
    threads = 1024 if n >= 65536 else 256
    it, nw = cdiv(n // 4, threads), threads // 64
    ax = dict(axis=(1, 2, 3), keepdims=True)
    pivot = m[:, :, :1, :1]
    mean = m.mean(**ax)
    e_mean = gamma(1 + 2 + it + 6 + nw + 2) * np.abs(m - pivot).mean(**ax) + U * np.abs(mean)
    c = m - mean
    dc = e_mean + U * np.abs(c)
    ms = (c ** 2).mean(**ax)
    e_ms = (2 * np.abs(c) * dc + dc ** 2).mean(**ax) + gamma(2 + 2 + it + 6 + nw + 2) * ms
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(ms > 0, e_ms / ms, 0.0)
        r = np.where(ms > 0, 1.0 / np.sqrt(ms), 0.0)
    rel_r = 0.5 * rel / (1.0 - np.minimum(rel, 0.5)) + 3 * U
    return r * dc * (1.0 + rel_r) + np.abs(c) * r * (rel_r + 2 * U)


# ---- float64 synthesis and projector loop ----
def state64(G):
    """The state dict of a generator as float64 CPU tensors (the reference's key names, blur kernels included)."""
    return {k: v.detach().double().cpu() for k, v in G.state_dict().items()}


def _styled(O, sd, pre, x, style, noise, upsample, mask, pres):
    """oracle.styled_layer; with ``mask`` the leaky-relu region of this layer is imposed (oracle._lrelu's ``mask``: the
    region the path under test ran on), with ``pres`` the pre-activation is kept."""
    if mask is None and pres is None:
        return O.styled_layer(sd, pre, x, style, noise, upsample=upsample)
    out = O.modulated_conv(sd, pre + '.conv', x, style, upsample=upsample) + sd[pre + '.noise.weight'] * noise
    if pres is not None:
        pres.append((out + sd[pre + '.activate.bias'].view(1, -1, 1, 1)).detach())
    return O.fused_leaky_relu(out, sd[pre + '.activate.bias'], mask=mask)


def synthesis(sd, latents, noise, size, masks=None, pres=None):
    """0.5 * skip + 0.5 of the synthesis network for W+ latents (B, n_latent, D) and per-image (or shared) noise maps, in the
    precision of ``sd``: assembled from the pieces of oracle/stylegan2_oracle.py.  ``masks``: one bool NCHW tensor per styled
    layer, the leaky-relu regions to evaluate on (None: the reference's own); ``pres``: a list that receives the styled
    layers' pre-activations."""
    from oracle import stylegan2_oracle as O
    log_size = int(math.log2(size))
    B = latents.shape[0]
    k = [0]

    def styled(pre, x, style, nz, upsample=False):
        k[0] += 1
        return _styled(O, sd, pre, x, style, nz, upsample, None if masks is None else masks[k[0] - 1], pres)
    out = sd['input.const'].repeat(B, 1, 1, 1)
    out = styled('conv1', out, latents[:, 0], noise[0])
    skip = O.to_rgb(sd, 'to_rgb1', out, latents[:, 1])
    idx = 1
    for j in range(log_size - 2):
        out = styled('layers.%d' % (2 * j), out, latents[:, idx], noise[1 + 2 * j], upsample=True)
        out = styled('layers.%d' % (2 * j + 1), out, latents[:, idx + 1], noise[2 + 2 * j])
        skip = O.to_rgb(sd, 'to_rgbs.%d' % j, out, latents[:, idx + 2], skip)
        idx += 2
    return 0.5 * skip + 0.5


def region_masks(recorded):
    """The leaky-relu regions of a forward of ``Generator.synthesize`` from its ``_record_regions`` list (NHWC outputs of the
    styled layers; leaky-relu keeps the sign) as bool NCHW CPU tensors."""
    return [(t > 0).permute(0, 3, 1, 2).cpu() for t in recorded]


def region_changes(masks, pres):
    """(number of units whose imposed region differs from the reference's own, the largest |pre-activation| among them)."""
    n, worst = 0, 0.0
    for m, p in zip(masks, pres):
        diff = m != (p > 0)
        n += int(diff.sum())
        if diff.any():
            worst = max(worst, float(p[diff].abs().max()))
    return n, worst


def to_latents(w, n_latent):
    return w.unsqueeze(1).repeat(1, n_latent, 1) if w.dim() == 2 else w


def loss_and_grads(sd, size, n_latent, target, w, maps, lam, reg_weight, noise_opt, masks=None, pres=None):
    """One forward and backward of the objective in float64 torch -> (loss rows (N,), pix rows (L, N), reg (layers, N), d w,
    [d map]).  ``masks`` / ``pres``: as in ``synthesis``."""
    w = w.detach().clone().requires_grad_()
    maps = [m.detach().clone().requires_grad_(noise_opt) for m in maps]
    x = synthesis(sd, to_latents(w, n_latent), maps, size, masks=masks, pres=pres)
    total, rows = image_end_torch(x, target, lam)
    regs = torch.stack([noise_reg_torch(m) for m in maps]) if noise_opt else torch.zeros(len(maps), w.shape[0], dtype=torch.float64)
    (total + reg_weight * regs.sum()).backward()
    loss = (torch.as_tensor(lam, dtype=torch.float64).view(-1, 1) * rows).sum(0) + reg_weight * regs.sum(0)
    return loss.detach(), rows.detach(), regs.detach(), w.grad, [m.grad for m in maps]


def normalize_torch(m):
    return torch.from_numpy(noise_normalize(m.numpy()))


def projector(sd, size, n_latent, target, w0, maps0, gauss, lam, reg_weight, lr0, noise_opt, w_std=0.0, betas=(0.9, 0.999),
              eps=1e-8, noise_factor=0.05, rampdown=0.25, rampup=0.05, noise_ramp=0.75, regions=None):
    """The projector loop in float64; ``gauss``: one draw per step in w's shape (their number is the number of steps).  ->
    list per step of dict(w, maps, loss, pix, reg, flips) after the step (loss rows of the step's forward).  ``regions``: per
    step the masks of ``synthesis`` (the regions the path under test ran on); ``flips`` is then ``region_changes``."""
    S = len(gauss)
    w = w0.double().clone()
    maps = [m.double().clone() for m in maps0]
    params = [w] + (maps if noise_opt else [])
    m1 = [torch.zeros_like(p) for p in params]
    m2 = [torch.zeros_like(p) for p in params]
    out = []
    for s in range(S):
        t = s / S
        w_in = w + gauss[s].double() * perturbation(t, w_std, noise_factor, noise_ramp)
        pres = []
        loss, rows, regs, gw, gmaps = loss_and_grads(sd, size, n_latent, target, w_in, maps, lam, reg_weight, noise_opt,
                                                     masks=None if regions is None else regions[s], pres=pres)
        lr = lr0 * schedule(t, rampdown, rampup)
        grads = [gw] + (gmaps if noise_opt else [])
        bc1, bc2 = 1.0 - betas[0] ** (s + 1), 1.0 - betas[1] ** (s + 1)
        for p, g, a, b in zip(params, grads, m1, m2):
            a.mul_(betas[0]).add_(g, alpha=1.0 - betas[0])
            b.mul_(betas[1]).addcmul_(g, g, value=1.0 - betas[1])
            p.sub_((lr / bc1) * a / (b.sqrt() / math.sqrt(bc2) + eps))
        if noise_opt:
            for i in range(len(maps)):
                maps[i].copy_(normalize_torch(maps[i]))
        out.append({'w': w.clone(), 'maps': [m.clone() for m in maps], 'loss': loss, 'pix': rows, 'reg': regs,
                    'flips': region_changes(regions[s], pres) if regions is not None else (0, 0.0)})
    return out
