"""Float64 references of the SimCLR augmentation kernels (csrc/augment.hip), in plain torch on whatever device the
inputs live on, using none of this project's kernels.  Every function takes the fp32 tensors the kernel read (images, the
(B, 16) parameter block of include/contrad_hip.h, the 1-D blur taps) and returns float64 results, so that the difference
is the kernel's own error.  tests/test_aug_sg2_ref64_cpu.py checks them against the fp32 oracle, the reference's goldens
and CPU float64 autograd.

Parameter columns: 0..3 theta00 (last axis, W), theta11 (H), theta02, theta12; 4 flip sign; 5 jitter mask; 6 contrast
factor; 7..9 f_h, f_s, f_v; 10 gray mask; 11 blur mask; 12..14 cutout mask, row and column centre; 15 contrast first.
(The reference's sampler names shape[2] "width": theta00 = w / shape[2] scales the last axis.  The kernels take theta as
the sampler wrote it, so a non-square image keeps the quirk; see oracle.contrad_oracle.sample_resized_crop_theta.)"""
import math

import torch
import torch.nn.functional as F

f64 = torch.float64
GRAY = (0.299, 0.587, 0.114)


def _d(t):
    return t.to(f64)


def theta(P):
    P = _d(P)
    th = torch.zeros(P.shape[0], 2, 3, dtype=f64, device=P.device)
    th[:, 0, 0], th[:, 1, 1], th[:, 0, 2], th[:, 1, 2] = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    return th


def crop_flip(x, P):
    """RandomResizeCropLayer + HorizontalFlipLayer: affine_grid + grid_sample (bilinear, reflection,
    align_corners=False), then the flip as the exact column permutation the reference's second grid_sample is."""
    x = x if x.dtype == f64 else _d(x)
    grid = F.affine_grid(theta(P), list(x.shape), align_corners=False)
    y = F.grid_sample(x, grid, mode='bilinear', padding_mode='reflection', align_corners=False)
    flip = (P[:, 4] < 0).view(-1, 1, 1, 1)
    return torch.where(flip, y.flip(-1), y)


def crop_flip_adjoint(g, P, H, W):
    """The transpose of crop_flip applied to g (B, 3, H, W): float64 autograd of the gather."""
    x = torch.zeros(g.shape[0], g.shape[1], H, W, dtype=f64, device=g.device, requires_grad=True)
    y = crop_flip(x, P)
    return torch.autograd.grad(y, x, _d(g))[0]


def rgb2hsv(rgb):
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    cmax, cmin = rgb.max(1)[0], rgb.min(1)[0]
    hue = torch.atan2(math.sqrt(3) * (g - b), 2 * r - g - b)
    hue = torch.remainder(hue, 2 * math.pi) / (2 * math.pi)
    sat = 1 - cmin / (cmax + 1e-8)
    hsv = torch.stack([hue, sat, cmax], 1)
    return torch.where(torch.isfinite(hsv), hsv, torch.zeros_like(hsv))


def hsv2rgb(hsv):
    h, s, v = hsv[:, 0:1], hsv[:, 1:2], hsv[:, 2:3]
    n = torch.tensor([5., 3., 1.], dtype=f64, device=hsv.device).view(1, 3, 1, 1)
    k = torch.remainder(n + h * 6, 6)
    t = torch.clamp(torch.minimum(k, 4 - k), 0, 1)
    return v - v * s * t


def hsv_jitter(x, P):
    """RandomHSVFunction.forward with the 255/360 hue quirk (its backward is the identity: see simclr_bwd)."""
    fh, fs, fv = [_d(P[:, c]).view(-1, 1, 1) for c in (7, 8, 9)]
    hsv = rgb2hsv(x)
    h = torch.remainder(hsv[:, 0] + fh * 255. / 360., 1)
    hsv = torch.clamp(torch.stack([h, hsv[:, 1] * fs, hsv[:, 2] * fv], 1), 0, 1)
    return hsv2rgb(hsv)


class _StraightThrough(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, P):
        return hsv_jitter(x, P)

    @staticmethod
    def backward(ctx, g):
        return g, None


def contrast_pre(x, P, has_contrast):
    """adjust_contrast before its clamp: (x - mean) * f + mean, or x when there is no contrast factor."""
    if not has_contrast:
        return x
    m = x.mean((2, 3), keepdim=True)
    return (x - m) * _d(P[:, 6]).view(-1, 1, 1, 1) + m


def contrast_first(P, cf):
    """The per-sample op order: the launch argument, or column 15 when it is negative (graph replay)."""
    if cf < 0:
        return P[:, 15] != 0
    return torch.full((P.shape[0],), bool(cf), device=P.device)


def _sel(mask, a, b):
    return torch.where(mask.view(-1, 1, 1, 1), a, b)


def simclr_parts(x, P, cf, has_contrast, straight_through=False):
    """The fused pipeline (crop + flip -> RandomApply(jitter) -> RandomApply(gray)) -> (y, pre), pre the float64 value
    each jittered element had before the contrast clamp (NaN where the sample is not jittered)."""
    hsv = _StraightThrough.apply if straight_through else hsv_jitter
    c = crop_flip(x, P)
    first = contrast_first(P, cf)
    a = _sel(first, c, hsv(c, P))
    pre = contrast_pre(a, P, has_contrast)
    cl = torch.clamp(pre, 0, 1)
    jit = _sel(first, hsv(cl, P), cl)
    jmask = P[:, 5] != 0
    y = _sel(jmask, jit, c)
    gw = torch.tensor(GRAY, dtype=f64, device=x.device).view(1, 3, 1, 1)
    l = (y * gw).sum(1, keepdim=True).expand_as(y)
    y = _sel(P[:, 10] != 0, l, y)
    return y, torch.where(jmask.view(-1, 1, 1, 1), pre.detach(), torch.full_like(pre, float('nan')))


def simclr(x, P, cf, has_contrast):
    return simclr_parts(x, P, cf, has_contrast)[0]


def simclr_bwd(x, P, gout, cf, has_contrast):
    """d loss / d x of simclr given d loss / d y = gout: float64 autograd with the HSV stage straight-through
    (oracle._StraightThroughHSV); torch.clamp passes the gradient at the boundary values 0 and 1."""
    xd = _d(x).requires_grad_(True)
    y, _ = simclr_parts(xd, P, cf, has_contrast, straight_through=True)
    return torch.autograd.grad(y, xd, _d(gout))[0]


def clamp_grad(P, gout):
    """The gradient arriving at the contrast clamp: gout through the gray blend's transpose."""
    g = _d(gout)
    gw = torch.tensor(GRAY, dtype=f64, device=g.device).view(1, 3, 1, 1)
    return _sel(P[:, 10] != 0, g.sum(1, keepdim=True) * gw, g)


def simclr_bwd_closed(x, P, gout, cf, has_contrast, passing=None):
    """simclr_bwd in the closed form the kernels evaluate: gray backward, the clamp mask gm = g * passing, contrast
    backward f * gm + (1 - f) * mean(gm) on jittered samples (HSV straight-through), then the gather transpose.
    ``passing`` (B, 3, H, W) bool overrides the clamp mask (default: 0 <= pre <= 1, as torch.clamp)."""
    B, _, H, W = x.shape
    _, pre = simclr_parts(_d(x), P, cf, has_contrast)
    if passing is None:
        passing = (pre >= 0) & (pre <= 1)
    g = clamp_grad(P, gout)
    gm = torch.where(passing, g, torch.zeros_like(g))
    f = _d(P[:, 6]).view(-1, 1, 1, 1) if has_contrast else torch.ones(B, 1, 1, 1, dtype=f64, device=g.device)
    gc = _sel(P[:, 5] != 0, f * gm + (1 - f) * gm.mean((2, 3), keepdim=True), g)
    return crop_flip_adjoint(gc, P, H, W)


def resolve_kinks(x, P, gout, cf, has_contrast, got, tau=1e-5):
    """The clamp kinks of the backward.  K = jittered elements whose float64 pre-clamp value lies within tau of 0 or 1:
    fp32 may put them on either side of the clamp.  Starting from the float64 mask, each element of K is flipped when
    that brings the reference closer to ``got`` on its sample (the flip moves the <= 4 pixels it samples from and,
    through the contrast mean, its channel).  -> (reference with the chosen mask, |K|, number of flips).  Every other element
    keeps the float64 mask, so the comparison that follows needs no exclusion and no slack."""
    B, _, H, W = x.shape
    _, pre = simclr_parts(_d(x), P, cf, has_contrast)
    K = ((pre.abs() < tau) | ((pre - 1).abs() < tau)) & ~torch.isnan(pre)
    passing = (pre >= 0) & (pre <= 1)
    ref = simclr_bwd_closed(x, P, gout, cf, has_contrast, passing)
    g = clamp_grad(P, gout)
    got = _d(got)
    flips = 0
    for b, c, i, j in K.nonzero().tolist():
        dg = -g[b, c, i, j] if passing[b, c, i, j] else g[b, c, i, j]
        f = float(P[b, 6]) if has_contrast else 1.0
        dgc = torch.zeros(1, 3, H, W, dtype=f64, device=g.device)
        dgc[0, c] += (1 - f) * dg / (H * W)
        dgc[0, c, i, j] += f * dg
        delta = crop_flip_adjoint(dgc, P[b:b + 1], H, W)[0]
        if (got[b] - ref[b] - delta).norm() < (got[b] - ref[b]).norm():
            ref[b] += delta
            passing[b, c, i, j] = ~passing[b, c, i, j]
            flips += 1
    return ref, int(K.sum()), flips


def gaussian_blur(x, P, k1d):
    """RandomApply(GaussianBlur): separable (2R+1)-tap correlation, reflect padding, on samples with blur mask != 0."""
    x = x if x.dtype == f64 else _d(x)
    g = _d(k1d)
    R = (g.numel() - 1) // 2
    C = x.shape[1]
    k2 = torch.outer(g, g).view(1, 1, 2 * R + 1, 2 * R + 1).repeat(C, 1, 1, 1)
    y = F.conv2d(F.pad(x, [R, R, R, R], mode='reflect'), k2, groups=C)
    return _sel(P[:, 11] != 0, y, x)


def gaussian_blur_bwd(gout, P, k1d):
    xd = torch.zeros(gout.shape, dtype=f64, device=gout.device, requires_grad=True)
    return torch.autograd.grad(gaussian_blur(xd, P, k1d), xd, _d(gout))[0]


def cutout(y, P, length):
    """RandomApply(CutOut(length)) with the centres of columns 13 / 14 (exact: a 0/1 mask)."""
    B, C, H, W = y.shape
    half = (length - 1) // 2
    i = torch.arange(H, device=y.device).view(1, H, 1)
    j = torch.arange(W, device=y.device).view(1, 1, W)
    hc, wc = P[:, 13].long().view(B, 1, 1), P[:, 14].long().view(B, 1, 1)
    win = ((i - hc).abs() <= half) & ((j - wc).abs() <= half) & (P[:, 12] != 0).view(B, 1, 1)
    return torch.where(win.unsqueeze(1), torch.zeros_like(y), y)
