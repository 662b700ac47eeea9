"""Float64 references of the StyleGAN2 op kernels (csrc/stylegan2_ops.hip), in plain torch on whatever device the inputs
live on, using none of this project's kernels.  Every function takes the fp32 tensors the kernel read and returns float64
results, so that the difference is the kernel's own error.  Activations are NHWC ([major, h, w, minor]) as the kernels
see them.  tests/test_aug_sg2_ref64_cpu.py checks them against the fp32 oracle, the reference's goldens and CPU float64
autograd."""
import math

import torch
import torch.nn.functional as F

f64 = torch.float64
SQRT2 = math.sqrt(2.0)


def _d(t):
    return None if t is None else t.to(f64)


def upfirdn2d(x, k, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """upfirdn2d_native per axis: zero-insertion upsampling, padding (negative crops), correlation with the flipped
    kernel, decimation.  x [major, in_h, in_w, minor] -> [major, out_h, out_w, minor]."""
    x, k = _d(x), _d(k)
    M, H, W, C = x.shape
    kh, kw = k.shape
    t = x.permute(0, 3, 1, 2).reshape(M * C, 1, H, 1, W, 1)
    t = F.pad(t, [0, up_x - 1, 0, 0, 0, up_y - 1]).reshape(M * C, 1, H * up_y, W * up_x)
    t = F.pad(t, [max(pad_x0, 0), max(pad_x1, 0), max(pad_y0, 0), max(pad_y1, 0)])
    t = t[:, :, max(-pad_y0, 0):t.shape[2] - max(-pad_y1, 0), max(-pad_x0, 0):t.shape[3] - max(-pad_x1, 0)]
    t = F.conv2d(t, torch.flip(k, [0, 1]).view(1, 1, kh, kw))[:, :, ::down_y, ::down_x]
    return t.reshape(M, C, t.shape[2], t.shape[3]).permute(0, 2, 3, 1)


def out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    return (in_h * up_y + pad_y0 + pad_y1 - kh) // down_y + 1, (in_w * up_x + pad_x0 + pad_x1 - kw) // down_x + 1


def fused_epilogue(v, addend=None, act_ref=None, slope=0.2, gain=1.0):
    """contrad_upfirdn2d_fused: v [+ addend] -> (out, out2 = v * (act_ref > 0 ? gain : slope * gain))."""
    v = _d(v)
    if addend is not None:
        v = v + _d(addend)
    out2 = None
    if act_ref is not None:
        out2 = v * torch.where(act_ref > 0, torch.tensor(float(gain), dtype=f64, device=v.device),
                               torch.tensor(float(slope) * float(gain), dtype=f64, device=v.device))
    return v, out2


def modconv_epilogue(v, bias, demod=None, noise=None, noise_w=None, post=None):
    """sqrt2 * lrelu_0.2(v * demod[n, k] + noise_w * noise[n, h, w] + bias[k]) [* post[n, k]], v [N, h, w, K]."""
    v = _d(v)
    N = v.shape[0]
    if demod is not None:
        v = v * _d(demod).view(N, 1, 1, -1)
    if noise is not None and noise_w is not None:
        v = v + _d(noise_w)[0] * _d(noise).view(N, v.shape[1], v.shape[2], 1)
    v = v + _d(bias).view(1, 1, 1, -1)
    v = torch.where(v > 0, v, 0.2 * v) * SQRT2
    if post is not None:
        v = v * _d(post).view(N, 1, 1, -1)
    return v


def fused_bias_act(x, bias, ref, step_b, size_b, act, grad, alpha, scale):
    """fused_bias_act: grad 0 y = act(x + bias[(i / step_b) % size_b]) * scale; grad 1 y = (x + b) * act'(ref) * scale;
    grad 2 y = 0.  act 1 linear, 3 leaky-relu(alpha).  x flat."""
    v = _d(x)
    if bias is not None:
        i = torch.arange(v.numel(), device=v.device)
        v = v + _d(bias)[(i // step_b) % size_b]
    alpha, scale = float(alpha), float(scale)
    if grad == 2:
        return torch.zeros_like(v)
    if act == 1:
        return v * scale
    sel = v if grad == 0 else _d(ref)
    return torch.where(sel > 0, v, v * alpha) * scale


def lincomb(x, z, a, b):
    return float(a) * _d(x) + float(b) * _d(z)


def scale_dev(x, s, c):
    return _d(x) * (float(c) * _d(s)[0])


def pixelnorm(x, M, K):
    x = _d(x).view(M, K)
    return x * torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-8)


def nhwc_scale(x, s, N, HW, C):
    return _d(x).view(N, HW, C) * _d(s).view(N, 1, C)


def nhwc_dot(a, b, N, HW, C, b_per_channel):
    a = _d(a).view(N, HW, C)
    b = _d(b).view(N, HW, C) if b_per_channel else _d(b).view(N, HW, 1)
    return (a * b).sum(1)


def sumsq(x, scale):
    x = _d(x)
    return float(scale) * (x * x).sum()


def mbstd_forward(x, B, P, C, Cp):
    """_minibatch_stddev_layer on [B][P][C] -> [B][P][Cp]: group G = min(B, 4), sample b = g * M + m; channel C = the
    mean over (p, c) of sqrt(var_g + 1e-8) (biased), channels above C = 0."""
    G = min(B, 4)
    M = B // G
    x = x.view(B, P, C)
    s = torch.sqrt(x.view(G, M, P, C).var(0, unbiased=False) + 1e-8).mean((1, 2))   # [M]
    chan = s.repeat(G).view(B, 1, 1).expand(B, P, 1)
    pad = torch.zeros(B, P, Cp - C - 1, dtype=x.dtype, device=x.device)
    return torch.cat([x, chan, pad], 2)


def mbstd(mode, x, B, P, C, Cp, gy=None, h=None):
    """Mode 0: the forward.  Mode 1: d/dx <forward(x), gy>.  Mode 2: (d/dx, d/dgy) of <mode-1 result, h>: float64
    double-backward autograd of the forward."""
    xd = _d(x).view(B, P, C).detach().requires_grad_(mode > 0)
    if mode == 0:
        return mbstd_forward(xd, B, P, C, Cp)
    gyd = _d(gy).view(B, P, Cp).detach().requires_grad_(mode == 2)
    y = mbstd_forward(xd, B, P, C, Cp)
    gx = torch.autograd.grad(y, xd, gyd, create_graph=(mode == 2))[0]
    if mode == 1:
        return gx.detach()
    gx2, ggy = torch.autograd.grad(gx, (xd, gyd), _d(h).view(B, P, C))
    return gx2, ggy
