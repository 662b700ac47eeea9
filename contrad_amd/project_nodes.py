"""The autograd pieces of the StyleGAN2 projector (contrad_amd/project.py).

* ``ModconvEpilogueNoiseFn``: ``autograd_ops.ModconvEpilogueFn`` whose backward also returns the gradient of the noise map
  (``ops.proj_noise_grad``).  Training never asks for it -- the maps are fresh draws there -- so the training node returns None.
* ``styled_conv_noise``: ``Generator._styled_conv_grad`` ending in that node.  The generator's own method stays as it is (the
  training path is pinned bit for bit), so its dozen lines are restated here.
* ``image_end`` / ``noise_reg_``: the two loss ends as plain functions.  They are ends: each returns its rows and the gradient
  (or adds it in place); nothing differentiates through them.
"""
import torch
from torch.autograd import Function

from . import autograd_ops as A
from . import ops


class ModconvEpilogueNoiseFn(Function):
    """out = sqrt2 * lrelu_0.2(y * demod[n,k] + noise_w * noise[n,h,w] + bias[k]) as ``ModconvEpilogueFn`` computes it (same
    launch, same bits); the backward returns the gradients of the conv output, the demodulation factors, the noise map, the
    noise strength and the bias, each only where ``ctx.needs_input_grad`` asks.  First-order."""

    @staticmethod
    def forward(ctx, y, demod, noise, noise_w, bias):
        y, demod, noise = A._cont(y), A._cont(demod), A._cont(noise)
        out = ops.modconv_epilogue_(y, demod, noise, noise_w, bias, out=torch.empty_like(y))
        ctx.save_for_backward(y, demod, noise, noise_w, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, demod, noise, noise_w, out = ctx.saved_tensors
        g_pre = ops.fused_bias_act(A._cont(g), None, out, 3, 1, 0.2, A.SQRT2)
        gy = ops.nhwc_scale(g_pre, demod) if ctx.needs_input_grad[0] else None
        gdemod = ops.nhwc_dot(g_pre, y) if ctx.needs_input_grad[1] else None
        gnoise = ops.proj_noise_grad(g_pre, noise_w.detach().reshape(1)) if ctx.needs_input_grad[2] else None
        gnw = ops.nhwc_dot(g_pre, noise, per_channel=False).sum().reshape(1) if ctx.needs_input_grad[3] else None
        gb = ops.colstats(g_pre.view(-1, g_pre.shape[-1]))[0] if ctx.needs_input_grad[4] else None
        return gy, gdemod, gnoise, gnw, gb


def styled_conv_noise(G, layer, x, w_lat, noise, c):
    """``Generator._styled_conv_grad`` with the noise map as a differentiable input (``noise``: (B, 1, H', W') given)."""
    mc = layer.conv
    B, H, W, _ = x.shape
    s = G._style(mc, w_lat, c)
    d = A.Conv2dFn.apply((s * s).view(B, 1, 1, -1), c['wsq'][mc], (mc.out_channel, 1, 1, 1, 0)).view(B, -1)
    demod = torch.rsqrt(d + 1e-8)
    xm = A.NhwcScaleFn.apply(x, s)
    wp = c['packed'][c['conv'][mc]]
    if mc.upsample:
        y = A.ConvDgradFn.apply(xm, wp, (B, 2 * H + 1, 2 * W + 1, mc.out_channel), (mc.in_channel, 3, 3, 2, 0))
        p0, p1 = mc.blur.pad
        y = A.UpFirDn2dFn.apply(y, mc.blur.kernel, 1, 1, (p0, p1, p0, p1))
    else:
        y = A.Conv2dFn.apply(xm, wp, (mc.out_channel, 3, 3, 1, 1))
    noise = noise.expand(B, 1, y.shape[1], y.shape[2]).contiguous()
    return ModconvEpilogueNoiseFn.apply(y, demod, noise, layer.noise.weight, layer.activate.bias)


def image_end(x, target, level_weights, pix=None, gx=None, partial=None):
    """(pix rows (L, N), d sum loss_pix / d x) of the image ``x`` the differentiable path painted (``ops.proj_image_end`` on
    its values); the caller sends the gradient into the graph with ``x.backward(gx)``."""
    return ops.proj_image_end(x.detach().contiguous(), target, level_weights, pix=pix, gx=gx, partial=partial)


def noise_reg_(noise, grad, reg_weight, reg=None, scratch=None):
    """reg (N,) of one map set; ``grad`` (the maps' ``.grad``) receives ``+= reg_weight * d reg / d noise`` in place."""
    return ops.proj_noise_reg(noise.detach(), grad, reg_weight, reg=reg, scratch=scratch)
