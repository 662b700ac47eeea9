"""Standard GAN losses -- counterpart of training/gan/std.py (``--mode=std``, with ``--penalty=none|cr|bcr``).

One D call on [reals | fakes] (2N images), the GAN term and its gradient from one fused launch (csrc/baseline_aug.hip:
gan_d_loss_2n_kernel), the penalty from ``contrad_amd.penalty``."""
import torch

from ... import ops
from ...penalty import compute_penalty
from .contrad import _GanGLoss

D_LOSSES = ('nonsat', 'wgan', 'hinge', 'lsgan')


class _GanDLoss2N(torch.autograd.Function):
    """std.py:14-25 on logits (2N,1), reals first: returns [loss, mean d_real, mean d_gen]."""

    @staticmethod
    def forward(ctx, d_all, N, kind):
        out, grad = ops.gan_d_loss_2n(d_all.contiguous(), N, kind)
        ctx.save_for_backward(grad)
        loss, d_real, d_gen = out.unbind(0)
        ctx.mark_non_differentiable(d_real, d_gen)
        return loss, d_real, d_gen

    @staticmethod
    def backward(ctx, g, _g1, _g2):
        grad, = ctx.saved_tensors
        return grad * g, None, None


def d_loss_and_penalty(P, D, options, images, gen_images, all_images, d_all, losses):
    """The part the three baseline modes share: GAN term on the (2N,1) logits + compute_penalty on the UN-augmented batch
    (std.py:14-36)."""
    if options['loss'] not in losses:
        raise NotImplementedError()
    N = images.size(0)
    d_loss, m_real, m_gen = _GanDLoss2N.apply(d_all, N, options['loss'])
    penalty = compute_penalty(P.penalty, P=P, D=D, all_images=all_images, images=images, gen_images=gen_images,
                              d_real=d_all[:N], d_gen=d_all[N:], d_all=d_all, lbd=options['lbd'], lbd2=options['lbd2'])
    return d_loss, {"penalty": penalty, "d_real": m_real, "d_gen": m_gen}


def loss_D_fn(P, D, options, images, gen_images):
    gen_images = gen_images.detach()
    all_images = torch.cat([images, gen_images], dim=0)
    return d_loss_and_penalty(P, D, options, images, gen_images, all_images, D(all_images), D_LOSSES)


def loss_G_fn(P, D, options, images, gen_images):
    """std.py:39-48: 'nonsat' -> softplus(-d), 'lsgan' -> 0.5 (d - 1)^2, anything else -> -d (means)."""
    kind = options['loss'] if options['loss'] in ('nonsat', 'lsgan') else 'wgan'
    return _GanGLoss.apply(D(gen_images), kind)
