"""Counterpart of the reference's ``penalty.py``: ``compute_penalty(mode, **kwargs)`` for the baseline training modes.

``cr`` (consistency regularisation) and ``bcr`` (its balanced form) call the discriminator a SECOND time on the augmented
batch, as the reference does (penalty.py:45-58).  The two calls are not merged into one batch: in train mode every call
advances the spectral-norm power iteration, and the second call has to see the ``u`` / ``v`` the first one left.  The
squared-difference term and both of its gradients come from one launch (csrc/baseline_aug.hip: consistency_kernel).

``gp`` (WGAN-GP's gradient penalty) is a further D call, on the interpolated batch and on the discriminator's second-order
form (``D.second_order()``): its input gradient is taken with ``create_graph=True`` and the penalty's backward runs the
double backward of the any-order node family into ``weight_orig`` (csrc/gp.hip: the interpolation, the penalty and its
cotangent).
"""
import inspect

import torch
from torch.autograd.function import once_differentiable

from . import autograd_ops as A
from . import ops
from .hostio import upload


class _Consistency(torch.autograd.Function):
    """lbd0 * mean((a - b)^2 over rows [0, n0)) + lbd1 * mean(... over rows [n0, n0 + n1)) on (n, 1) logit columns."""

    @staticmethod
    def forward(ctx, a, b, n0, n1, lbd0, lbd1):
        out, ga, gb = ops.consistency(a.float(), b.float(), n0, n1, lbd0, lbd1)
        ctx.save_for_backward(ga, gb)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        ga, gb = ctx.saved_tensors
        return ga * g, gb * g, None, None, None, None


def call_with_accepted_args(fn, **kwargs):
    """utils.call_with_accepted_args of the reference: pass the keyword arguments ``fn`` names."""
    accepted = inspect.signature(fn).parameters
    return fn(**{k: v for k, v in kwargs.items() if k in accepted})


def no_penalty(images):
    return torch.zeros(1, device=images.device)


class _GradientPenalty(torch.autograd.Function):
    """lbd * mean_n (||grad_n||_2 - 1)^2 on an (N, C, H, W) input gradient; value, norms and the cotangent d out / d grad
    from one call (csrc/gp.hip), the backward scales the saved cotangent."""

    @staticmethod
    def forward(ctx, grad, lbd):
        out, _norms, cot = ops.gp_penalty(grad.contiguous().float(), lbd)
        ctx.save_for_backward(cot)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cot, = ctx.saved_tensors
        return cot * g, None


def gradient_penalty(D, images, gen_images, lbd):
    """penalty.py:16-42.  ``alpha`` is drawn on the host where the reference draws it (torch.rand(N, 1, 1, 1), CPU
    generator) and handed over as an (N,) block; D(xhat) is one more discriminator call in the caller's mode, i.e. one
    more power iteration in train mode."""
    second_order = getattr(D, 'second_order', None)
    if second_order is None:
        raise NotImplementedError("penalty 'gp' (penalty.py:16-42) differentiates the input gradient of D: it needs a "
                                  "second-order path through the discriminator, which %s does not offer (no "
                                  "second_order())" % type(D).__name__)
    N = images.size(0)
    alpha = upload(torch.rand(N, 1, 1, 1).view(N), images.device)
    xhat = ops.gp_interpolate(images.detach().contiguous().float(), gen_images.detach().contiguous().float(), alpha)
    xhat.requires_grad_()
    with second_order():
        d = D(xhat)
    with A.input_grad_only():       # this backward is asked for d / d xhat only: skip the parameter gradients
        grad, = torch.autograd.grad(outputs=d.sum(), inputs=xhat, create_graph=True, retain_graph=True)
    return _GradientPenalty.apply(grad, float(lbd))


def consistency(D, P, images, d_real, lbd):
    """penalty.py:45-47."""
    d_aug = D(P.augment_fn(images))
    return _Consistency.apply(d_real, d_aug, images.size(0), 0, lbd, 0.0)


def balanced_consistency(D, P, all_images, d_real, d_gen, lbd, lbd2, d_all=None):
    """penalty.py:50-58.  ``d_all`` (optional): the (2N, 1) logits d_real and d_gen are the halves of, which saves
    concatenating them again."""
    d_aug_all = D(P.augment_fn(all_images))
    N = all_images.size(0) // 2
    if d_all is None:
        d_all = torch.cat([d_real, d_gen], dim=0)
    return _Consistency.apply(d_all, d_aug_all, N, all_images.size(0) - N, lbd, lbd2)


def compute_penalty(mode='none', **kwargs):
    """penalty.py:61-69."""
    _mapping = {'none': no_penalty, 'gp': gradient_penalty, 'cr': consistency, 'bcr': balanced_consistency}
    return call_with_accepted_args(_mapping[mode], **kwargs)
