"""Float64 restatements of the gradient penalty (the reference's penalty.py:16-42; csrc/gp.hip, contrad_amd/penalty.py) in
plain torch on the CPU -- none of this project's kernels, like baselines_ref64.py.

``interpolate`` and ``penalty`` (value, per-sample norms and the cotangent d value / d grad) are written out by hand;
``second_order_grads`` pulls the hand-written cotangent back through the graph of the discriminator's input gradient (a
float64 autograd graph built with ``create_graph=True``), which is what the penalty's backward does on the GPU.  The
SNDCGAN- and SNResNet18-shaped discriminators are the float64 model code the other step tests use (oracle.contrad_oracle, with
its imposed linear regions); the error measure is dstep_ref64.errors.  tests/test_gp_ref64_cpu.py checks all of it against
float64 autograd of the reference's own expression.
"""
import torch

from dstep_ref64 import errors  # noqa: F401  (max-norm, rel-L2) of a float32 result against float64
from oracle import contrad_oracle as O

f64 = torch.float64


def interpolate(x, g, alpha):
    """xhat[n] = alpha[n] x[n] + (1 - alpha[n]) g[n]; alpha (N,)."""
    a = alpha.to(f64).reshape(-1, 1, 1, 1)
    return a * x.to(f64) + (1.0 - a) * g.to(f64)


def penalty(grad, lbd):
    """grad (N, ...) -> (lbd mean_n (||grad_n|| - 1)^2, norms (N,), cot = d value / d grad); cot_n = 0 where the norm is 0
    (what torch's 2-norm backward returns there)."""
    g = grad.to(f64)
    N = g.shape[0]
    flat = g.reshape(N, -1)
    norms = flat.pow(2).sum(1).sqrt()
    value = lbd * (norms - 1.0).pow(2).sum() / N
    scale = torch.where(norms > 0, 2.0 * lbd * (norms - 1.0) / (N * norms.clamp_min(1e-300)), torch.zeros_like(norms))
    return value, norms, (flat * scale[:, None]).reshape(g.shape)


def input_gradient(d_fn, xhat):
    """(xhat with requires_grad, d D(xhat).sum() / d xhat as a differentiable float64 graph)."""
    xhat = xhat.detach().to(f64).requires_grad_()
    grad, = torch.autograd.grad(d_fn(xhat).sum(), xhat, create_graph=True)
    return xhat, grad


def second_order_grads(d_fn, params, x, g, alpha, lbd):
    """-> (value, norms, [d value / d p for p in params] (None where the penalty does not reach p)): the cotangent of
    ``penalty`` pulled back through the input-gradient graph."""
    _, grad = input_gradient(d_fn, interpolate(x, g, alpha))
    value, norms, cot = penalty(grad.detach(), lbd)
    grads = torch.autograd.grad(grad, params, grad_outputs=cot, allow_unused=True)
    return value, norms, list(grads)


def reference_expression(d_fn, x, g, alpha, lbd):
    """The reference's lines, on float64 tensors, left to autograd: (differentiable value, norms)."""
    _, grad = input_gradient(d_fn, interpolate(x, g, alpha))
    norms = grad.reshape(grad.shape[0], -1).norm(2, dim=1)
    return lbd * ((norms - 1) ** 2).mean(), norms


# ---- the two discriminators, float64, parameters from a state dict ---------------------------------------------------
FORWARDS = {'sndcgan': O.sndcgan_d_forward, 'snresnet18': O.snresnet18_forward}


def leaf_state(sd):
    """float64 copy of a state dict whose parameters (weight_orig, bias) are leaves that require grad."""
    out = {k: torch.as_tensor(v).detach().to(f64).clone() for k, v in sd.items()}
    for k in out:
        if k.endswith('weight_orig') or k.endswith('bias'):
            out[k].requires_grad_()
    return out


def d_logits(arch, sd, training, act_masks=None, hidden_masks=None):
    """x -> logits of the float64 discriminator; in train mode every call advances u / v in ``sd``, as a module does."""
    fwd = FORWARDS[arch]
    return lambda x: fwd(sd, x, sg_linear=False, training=training, act_masks=act_masks, hidden_masks=hidden_masks)[0]


def gp_step(arch, sd, x, fake, alpha, lbd, training=True, masks=None):
    """The 'gp' half of a std D-step on a leaf_state() dict: one D call on the interpolated batch (one power iteration in
    train mode) -> (value, norms, {parameter name: gradient or None}).  ``masks`` = (act_masks, hidden_masks) imposes the
    linear regions of that call."""
    am, hm = masks if masks is not None else (None, None)
    names = [k for k in sd if sd[k].requires_grad]
    value, norms, grads = second_order_grads(d_logits(arch, sd, training, am, hm), [sd[k] for k in names], x, fake, alpha,
                                             lbd)
    return value, norms, dict(zip(names, grads))
