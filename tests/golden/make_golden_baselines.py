#!/usr/bin/env python
"""Generate tests/golden/baselines.npz: the reference's baseline training modes (std / aug / aug_both with the CR / bCR
penalties, HorizontalFlipRandomCrop and DiffAugment) on small seeded inputs.

Runs ONLY in the build container (imports the read-only reference through _refshim.py; the HorizontalFlipRandomCrop values
of the reference's configs/defaults/augment.gin are bound from here).  Data only; the reference never travels.

Augmentation part: the reference's layers on 8-bit-valued images (they compress), with ``torch.bernoulli`` / ``torch.randint``
/ ``torch.rand`` wrapped to record what was drawn: seed, draws, input, output per case.
Step part, in FLOAT64 (the reference's own float32 run of the plain std step lands a LeakyReLU unit on the other side of
zero than float64 does, which moves its trunk gradients by 2.5 - 2.9e-3 of their norm, more than the 1e-3 the step tests
allow; the augmentations inside the steps run in float32, as they draw in the dtype of their input):
reference D_SNDCGAN filled by ``O.det_fill(seed=1234)`` (G: seed 4321, as the other sndcgan fixtures), N = 6,
lbd = lbd2 = 10, nonsat: the D-steps std+none, std+cr+hfrt, std+bcr+hfrt, aug+hfrt, aug_both+diffaug and the
aug_both+diffaug G-step; for each the losses, d_real, d_gen, the penalty, the parameter gradients of the GAN loss and of
the penalty SEPARATELY (norm of every tensor; the tensor itself up to 8192 entries, else its first 512), u / v after.

    python tests/golden/make_golden_baselines.py
"""
import contextlib
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()
_refshim.bind('HorizontalFlipRandomCrop', max_pixels=4, width=32, padding_mode='reflection')
from oracle import contrad_oracle as O  # noqa: E402

torch.set_num_threads(8)
N, LBD, LBD2 = 6, 10.0, 10.0


@contextlib.contextmanager
def recorded(draws):
    """Record, in order, what torch.bernoulli / torch.randint / torch.rand return inside the block."""
    orig = {k: getattr(torch, k) for k in ('bernoulli', 'randint', 'rand')}

    def wrap(name):
        def fn(*a, **k):
            v = orig[name](*a, **k)
            draws.append((name, v.clone()))
            return v
        return fn
    for k in orig:
        setattr(torch, k, wrap(k))
    try:
        yield
    finally:
        for k, v in orig.items():
            setattr(torch, k, v)


def images8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed)).float() / 255.0


def hfrt_block(draws):
    """{sign, kx, ky, 0} rows from the recorded (bernoulli, randint) pair of one HorizontalFlipRandomCrop call."""
    (n0, bern), (n1, shift) = draws
    assert n0 == 'bernoulli' and n1 == 'randint'
    P = torch.zeros(bern.shape[0], 4)
    P[:, 0] = bern * 2 - 1
    P[:, 1:3] = shift.float()
    return P


def diffaug_block(draws, policy, B):
    P = torch.zeros(B, 8)
    it = iter(draws)
    for stage in policy.split(','):
        if stage == 'color':
            r = [next(it) for _ in range(3)]
            assert all(n == 'rand' for n, _ in r)
            P[:, 0] = (r[0][1] - 0.5).view(B); P[:, 1] = (r[1][1] * 2).view(B); P[:, 2] = (r[2][1] + 0.5).view(B)
        else:
            r = [next(it) for _ in range(2)]
            assert all(n == 'randint' for n, _ in r)
            col = 3 if stage == 'translation' else 5
            P[:, col] = r[0][1].view(B).float(); P[:, col + 1] = r[1][1].view(B).float()
    assert next(it, None) is None
    return P


def gen_augment(out):
    import augment as A
    for tag, W, m, B, seed in (('hfrt32', 32, 4, 5, 101), ('hfrt8', 8, 7, 5, 102), ('hfrt8m4', 8, 4, 5, 103)):
        layer = A.HorizontalFlipRandomCrop() if tag == 'hfrt32' else \
            A.HorizontalFlipRandomCrop(max_pixels=m, width=W, padding_mode='reflection')
        assert layer.max_pixels == m and layer.width == W
        x = images8((B, 3, W, W), seed)
        draws = []
        torch.manual_seed(seed)
        with recorded(draws):
            y = layer(x)
        out.update({tag + '/seed': seed, tag + '/m': m, tag + '/x': x, tag + '/y': y, tag + '/P': hfrt_block(draws)})
    xd = images8((3, 3, 16, 12), 104)
    out['diffaug/x'] = xd
    for k, policy in enumerate(('color', 'translation', 'cutout', 'color,cutout', 'color,translation,cutout')):
        layer = A.DiffAugLayer(policy=policy)
        draws = []
        torch.manual_seed(200 + k)
        with recorded(draws):
            y = layer(xd)
        tag = 'diffaug/' + policy
        out.update({tag + '/seed': 200 + k, tag + '/y': y, tag + '/P': diffaug_block(draws, policy, 3)})
    assert A.diffaug().policy == 'color,cutout'


def put_grads(out, tag, named, grads):
    for (k, _), g in zip(named, grads):
        if g is None:                                   # a parameter the term does not reach (the projection heads)
            out[tag + 'none/' + k] = 1
            continue
        out[tag + 'gradnorm/' + k] = g.norm()
        if g.numel() <= 8192:
            out[tag + 'grad/' + k] = g
        else:
            out[tag + 'gradhead/' + k] = g.reshape(-1)[:512]


def gen_steps(out):
    import augment as A
    from importlib import import_module
    from models.gan import get_architecture
    sd = O.det_fill(O.sndcgan_d_param_shapes(), seed=1234)
    gsd = O.det_fill(O.sndcgan_g_param_shapes(), seed=4321)

    def fresh():
        G, D = get_architecture('sndcgan', (32, 32, 3))
        D.load_state_dict({k: v.clone() for k, v in sd.items()})
        gfull = dict(G.state_dict()); gfull.update({k: v.clone() for k, v in gsd.items()}); G.load_state_dict(gfull)
        return G.double().train(), D.double().train()

    x = images8((N, 3, 32, 32), 300).double()
    z = (torch.rand(N, 128, generator=torch.Generator().manual_seed(301)) * 2 - 1).double()

    def in_fp32(layer):         # the layers draw in the dtype of their input: float32 draws, as a training run makes them
        return lambda t: layer(t.float()).double()
    G, _ = fresh()
    with torch.no_grad():
        fake = G(z)
    out.update({'step/x': x, 'step/z': z, 'step/fake': fake, 'step/N': N, 'step/lbd': LBD, 'step/lbd2': LBD2})
    options = {'loss': 'nonsat', 'lbd': LBD, 'lbd2': LBD2}
    cases = (('std+none', 'std', 'none', 'none'), ('std+cr+hfrt', 'std', 'cr', 'hfrt'), ('std+bcr+hfrt', 'std', 'bcr', 'hfrt'),
             ('aug+hfrt', 'aug', 'none', 'hfrt'), ('aug_both+diffaug', 'aug_both', 'none', 'diffaug'))
    for k, (tag, mode, penalty, aug) in enumerate(cases):
        mod = import_module('training.gan.' + mode)
        _, D = fresh()
        P = Namespace(penalty=penalty, augment_fn=in_fp32(A.get_augment(mode=aug)))
        seed = 400 + k
        draws = []
        torch.manual_seed(seed)
        with recorded(draws):
            d_loss, aux = mod.loss_D_fn(P, D, options, x, fake)
        named = list(D.named_parameters())
        params = [p for _, p in named]
        t = 'step/' + tag + '/'
        out.update({t + 'seed': seed, t + 'd_loss': d_loss, t + 'penalty': aux['penalty'].reshape(()),
                    t + 'd_real': aux['d_real'], t + 'd_gen': aux['d_gen']})
        has_pen = aux['penalty'].requires_grad
        put_grads(out, t + 'gan/', named, torch.autograd.grad(d_loss, params, retain_graph=has_pen, allow_unused=True))
        if has_pen:
            gp = torch.autograd.grad(aux['penalty'], params, allow_unused=True)
            put_grads(out, t + 'pen/', named, gp)
            print('  %-18s penalty %.5f' % (tag, aux['penalty'].item()))
        if aug == 'hfrt':
            out[t + 'P'] = hfrt_block(draws)
        elif aug == 'diffaug':
            out[t + 'P'] = diffaug_block(draws, 'color,cutout', 2 * N)
        for name, v in D.state_dict().items():
            if name.endswith('weight_u'):
                out[t + 'after/' + name] = v
            elif name.endswith('weight_v'):
                out[t + 'afterhead/' + name] = v[:512]
        print('  %-18s d_loss %.5f d_real %.5f d_gen %.5f' % (tag, d_loss.item(), aux['d_real'].item(), aux['d_gen'].item()))

    # generator step of aug_both + diffaug (gradient through the augmentation into G)
    mod = import_module('training.gan.aug_both')
    G, D = fresh()
    for p in D.parameters():
        p.requires_grad = False
    P = Namespace(penalty='none', augment_fn=in_fp32(A.get_augment(mode='diffaug')))
    gen = G(z)
    draws = []
    torch.manual_seed(450)
    with recorded(draws):
        g_loss = mod.loss_G_fn(P, D, options, None, gen)
    named = list(G.named_parameters())
    t = 'gstep/'
    out.update({t + 'seed': 450, t + 'g_loss': g_loss, t + 'P': diffaug_block(draws, 'color,cutout', N)})
    put_grads(out, t, named, torch.autograd.grad(g_loss, [p for _, p in named], allow_unused=True))
    print('  G-step g_loss %.5f' % g_loss.item())


def main():
    out = {}
    gen_augment(out)
    gen_steps(out)
    blob = {}
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu()
            v = v.float() if v.dtype == torch.float64 else v      # computed in float64, stored rounded to float32
        blob[k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(HERE, 'baselines.npz')
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), 'bytes', len(blob), 'arrays')
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == '__main__':
    main()
