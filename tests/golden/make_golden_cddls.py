#!/usr/bin/env python
"""Generate tests/golden/cddls.npz: the reference's own ``_sample_cddls`` (test_gan_sample_cddls.py:57-76) in float64.

Runs ONLY in the build container (imports the read-only reference through _refshim.py; ``torchvision``, ``datasets`` and
``tqdm``, which the script imports at its top and the function never uses, are in-memory stubs).  The reference's
G_SNDCGAN / D_SNDCGAN are filled by ``cddls_ref64.fixture_networks`` (``O.det_fill``, seeds 4321 / 1234, as the other
sndcgan fixtures, plus converged spectral-norm vectors), the classifier is
a seeded ``LinearWrapper(8192, 10)``; N = 4, three steps, classes 3 and 7 from the SAME draws (z0, z2_0 and the noises are
stored once).  ``torch.randn_like`` and ``G.sample_latent`` are wrapped to record what they drew, rounded to
float32-representable values (half the bytes after compression: the fixture must stay under the size limit for
committed files); ``torch.clamp`` records z after every step, ``grad`` records the summed energy of every step.  z2
after step k is what step k + 1 hands to ``randn_like``, so every class runs twice from the same seed: three steps for
the images, four steps for z2 after the third.  Data only; the reference never travels.

    python tests/golden/make_golden_cddls.py
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()
from oracle import contrad_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import cddls_ref64 as R  # noqa: E402


def _stubs():
    tv, tvu = types.ModuleType('torchvision'), types.ModuleType('torchvision.utils')
    tvu.save_image = lambda *a, **k: None
    tv.utils = tvu
    tq = types.ModuleType('tqdm')
    tq.tqdm = lambda it, *a, **k: it
    ds = types.ModuleType('datasets')
    ds.get_dataset = lambda *a, **k: (None, None, (32, 32, 3))
    for name, mod in (('torchvision', tv), ('torchvision.utils', tvu), ('tqdm', tq), ('datasets', ds)):
        sys.modules.setdefault(name, mod)


N, STEPS, CLASSES, SEED = 4, 3, (3, 7), 77
# the fixture networks barely react to z (|g_z| ~ 2e-5 per entry): at these constants drift and noise have the same size in an
# increment of z, so a comparison of increments checks the gradient and the noise scaling alike
EPS, LBD, SIGMA_N = 0.1, 1000.0, 0.0005


def load_script():
    _stubs()
    spec = importlib.util.spec_from_file_location('_ref_cddls', os.path.join(_refshim.REFERENCE_ROOT,
                                                                            'test_gan_sample_cddls.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build():
    from models.gan import get_architecture
    from models.gan.base import LinearWrapper
    G, D = get_architecture('sndcgan', (32, 32, 3))
    gsd, dsd = R.fixture_networks()             # det_fill + converged spectral-norm vectors (see there)
    G.double(); D.double()
    gfull = dict(G.state_dict())
    gfull.update(gsd)
    G.load_state_dict(gfull)
    D.load_state_dict(dsd)
    torch.manual_seed(55)
    head = LinearWrapper(8192, 10)
    with torch.no_grad():           # float32-representable, and only the rows of CLASSES are stored
        head.weight.copy_(head.weight.float().double()); head.bias.copy_(head.bias.float().double())
    D.classifier = head
    G.double().eval()
    D.double().eval()
    return G, D, head


def run(mod, G, D, y, steps):
    rec = {'randn': [], 'clamp': [], 'e_sum': [], 'z0': None, 'randn_arg': []}
    o_randn, o_clamp, o_grad, o_latent = torch.randn_like, torch.clamp, mod.grad, G.sample_latent

    def randn_like(t, *a, **k):
        v = o_randn(t, *a, **k).float().double()
        rec['randn'].append(v.clone())
        rec['randn_arg'].append(t.detach().clone())
        return v

    def clamp(t, *a, **k):
        v = o_clamp(t, *a, **k)
        rec['clamp'].append(v.detach().clone())
        return v

    def grad(outputs, inputs, *a, **k):
        rec['e_sum'].append(float(outputs.item()))
        return o_grad(outputs=outputs, inputs=inputs, *a, **k)

    def sample_latent(n):
        rec['z0'] = o_latent(n).float().double()
        return rec['z0'].clone()

    P = argparse.Namespace(n_steps=steps, eps=EPS, lbd=LBD, sigma_n=SIGMA_N)
    torch.randn_like, torch.clamp, mod.grad, G.sample_latent = randn_like, clamp, grad, sample_latent
    try:
        torch.manual_seed(SEED)
        images = mod._sample_cddls(P, G, D, y, N)
    finally:
        torch.randn_like, torch.clamp, mod.grad, G.sample_latent = o_randn, o_clamp, o_grad, o_latent
    rec['images'] = images
    return rec


def main():
    torch.set_default_dtype(torch.float64)
    mod = load_script()
    G, D, head = build()
    blob = {'eps': EPS, 'lbd': LBD, 'sigma_n': SIGMA_N, 'classes': np.array(CLASSES),
            'head.weight_rows': head.weight.detach()[list(CLASSES)].numpy().astype(np.float32),
            'head.bias_rows': head.bias.detach()[list(CLASSES)].numpy().astype(np.float32)}
    for y in CLASSES:
        a, b = run(mod, G, D, y, STEPS), run(mod, G, D, y, STEPS + 1)
        assert torch.equal(a['z0'], b['z0']) and all(torch.equal(p, q) for p, q in zip(a['randn'], b['randn']))
        if 'z0' not in blob:
            blob['z0'] = a['z0'].numpy().astype(np.float32)
            blob['z2_0'] = a['randn'][0].numpy().astype(np.float32)
            blob['n'] = np.stack([a['randn'][1 + 2 * k].numpy() for k in range(STEPS)]).astype(np.float32)
            blob['n2'] = np.stack([a['randn'][2 + 2 * k].numpy() for k in range(STEPS)]).astype(np.float32)
        else:       # both classes run on the same draws
            assert np.array_equal(blob['z0'], a['z0'].numpy()) and np.array_equal(blob['z2_0'], a['randn'][0].numpy())
        # the three-step run clamps z three times, then the images; z2 before step k + 1 is randn_like's argument there
        zs = torch.stack(a['clamp'][:STEPS])
        z2s = [b['randn_arg'][2 + 2 * k] for k in range(STEPS + 1)]           # z2_0 .. z2_3
        assert torch.equal(z2s[0], a['randn'][0])
        blob['y%d.z' % y] = zs.numpy()
        blob['y%d.z2_last' % y] = z2s[STEPS].numpy()
        blob['y%d.z2_sums' % y] = torch.stack([t.reshape(N, -1).sum(1) for t in z2s]).numpy()
        blob['y%d.images' % y] = a['images'].numpy()
        blob['y%d.e_sum' % y] = np.array(a['e_sum'])
        print('class', y, 'e_sum', a['e_sum'], 'clamped entries per step', [(t.abs() == 1).sum().item() for t in zs],
              '|dz|', [(zs[k] - (zs[k - 1] if k else a['z0'])).norm().item() for k in range(STEPS)],
              '|s n|', [(SIGMA_N * EPS ** 0.5 * a['randn'][1 + 2 * k]).norm().item() for k in range(STEPS)])
    path = os.path.join(HERE, 'cddls.npz')
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
