#!/usr/bin/env python
"""Generate tests/golden/cddls_snresnet18.npz: the reference's own ``_sample_cddls`` (test_gan_sample_cddls.py:57-76) in
float64 on its ``get_architecture('snresnet18', (32, 32, 3))`` (G_SNDCGAN + D_SNResNet18).

Runs ONLY in the build container, like make_golden_cddls.py, whose recording wrappers (``load_script``, ``run``) it uses.
The networks are filled by ``cddls_snresnet_ref64.fixture_networks`` (``O.det_fill`` plus converged spectral-norm
vectors), the classifier is a seeded ``LinearWrapper(512, 10)`` with float32-representable rows; N = 4, three steps,
classes 3 and 7 on the SAME draws.  Stored: what cddls.npz stores.  Printed per step and class: the norms of the drift
``0.5 eps g_z`` and of the noise ``sigma_n sqrt(eps) n`` (within a factor 10 of each other by the choice of the constants
below) and the number of entries of z on the clamp (none).  Data only; the reference never travels.

    python tests/golden/make_golden_cddls_snresnet.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_cddls as M  # noqa: E402  (installs the reference shim)
import cddls_snresnet_ref64 as RS  # noqa: E402

# seed 89: the first from 78 up at which every step's float64 run keeps clear of the LeakyReLU kinks (the condition of
# test_cddls_snresnet_ref64_cpu.py::test_same_region_comparisons_are_well_conditioned) and no entry of z reaches the clamp
N, STEPS, CLASSES, SEED = M.N, M.STEPS, M.CLASSES, 89
# chosen so that drift and noise have the same order in an increment of z (printed below, asserted by the CPU test)
EPS, LBD, SIGMA_N = 0.1, 1000.0, 0.001


def build():
    from models.gan import get_architecture
    from models.gan.base import LinearWrapper
    G, D = get_architecture('snresnet18', (32, 32, 3))
    gsd, dsd = RS.fixture_networks()
    G.double(); D.double()
    gfull = dict(G.state_dict())
    gfull.update(gsd)
    G.load_state_dict(gfull)
    D.load_state_dict(dsd)
    torch.manual_seed(56)
    head = LinearWrapper(512, 10)
    with torch.no_grad():           # float32-representable, and only the rows of CLASSES are stored
        head.weight.copy_(head.weight.float().double()); head.bias.copy_(head.bias.float().double())
    D.classifier = head
    G.double().eval()
    D.double().eval()
    return G, D, head


def main():
    torch.set_default_dtype(torch.float64)
    mod = M.load_script()
    G, D, head = build()
    M.EPS, M.LBD, M.SIGMA_N, M.SEED = EPS, LBD, SIGMA_N, SEED          # M.run reads its module's constants
    blob = {'eps': EPS, 'lbd': LBD, 'sigma_n': SIGMA_N, 'classes': np.array(CLASSES),
            'head.weight_rows': head.weight.detach()[list(CLASSES)].numpy().astype(np.float32),
            'head.bias_rows': head.bias.detach()[list(CLASSES)].numpy().astype(np.float32)}
    for y in CLASSES:
        a, b = M.run(mod, G, D, y, STEPS), M.run(mod, G, D, y, STEPS + 1)
        assert torch.equal(a['z0'], b['z0']) and all(torch.equal(p, q) for p, q in zip(a['randn'], b['randn']))
        if 'z0' not in blob:
            blob['z0'] = a['z0'].numpy().astype(np.float32)
            blob['z2_0'] = a['randn'][0].numpy().astype(np.float32)
            blob['n'] = np.stack([a['randn'][1 + 2 * k].numpy() for k in range(STEPS)]).astype(np.float32)
            blob['n2'] = np.stack([a['randn'][2 + 2 * k].numpy() for k in range(STEPS)]).astype(np.float32)
        else:       # both classes run on the same draws
            assert np.array_equal(blob['z0'], a['z0'].numpy()) and np.array_equal(blob['z2_0'], a['randn'][0].numpy())
        zs = torch.stack(a['clamp'][:STEPS])
        z2s = [b['randn_arg'][2 + 2 * k] for k in range(STEPS + 1)]           # z2_0 .. z2_3
        assert torch.equal(z2s[0], a['randn'][0])
        blob['y%d.z' % y] = zs.numpy()
        blob['y%d.z2_last' % y] = z2s[STEPS].numpy()
        blob['y%d.z2_sums' % y] = torch.stack([t.reshape(N, -1).sum(1) for t in z2s]).numpy()
        blob['y%d.images' % y] = a['images'].numpy()
        blob['y%d.e_sum' % y] = np.array(a['e_sum'])
        noise = [SIGMA_N * EPS ** 0.5 * a['randn'][1 + 2 * k] for k in range(STEPS)]
        drift = [(zs[k] - (zs[k - 1] if k else a['z0'])) - noise[k] for k in range(STEPS)]
        print('class', y, 'e_sum', a['e_sum'], 'entries of z on the clamp per step', [(t.abs() == 1).sum().item() for t in zs],
              '|drift|', [d.norm().item() for d in drift], '|noise|', [t.norm().item() for t in noise])
    path = os.path.join(HERE, 'cddls_snresnet18.npz')
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
