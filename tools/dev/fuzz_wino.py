"""dev: random shapes through the forced Winograd entry points (F(4x4,3x3) both cout-block widths, F(2x2,3x3), the strided kernels)
against the float64 references of the test suite (tests/conv_ref64.py: im2col GEMM on float64 CUDA tensors); prints the worst
max-norm and rel-L2 error per kernel family, on the scale of tests/test_conv_paths_gpu.py.  usage: python tools/dev/fuzz_wino.py [cases] [seed]"""
import os
import random
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, 'tests'))
import conv_ref64 as R  # noqa: E402
from contrad_amd import ops  # noqa: E402


def main(cases=60, seed=0):
    rnd = random.Random(seed)
    dev = torch.device('cuda')
    worst = {}
    for it in range(cases):
        fam = rnd.choice(['f44', 'f44', 'f44', 'f22', 'k4s2', 'k3s2'])
        g = torch.Generator().manual_seed(seed * 1000 + it)
        if fam in ('f44', 'f22'):
            H = rnd.choice([4, 8, 16, 32, 64]) if fam == 'f44' else rnd.choice([4, 8, 16, 32])
            W = H if H < 32 else rnd.choice([32, 64])
            if fam == 'f44' and W >= 32 and H < 16:
                H = 16
            C = rnd.choice([32, 64, 96, 128]) if fam == 'f44' else rnd.choice([16, 32, 48, 64])
            K = rnd.choice([32, 64, 96, 128, 160]) if fam == 'f44' else rnd.choice([64, 128])
            N = rnd.choice([1, 2, 3, 5, 9, 33, 70])
            mode = rnd.choice([0, 1])
            x = torch.randn(N, H, W, C if mode == 0 else K, generator=g)
            w = torch.randn(K, C, 3, 3, generator=g) * 0.1
            if mode == 1 and ((fam == 'f44' and (K % 32 or C % 32)) or (fam == 'f22' and (K % 16 or C % 64))):
                continue
            wp = ops.pack_weight(w).to(dev)
            try:
                y = ops.conv2d_wino(mode, x.to(dev), wp, C, K, f44=(fam == 'f44'))
            except RuntimeError:
                continue
            xd, wd = x.to(dev), w.to(dev)
            ref = R.fwd(xd, wd, None, 1, 1) if mode == 0 else R.dgrad(xd, wd, (H, W), 1, 1)
            key = '%s mode %d%s' % (fam, mode, ' (32-wide)' if fam == 'f44' and (((K if mode == 0 else C) % 64) or W == 4) else '')
        elif fam == 'k4s2':
            G = rnd.choice([4, 8, 16]); C = rnd.choice([8, 16, 24, 32]); K = rnd.choice([64, 128]); N = rnd.choice([1, 3, 9, 40])
            x = torch.randn(N, 2 * G, 2 * G, C, generator=g); w = torch.randn(K, C, 4, 4, generator=g) * 0.1
            y = ops.conv2d_wino(0, x.to(dev), ops.pack_weight(w).to(dev), C, K, k4s2=True)
            ref = R.fwd(x.to(dev), w.to(dev), None, 2, 1)
            key = 'k4s2 forward'
        else:
            G = rnd.choice([4, 8, 16, 32, 64]); C = rnd.choice([16, 32, 48]); K = rnd.choice([64, 128]); N = rnd.choice([1, 2, 5, 9, 40])
            x = torch.randn(N, 2 * G + 1, 2 * G + 1, C, generator=g); w = torch.randn(K, C, 3, 3, generator=g) * 0.1
            y = ops.conv2d_wino(0, x.to(dev), ops.pack_weight(w).to(dev), C, K, k3s2=True)
            ref = R.fwd(x.to(dev), w.to(dev), None, 2, 0)
            key = 'k3s2 forward'
        e, e2 = R.errors(y, ref)
        n, m, m2 = worst.get(key, (0, 0.0, 0.0))
        worst[key] = (n + 1, max(m, e), max(m2, e2))
        assert e < 1e-4, (key, tuple(x.shape), C, K, e)
    for k in sorted(worst):
        print('%-28s %3d cases  worst max-norm %.2e  rel-L2 %.2e' % (k, worst[k][0], worst[k][1], worst[k][2]))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
