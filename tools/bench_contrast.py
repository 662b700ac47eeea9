"""Dev tool: the time of one evaluation of the contrastive diagnostics (contrad_amd/contrast.py) at the hook's default size,
by stage.  A record behind profiles/contrast.txt; no threshold.

    python tools/bench_contrast.py [OUT.txt]      # n = 2000, blocks of 512, sndcgan at 32 x 32, --aug simclr

Times are HIP-event medians over repeated windows with the min - max spread (tools/bench_knn.py's ``windows``), one process.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import contrast, features, lineval, ops  # noqa: E402
from contrad_amd.augment import SimCLRAugment  # noqa: E402
from contrad_amd.models.gan import get_architecture  # noqa: E402

if __name__ == '__main__':
    dev = torch.device('cuda', 0)
    n, batch, temp, t = 2000, 512, 0.1, 2.0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    D = features.freeze(get_architecture('sndcgan', (32, 32, 3))[1].to(dev))
    x = torch.from_numpy(lineval.synthetic_set(0, 10, n, 1)['x_train']).to(dev)
    aug = SimCLRAugment(scale=(0.2, 1.0)).to(dev)
    out = contrast.contrast_of(D, x, aug, n, batch, temp, t, seed=1)
    emit('contrast_of n = %d, blocks of %d, sndcgan 32 x 32, simclr: %s' % (n, batch, contrast.log_line(0, out).split('] ', 1)[1]))
    emit(fmt('contrast_of: all (views, 2 x %d forwards, statistics, one read)' % n, windows(lambda: contrast.contrast_of(D, x, aug, n, batch, temp, t, seed=1), iters=1, reps=5, warm=1)))
    g = torch.Generator(device='cpu').manual_seed(0)
    pA, pB = (features.normalize_rows(torch.randn(n, 128, generator=g).to(dev)) for _ in range(2))
    fA, fB = (features.normalize_rows(torch.randn(n, 8192, generator=g).to(dev)) for _ in range(2))
    emit(fmt('  contrast_stats on normalised rows (d 128 and 8192): everything after the forwards',
             windows(lambda: contrast.contrast_stats(pA, pB, batch, temp, t, normalize=False, fA=fA, fB=fB), iters=1, reps=5, warm=1)))
    S = next(features.similarity_chunks(pA, features.bank_of(pA)))[1]
    cell = torch.zeros(1, dtype=torch.float64, device=dev)
    emit(fmt('  gauss_sums on one (%d, %d) chunk of S: two launches' % (S.shape[0], n), windows(lambda: ops.gauss_sums(S, n, t, self0=0, out=cell))))
    z = torch.cat([pA[:batch], pB[:batch]])
    emit(fmt('  block_ranks of one block of %d rows: bank, GEMM, diagonal, thresholds, one count pass' % (2 * batch), windows(lambda: contrast.block_ranks(z, batch))))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])) or '.', exist_ok=True)
        with open(sys.argv[1], 'a') as f:
            f.write('\n'.join(lines) + '\n')
