"""Dev tool: one latent-recovery step (contrad_amd/recover.py) at batch 500, 32 x 32, with the cDDLS step of
tools/bench_cddls.py timed in the same process for scale.

    python tools/bench_recover.py            # pixel-only and sndcgan-feature steps, eager and hipGraph replay, then the cDDLS step
    python tools/bench_recover.py kernels    # 30 eager pixel-only steps, for `rocprofv3 --kernel-trace --stats -- python tools/bench_recover.py kernels`
    python tools/bench_recover.py kernels-feature   # the same with the sndcgan feature term

Times are HIP-event medians of 9 windows x 20 steps with the min - max spread (bench_cddls.windows).  There is no "before":
the parent has no such path.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cddls import BATCH, dev, networks, report, sampler, windows  # noqa: E402
from contrad_amd.recover import DEFAULT_STEPS, LatentRecovery  # noqa: E402


def recovery(G, D, feature, graph):
    S = LatentRecovery(G, BATCH, D=D if feature else None, lambda_feat=1.0 if feature else 0.0, graph=graph)
    S.set_targets(torch.rand(BATCH, 3, 32, 32, device=dev, generator=torch.Generator(device='cuda').manual_seed(2)))
    S.start(G.sample_latent(BATCH))
    return S


def main(mode='all'):
    G, D = networks('sndcgan')
    if mode in ('kernels', 'kernels-feature'):
        S = recovery(G, D, mode == 'kernels-feature', False)
        for _ in range(30):
            S.step()
        torch.cuda.synchronize()
        print('30 eager recovery steps at batch %d done' % BATCH, flush=True)
        return
    if mode != 'all':
        raise SystemExit(__doc__)
    for feature in (False, True):
        for graph in (False, True):
            t = windows(recovery(G, D, feature, graph).step)
            report('recovery step, %s, %s, batch %d' % ('sndcgan feature term' if feature else 'pixel-only',
                                                        'hipGraph replay' if graph else 'host-driven', BATCH), t,
                   '   default run (%d steps): %.1f s per batch' % (DEFAULT_STEPS, DEFAULT_STEPS * t[0] / 1e3))
    for graph in (False, True):
        report('cDDLS step (for scale), %s, batch %d' % ('hipGraph replay' if graph else 'host-driven', BATCH),
               windows(sampler(G, D, graph=graph).step))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'all')
