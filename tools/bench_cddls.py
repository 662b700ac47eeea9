"""Dev tool: one cDDLS Langevin step (contrad_amd/cddls.py) at the reference's default batch (500, 32 x 32), one
configuration per process.

    python tools/bench_cddls.py dhalf            # the sampler's D half: eval forward + input gradient, feature seed included
    python tools/bench_cddls.py dhalf-graph      # the same launches replayed from a hipGraph (device time)
    python tools/bench_cddls.py dhalf-autograd   # the only way without the sampler: D.eval(); D(x).sum().backward() on x.requires_grad_()
    python tools/bench_cddls.py step             # whole step, host-driven
    python tools/bench_cddls.py step-graph       # whole step, hipGraph replay
    python tools/bench_cddls.py kernels          # 30 eager steps, for `rocprofv3 --kernel-trace --stats -- python tools/bench_cddls.py kernels`
    python tools/bench_cddls.py dhalf snresnet18 # any mode on G_SNDCGAN + D_SNResNet18 (second argument, default sndcgan)

Times are HIP-event medians over repeated windows with the min - max spread.  For sndcgan the autograd baseline
differentiates the logit alone (no classifier term): it is a lower bound of what composing the existing modules would cost
per step.  For snresnet18 it is the whole composition: D(x) with the penultimate features, the class logit, backward.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrad_amd import ops
from contrad_amd.cddls import CDDLSSampler
from contrad_amd.models.gan import get_architecture

dev = torch.device('cuda')
BATCH = int(os.environ.get('CDDLS_BENCH_BATCH', '500'))


def windows(fn, iters=20, reps=9, warm=10):
    """Median and (min, max) time per call in milliseconds over ``reps`` event-bracketed windows of ``iters`` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def networks(arch='sndcgan'):
    torch.manual_seed(0)
    G, D = get_architecture(arch, (32, 32, 3))
    G.to(dev); D.to(dev)
    with torch.no_grad():           # fresh u, v are random: a few train-mode passes make them what a checkpoint holds
        D.train()
        for _ in range(5):
            D(torch.rand(8, 3, 32, 32, device=dev))
    G.eval(); D.eval()
    for p in list(G.parameters()) + list(D.parameters()):
        p.requires_grad_(False)
    return G, D


def sampler(G, D, graph=False):
    g = torch.Generator().manual_seed(1)
    W, b = (0.01 * torch.randn(10, D.d_penul, generator=g)).to(dev), torch.zeros(10, device=dev)
    S = CDDLSSampler(G, D, W, b, BATCH, seed=1, graph=graph)
    S.set_class(3)
    S.start(G.sample_latent(BATCH))
    return S


def report(name, t, extra=''):
    print('%-64s %8.3f ms  (min %.3f, max %.3f)%s' % ((name,) + tuple(t) + (extra,)), flush=True)


def run_length(t_ms):
    return '   default run (10 classes x 2 batches x 1000 steps): %.1f min' % (20000 * t_ms / 60e3)


def main(mode, arch='sndcgan'):
    G, D = networks(arch)
    if mode == 'dhalf-autograd':
        x = torch.rand(BATCH, 3, 32, 32, device=dev).requires_grad_()
        w_y = 0.01 * torch.randn(D.d_penul, device=dev)

        def fn():
            x.grad = None
            if arch == 'sndcgan':
                D(x).sum().backward()
            else:
                d, aux = D(x, penultimate=True)
                (-(d.view(-1) + aux['penultimate'] @ w_y)).sum().backward()
        report('D half, autograd %s, batch %d' % ('node (weight prep + filter prep + 3 heads)' if arch == 'sndcgan'
                                                  else 'composition with the class logit, ' + arch, BATCH), windows(fn))
        return
    S = sampler(G, D, graph=(mode == 'step-graph'))
    if mode in ('dhalf', 'dhalf-graph'):
        S.step()
        torch.cuda.synchronize()

        def fn():
            with torch.no_grad():
                S._d_forward()
                S._d_backward()
        if mode == 'dhalf':
            report('D half, sampler (forward + input gradient + feature seed), %s, batch %d' % (arch, BATCH), windows(fn))
        else:
            g, scratch = torch.cuda.CUDAGraph(), {}
            with ops.private_workspace(scratch), torch.cuda.graph(g):
                fn()
            torch.cuda.synchronize()
            report('D half, sampler, hipGraph replay, %s, batch %d' % (arch, BATCH), windows(g.replay))
    elif mode in ('step', 'step-graph'):
        t = windows(S.step)
        report('whole step, %s, %s, batch %d' % ('hipGraph replay' if mode == 'step-graph' else 'host-driven', arch, BATCH), t,
               run_length(t[0]))
    elif mode == 'kernels':
        for _ in range(30):
            S.step()
        torch.cuda.synchronize()
        print('30 eager steps at batch %d done' % BATCH, flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'step', sys.argv[2] if len(sys.argv) > 2 else 'sndcgan')
