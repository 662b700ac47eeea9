"""Dev tool: the linear-evaluation head (csrc/linhead.hip) against the same iteration written in torch ops on the same
GPU, and one epoch of the lin-eval loop eager vs --graph.

    python tools/bench_lineval.py head       # fused vs torch-op iteration at (256, 8192, 10) and (256, 8192, 100)
    python tools/bench_lineval.py kernels    # the launches alone, for a `rocprofv3 --kernel-trace --stats -- ...` run
    python tools/bench_lineval.py epoch      # epoch wall time on the synthetic 50 000-image set, eager and --graph
    python tools/bench_lineval.py epoch-inline   # one eager epoch in-process, for a kernel trace (trunk / head split)

The torch-op baseline is what a user would otherwise run on this checkout: F.linear, F.cross_entropy, topk accuracy,
backward, torch.optim.SGD and the three .item() reads of the reference's loop.  Times are HIP-event medians over
repeated windows with the min - max spread; one process, one configuration at a time.
"""
import csv
import os
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrad_amd import ops

dev = torch.device('cuda')
SHAPES = [(256, 8192, 10), (256, 8192, 100)]


def windows(fn, iters=100, reps=9, warm=30):
    """Median and (min, max) time per call in microseconds over ``reps`` event-bracketed windows of ``iters`` calls."""
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
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(out), min(out), max(out)


def graphed(fn, inner=20):
    """``fn`` captured ``inner`` times into one hipGraph: the device time of the launches without the host's launch rate."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    scratch = {}
    with ops.private_workspace(scratch), torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    return g, inner, scratch


def setup(N, K, C):
    gen = torch.Generator().manual_seed(0)
    Fd = (torch.randn(N, K, generator=gen).relu() * 2 / K ** 0.5).to(dev)
    W = ((torch.rand(C, K, generator=gen) * 2 - 1) / K ** 0.5).to(dev)
    b = torch.zeros(C, device=dev)
    y = torch.randint(0, C, (N,), generator=gen).to(dev)
    return Fd, W, b, y


def torch_accuracy(output, target, topk):
    _, pred = output.topk(max(topk), 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / target.size(0)) for k in topk]


def fmt(name, t):
    return '%-58s %8.1f us  (min %.1f, max %.1f)' % ((name,) + tuple(t))


def head():
    for (N, K, C) in SHAPES:
        Fd, W, b, y = setup(N, K, C)
        dl, meters, lr = torch.empty(N, C, device=dev), torch.zeros(4, dtype=torch.float64, device=dev), torch.full((1,), 1e-3, device=dev)

        def fused_train():
            ops.linhead_fwd(Fd, W, b, y=y, dlogits=dl, meters=meters, want_logits=False)
            ops.linhead_wgrad_sgd(Fd, dl, W, b, lr=lr)

        def fused_eval():
            ops.linhead_fwd(Fd, W, b, y=y, meters=meters, want_logits=False)

        def fused_wgrad():
            ops.linhead_wgrad_sgd(Fd, dl, W, b, lr=lr)

        lin = torch.nn.Linear(K, C).to(dev)
        opt = torch.optim.SGD(lin.parameters(), lr=1e-3)

        def torch_train():
            out = F.linear(Fd, lin.weight, lin.bias)
            loss = F.cross_entropy(out, y)
            a1, a5 = torch_accuracy(out, y, (1, 5))
            loss.item(); a1.item(); a5.item()
            opt.zero_grad()
            loss.backward()
            opt.step()

        def torch_eval():
            with torch.no_grad():
                out = F.linear(Fd, lin.weight, lin.bias)
                loss = F.cross_entropy(out, y)
                a1, = torch_accuracy(out, y, (1,))
            loss.item(); a1.item()

        print('--- N x K x C = %d x %d x %d' % (N, K, C), flush=True)
        print(fmt('train iteration, fused (launches 1 - 3), host-driven', windows(fused_train)), flush=True)
        print(fmt('train iteration, torch ops + 3 .item()', windows(torch_train)), flush=True)
        print(fmt('eval iteration, fused (launches 1 - 2), host-driven', windows(fused_eval)), flush=True)
        print(fmt('eval iteration, torch ops + 2 .item()', windows(torch_eval)), flush=True)
        for name, fn, nbytes in (('train iteration, fused, graph replay (device time)', fused_train, None),
                                 ('launches 1 + 2, graph replay (device time)', fused_eval, None),
                                 ('launch 3, graph replay (device time)', fused_wgrad, 4.0 * (N * K + N * C + 2 * C * K))):
            g, inner, _keep = graphed(fn)
            med, lo, hi = windows(g.replay, iters=20, reps=9, warm=5)
            t = (med / inner, lo / inner, hi / inner)
            extra = '' if nbytes is None else '   %.2f TB/s over F + dlogits + W read and written' % (nbytes / t[0] / 1e6)
            print(fmt(name, t) + extra, flush=True)


def kernels():
    for (N, K, C) in SHAPES:
        Fd, W, b, y = setup(N, K, C)
        dl, meters, lr = torch.empty(N, C, device=dev), torch.zeros(4, dtype=torch.float64, device=dev), torch.full((1,), 1e-3, device=dev)
        for _ in range(200):
            ops.linhead_fwd(Fd, W, b, y=y, dlogits=dl, meters=meters, want_logits=False)
            ops.linhead_wgrad_sgd(Fd, dl, W, b, lr=lr)
        torch.cuda.synchronize()
        S = ops.linhead_plan(N, K, C)[0]
        print('N x K x C = %d x %d x %d: launch 1 moves %.2f MB (F, W, partial sums written), launch 3 %.2f MB (F, dlogits, W read '
              'and written)' % (N, K, C, 4e-6 * (N * K + C * K + S * N * C), 4e-6 * (N * K + N * C + 2 * C * K)), flush=True)


def epoch(epochs=3):
    from contrad_amd.models.gan import get_architecture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    for extra in ([], ['--graph']):
        with tempfile.TemporaryDirectory() as d:
            torch.save(D.state_dict(), os.path.join(d, 'dis.pt'))
            cmd = ['timeout', '-k', '10', '400', sys.executable, os.path.join(root, 'test_lineval.py'), os.path.join(d, 'dis.pt'),
                   'sndcgan', '--synthetic', '--seed', '1', '--epochs', str(epochs)] + extra
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)      # a fresh child per run, one at a time
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit(r.returncode)
            rows = list(csv.reader(open(os.path.join(d, 'lin_eval_1.csv'))))[1:]
            print('%-8s epoch wall time (196 train + 40 test batches of 256, s): %s   last row: %s' % (
                'graph' if extra else 'eager', ' '.join('%.3f' % float(r_[1]) for r_ in rows), ','.join(rows[-1])), flush=True)


def epoch_inline():
    """One eager epoch in this process (for a kernel trace: trunk and head kernels of the loop, by name)."""
    from contrad_amd import lineval
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(0)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    with tempfile.TemporaryDirectory() as d:
        torch.save(D.state_dict(), os.path.join(d, 'dis.pt'))
        lineval.main([os.path.join(d, 'dis.pt'), 'sndcgan', '--synthetic', '--seed', '1', '--epochs', '1'])


if __name__ == '__main__':
    {'head': head, 'kernels': kernels, 'epoch': epoch, 'epoch-inline': epoch_inline}[sys.argv[1] if len(sys.argv) > 1 else 'head']()
