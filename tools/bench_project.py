"""Dev tool: the StyleGAN2 projector (contrad_amd/project.py, csrc/project/project.hip) measured.

    python tools/bench_project.py kernels [OUT.txt]   # the four kernels against a torch composition of the same arithmetic
    python tools/bench_project.py whole   [OUT.txt]   # projector steps per second for StyleGAN2 at 32 x 32 (random weights)

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time; the
torch compositions (fp32 tensor ops, several launches and temporaries) run in the same process, alternating with ours.  For the
record only: nothing is gated on a time.
"""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import ops, project  # noqa: E402

dev = torch.device('cuda', 0)


def torch_image_end(x, t, lam):
    x = x.detach().requires_grad_()
    rows = []
    for l in range(len(lam)):
        a, b = (F.avg_pool2d(v, 1 << l) if l else v for v in (x, t))
        rows.append(((a - b) ** 2).flatten(1).mean(1))
    rows = torch.stack(rows)
    (torch.tensor(lam, device=x.device).view(-1, 1) * rows).sum().backward()
    return rows, x.grad


def torch_noise_reg(m, acc, scale):
    m = m.detach().requires_grad_()
    cur, reg = m, 0.0
    while True:
        reg = reg + (cur * torch.roll(cur, 1, 3)).flatten(1).mean(1) ** 2 + (cur * torch.roll(cur, 1, 2)).flatten(1).mean(1) ** 2
        if cur.shape[2] <= 8:
            break
        cur = F.avg_pool2d(cur, 2)
    reg.sum().backward()
    return reg, acc.add_(m.grad, alpha=scale)


def torch_normalize(m):
    m -= m.mean(dim=(1, 2, 3), keepdim=True)
    m *= m.square().mean(dim=(1, 2, 3), keepdim=True).rsqrt()
    return m


def kernels(emit):
    g = torch.Generator(device=dev).manual_seed(0)
    for N, S, lam in ((8, 32, (1.0,)), (8, 32, (1.0, 1.0, 1.0, 1.0)), (8, 512, (1.0,)), (8, 512, (1.0, 1.0, 1.0, 1.0))):
        x, t = torch.rand(N, 3, S, S, generator=g, device=dev), torch.rand(N, 3, S, S, generator=g, device=dev)
        pix, gx = torch.empty(len(lam), N, device=dev), torch.empty_like(x)
        part = torch.empty(ops.proj_image_end_partial_floats(len(lam), N, S, S), device=dev)
        for rnd in range(2):
            tm = windows(lambda: ops.proj_image_end(x, t, lam, pix=pix, gx=gx, partial=part))
            emit(fmt('image_end %d x 3 x %d^2, %d levels, round %d' % (N, S, len(lam), rnd), tm,
                     '  %6.0f GB/s of two reads and one write' % (3.0 * x.numel() * 4 / tm[0] * 1e-6)))
            tm = windows(lambda: torch_image_end(x, t, lam))
            emit(fmt('  torch composition (avg_pool2d, autograd), round %d' % rnd, tm))
    for shape in ((8, 4, 4, 512), (8, 32, 32, 128), (8, 512, 512, 64), (8, 512, 512, 8)):
        gp, nw = torch.randn(*shape, generator=g, device=dev), torch.full((1,), 0.1, device=dev)
        out = torch.empty(shape[0], 1, shape[1], shape[2], device=dev)
        for rnd in range(2):
            tm = windows(lambda: ops.proj_noise_grad(gp, nw, out=out))
            emit(fmt('noise_grad %s, round %d' % (shape, rnd), tm, '  %6.0f GB/s of one read' % (gp.numel() * 4 / tm[0] * 1e-6)))
            tm = windows(lambda: nw * gp.sum(-1))
            emit(fmt('  torch composition, round %d' % rnd, tm))
    for N, R in ((8, 8), (8, 32), (8, 128), (8, 512)):
        m, acc = torch.randn(N, 1, R, R, generator=g, device=dev), torch.zeros(N, 1, R, R, device=dev)
        reg, scratch = torch.empty(N, device=dev), torch.empty(ops.proj_noise_reg_scratch_floats(N, R), device=dev)
        for rnd in range(2):
            tm = windows(lambda: ops.proj_noise_reg(m, acc, 1e5, reg=reg, scratch=scratch))
            emit(fmt('noise_reg %d maps of %d^2, round %d' % (N, R, rnd), tm))
            tm = windows(lambda: torch_noise_reg(m, acc, 1e5))
            emit(fmt('  torch composition (roll, avg_pool2d, autograd), round %d' % rnd, tm))
            tm = windows(lambda: ops.proj_noise_normalize_(m))
            emit(fmt('noise_normalize %d maps of %d^2, round %d' % (N, R, rnd), tm))
            tm = windows(lambda: torch_normalize(m))
            emit(fmt('  torch composition, round %d' % rnd, tm))


def whole(emit):
    from contrad_amd.evaluate.gan import freeze
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(0)
    G = freeze(get_architecture('stylegan2', (32, 32, 3))[0].to(dev))
    w_avg, w_std = project.w_statistics(G, 1024)
    x = torch.rand(8, 3, 32, 32, device=dev)
    for space, noise in (('w', 'opt'), ('wplus', 'opt'), ('w', 'fixed')):
        proj = project.Projector(G, 8, space, noise, w_avg=w_avg, w_std=w_std)
        proj.set_targets(x)
        proj.start(noise=G.make_noise() if noise == 'fixed' else None)
        for s in range(5):
            proj.step(s, 100)
        torch.cuda.synchronize()
        t0 = time.time()
        for s in range(5, 55):
            proj.step(s, 100)
        torch.cuda.synchronize()
        emit('projector step, StyleGAN2 32 x 32, batch 8, space %s, noise %s: %.2f ms wall per step (eager)'
             % (space, noise, (time.time() - t0) / 50 * 1e3))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'kernels': kernels, 'whole': whole}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
