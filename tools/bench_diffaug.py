"""Dev tool: the fused DiffAugment kernels (csrc/baseline_aug.hip, policy color,cutout) against the same arithmetic
composed from torch ops on the same device, forward and forward + backward, at the batch of an ``aug_both`` D-step with
options.batch_size = 64 (2N = 128 images of 32 x 32).

    python tools/bench_diffaug.py [batch [size]]

Times are HIP-event medians over repeated windows with the min - max spread; both versions are timed in the same process,
alternating.  The composed version restates third_party/diffaug.py's stages (brightness, saturation, contrast, cutout by an
index mask) as torch tensor ops, with the same host-drawn parameters already on the device.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrad_amd import ops
from contrad_amd.augment import DiffAugLayer, _DiffAugFn

dev = torch.device('cuda')


def windows(fn, iters=50, reps=9, warm=20):
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


def composed(x, Pd):
    """color,cutout out of torch ops; Pd (B, 8) on the device."""
    B, _, H, W = x.shape
    b, s, c = (Pd[:, k].view(B, 1, 1, 1) for k in range(3))
    u = 2.0 * x - 1.0
    u = u + b
    m = u.mean(dim=1, keepdim=True)
    u = (u - m) * s + m
    m = u.mean(dim=[1, 2, 3], keepdim=True)
    u = (u - m) * c + m
    ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
    rows = torch.clamp(torch.arange(ch, device=dev).view(1, ch, 1) + Pd[:, 5].long().view(B, 1, 1) - ch // 2, 0, H - 1)
    cols = torch.clamp(torch.arange(cw, device=dev).view(1, 1, cw) + Pd[:, 6].long().view(B, 1, 1) - cw // 2, 0, W - 1)
    mask = torch.ones(B, H, W, device=dev)
    mask[torch.arange(B, device=dev).view(B, 1, 1), rows, cols] = 0
    u = u * mask.unsqueeze(1)
    return 0.5 * u + 0.5


def main(B, S):
    torch.manual_seed(0)
    layer = DiffAugLayer(policy='color,cutout')
    Pd = layer.sample(B, S, S).to(dev)
    x = torch.rand(B, 3, S, S, device=dev)
    g = torch.randn(B, 3, S, S, device=dev)
    xg = x.clone().requires_grad_()
    err = (ops.diffaug(x, Pd, layer.bits) - composed(x, Pd)).abs().max().item()
    print('fused vs composed, max abs difference of the outputs: %.2e' % err)
    assert err < 1e-5

    def fused_fwd():
        ops.diffaug(x, Pd, layer.bits)

    def composed_fwd():
        with torch.no_grad():
            composed(x, Pd)

    def fused_both():
        xg.grad = None
        _DiffAugFn.apply(xg, Pd, layer.bits).backward(g)

    def composed_both():
        xg.grad = None
        composed(xg, Pd).backward(g)

    def fused_bwd_kernel():
        ops.diffaug(g, Pd, layer.bits, backward=True)

    print('%-18s %-9s B=%d %dx%d  %9.1f us  (min %.1f, max %.1f)' % (('backward kernel', 'fused', B, S, S) + windows(fused_bwd_kernel)))
    nbytes = x.numel() * 4
    for name, a, b in (('forward', fused_fwd, composed_fwd), ('forward + backward', fused_both, composed_both)):
        for _ in range(2):                      # both versions twice, alternating: the spread between repeats is the noise
            for tag, fn in (('fused', a), ('composed', b)):
                t = windows(fn)
                print('%-18s %-9s B=%d %dx%d  %9.1f us  (min %.1f, max %.1f)' % ((name, tag, B, S, S) + t), flush=True)
    print('one read + one write of the batch: %.2f MB per direction' % (2 * nbytes / 1e6))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128, int(sys.argv[2]) if len(sys.argv) > 2 else 32)
