"""Dev tool: where the time of a sliced-Wasserstein evaluation (contrad_amd/swd.py, csrc/eval/swd.hip) goes.

    python tools/bench_swd.py kernels [OUT.txt]   # every kernel at the CIFAR shape: n = 16384 images of 32 x 32, 2^21 descriptors per level
    python tools/bench_swd.py whole   [OUT.txt]   # swd_of wall time: the CIFAR shape, and n = 2048 images of 512 x 512
    python tools/bench_swd.py sort    [OUT.txt]   # the row sort alone over row lengths, against its pass model and torch.sort

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time.
The sort's yardstick is its own pass-count model: every launch of the tile kernel and of the pass kernel reads and writes
the whole [rows][n] buffer once, so the model is passes x 2 x buffer bytes, held against 6.3 TB/s (the achievable HBM rate).
The network is data-oblivious (every compare-exchange writes both values back), so timing it on rows that are already
sorted measures the same work as on random rows; ``torch.sort(dim=1)`` on the same buffer is the outside reference point.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import features, ops, swd  # noqa: E402

dev = torch.device('cuda', 0)
HBM = 6.3e12


def sort_passes(n):
    """(tile launches, pass launches) of contrad_swd_sort_rows at row length n (csrc/eval/swd.hip: the host loop)."""
    tl = ops.swd_sort_tile().bit_length() - 1
    plog = max(int(n - 1).bit_length(), 0)
    tiles, passes = 1, 0
    for k in range(tl + 1, plog + 1):
        passes += (k - tl + 1) // 2
        tiles += 1
    return tiles, passes


def sort_lines(emit, rows, n):
    x = torch.randn(rows, n, device=dev)
    ref = torch.sort(x, dim=1).values
    got = ops.swd_sort_rows(x.clone(), n)
    assert torch.equal(got, ref)
    tiles, passes = sort_passes(n)
    nbytes = (tiles + passes) * 2.0 * rows * n * 4
    t = windows(lambda: ops.swd_sort_rows(got, n), iters=3, reps=7, warm=1)
    emit(fmt('swd_sort_rows [%d][%d]: %d tile + %d pass launches' % (rows, n, tiles, passes), t,
             '  %6.0f GB/s of its pass model (%.1f GB), %.2f of the model at HBM rate' % (nbytes / t[0] * 1e-6, nbytes * 1e-9,
                                                                                      nbytes / HBM * 1e3 / t[0])))
    t2 = windows(lambda: torch.sort(x, dim=1), iters=3, reps=7, warm=1)
    emit(fmt('torch.sort(dim=1) on the same [%d][%d] buffer (values and indices, out of place)' % (rows, n), t2,
             '  swd_sort_rows takes %.2f x its time' % (t[0] / t2[0])))
    del x, ref, got


def sort(emit):
    for n in (1 << 14, 1 << 17, 1 << 18, 1 << 21):
        sort_lines(emit, 128, n)


def kernels(emit):
    n, size, nhoods, m = 16384, 32, 128, 128
    g = torch.Generator(device='cpu').manual_seed(0)
    x = torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8).to(dev)
    fine = ops.swd_u8_planes(x)
    t = windows(lambda: ops.swd_u8_planes(x, out=fine))
    emit(fmt('swd_u8_planes %d x %d x %d' % (n, size, size), t, '  %6.0f GB/s' % (x.numel() * 5 / t[0] * 1e-6)))
    coarse = ops.swd_pyr_down(fine)
    t = windows(lambda: ops.swd_pyr_down(fine, out=coarse))
    emit(fmt('swd_pyr_down %d -> %d' % (size, size // 2), t, '  %6.0f GB/s' % ((fine.numel() + coarse.numel()) * 4 / t[0] * 1e-6)))
    t = windows(lambda: ops.swd_pyr_up_sub(fine, coarse))
    emit(fmt('swd_pyr_up_sub %d' % size, t, '  %6.0f GB/s' % ((2 * fine.numel() + coarse.numel()) * 4 / t[0] * 1e-6)))
    D = swd.draws(0, n, [size], nhoods, 1, m)[0]
    cx, cy = swd._centres(D['real'], dev)
    bank, stats = ops.swd_gather(fine, cx, cy, nhoods)
    n_desc, n_pad = n * nhoods, bank.shape[1]
    t = windows(lambda: ops.swd_gather(fine, cx, cy, nhoods, bank=bank, stats=stats), iters=5)
    emit(fmt('swd_gather %d descriptors -> bank [148][%d]' % (n_desc, n_pad), t, '  %6.0f GB/s of the bank written' % (bank.numel() * 4 / t[0] * 1e-6)))
    mu, sigma = swd.channel_stats(stats.cpu().numpy(), n_desc * 49)
    rows, _ = swd.projection_operands(D['dirs'][0], mu, sigma)
    rows = torch.from_numpy(rows).to(dev)
    proj = torch.empty(m, n_pad, device=dev)
    t = windows(lambda: features.similarities(rows, bank, proj), iters=3)
    emit(fmt('projection GEMM [%d][148] x [148][%d] (ops.conv2d_fwd)' % (m, n_pad), t,
             '  %5.1f TFLOP/s, %6.0f GB/s of bank read + projections written' % (2.0 * m * 148 * n_pad / t[0] * 1e-9,
                                                                                (bank.numel() + proj.numel()) * 4 / t[0] * 1e-6)))
    del bank, fine, coarse, x
    sort_lines(emit, m, n_desc)
    other = torch.randn(m, n_pad, device=dev)
    ops.swd_sort_rows(proj, n_desc)
    out = ops.swd_absdiff_sums(proj, other, n_desc)
    t = windows(lambda: ops.swd_absdiff_sums(proj, other, n_desc, out=out), iters=5)
    emit(fmt('swd_absdiff_sums [%d][%d]: two launches' % (m, n_desc), t, '  %6.0f GB/s of two reads' % (2.0 * m * n_desc * 4 / t[0] * 1e-6)))


def whole(emit):
    for n, size in ((16384, 32), (2048, 512)):
        g = torch.Generator(device=dev).manual_seed(0)
        sets = []
        for _ in range(2):                                             # 4 x 4 blocks of 0 ... 239 plus noise of 0 ... 15
            x = torch.randint(0, 240, (n, size // 4, size // 4, 3), generator=g, dtype=torch.uint8, device=dev)
            x = x.repeat_interleave(4, 1).repeat_interleave(4, 2)
            sets.append(x.add_(torch.randint(0, 16, x.shape, generator=g, dtype=torch.uint8, device=dev)).contiguous())
            del x
        t0 = time.time()
        D = swd.draws(0, n, swd.levels_of(size))
        t_draws = time.time() - t0
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.time()
            out = swd.swd_of(sets[0], sets[1], seed=0, draws=D)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        emit('swd_of n = %d, %d x %d, %d levels, %d descriptors per level: %.3f s (min %.3f, max %.3f) wall, first call included; '
             'draws on the host %.3f s; peak device memory %.2f GB; avg %.3f'
             % (n, size, size, len(out['levels']), n * 128, float(np.median(times)), min(times), max(times), t_draws,
                torch.cuda.max_memory_allocated() * 1e-9, out['avg']))
        del sets


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'kernels': kernels, 'whole': whole, 'sort': sort}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
