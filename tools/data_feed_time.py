#!/usr/bin/env python
"""What feeding the real batch costs per step: the ``train_gan`` loop body (``train_step``, ContraD, SNDCGAN,
configs/gan/cifar10/c10_b512.gin, one GPU) fed three ways, alternated in ONE process on the same code:

    synthetic : train_gan._synthetic_loader   (torch.rand on the host, .to(device, non_blocking=True) per step)
    device    : data.DeviceLoader              (50 000 random uint8 images resident, one gather launch per step)
    static    : one device batch reused every step -- the floor, and what bench.py measures

Each window is 20 steps timed with HIP events after 10 discarded steps; 9 windows per item, the items alternating
window by window.  ``--part gather`` times csrc/data.hip alone at (512, 32, 32) and (16, 512, 512) and reports the
achieved bytes per second against the bytes the gather has to move (B*H*W*3 in, B*H*W*12 out).

    timeout -k 10 300 python tools/data_feed_time.py --part eager  --out profiles/data_feed.txt && \\
    timeout -k 10 300 python tools/data_feed_time.py --part graph  --out profiles/data_feed.txt && \\
    timeout -k 10 120 python tools/data_feed_time.py --part gather --out profiles/data_feed.txt

Each part appends its table to ``--out``.  No GPU: an error, not a fallback.
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, STEPS, DISCARD = 9, 20, 10


def _stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def _loop(graph, batch, n_images, out):
    from contrad_amd import config, train_gan
    from contrad_amd.augment import get_augment
    from contrad_amd.data import DeviceLoader
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.optim import FusedAdam
    from contrad_amd.training.gan import setup
    dev = torch.device('cuda', 0)
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b512.gin')
    P = train_gan.parse_args([gin, 'sndcgan', '--mode=contrad', '--aug=simclr'] + (['--graph'] if graph else []))
    P = setup(P)
    P.rank, P.distributed = 0, False
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'), gin])
    options = train_gan.get_options_dict()
    if batch is not None:
        options['batch_size'] = batch
    B = options['batch_size']
    image_size = train_gan.IMAGE_SIZES[options['dataset']]
    torch.manual_seed(0); np.random.seed(0)
    G, D = get_architecture('sndcgan', image_size, P=P)
    G, D = G.to(dev), D.to(dev)
    opt_G = FusedAdam(G.parameters(), lr=options['lr'], betas=tuple(options['beta']))
    opt_D = FusedAdam(D.parameters(), lr=options['lr_d'], betas=tuple(options['beta']))
    P.augment_fn = get_augment(mode=P.aug).to(dev)
    graphed = train_gan.GraphedCritic() if graph else None

    h, w, c = image_size
    x = np.random.RandomState(0).randint(0, 256, (n_images, h, w, c)).astype(np.uint8)
    static = torch.rand(B, c, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    loaders = [('synthetic', train_gan._synthetic_loader(B, image_size, dev, 0)),
               ('device', DeviceLoader(x, B, 0, 1, flip=False, drop_last=True, device=dev)),
               ('static', itertools.repeat((static, None)))]
    times = {name: [] for name, _ in loaders}
    step = 0
    for _ in range(WINDOWS):
        for name, loader in loaders:
            for _ in range(DISCARD):
                step += 1
                train_gan.train_step(P, options, G, D, opt_G, opt_D, loader, step, (None, None), graphed)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(STEPS):
                step += 1
                losses = train_gan.train_step(P, options, G, D, opt_G, opt_D, loader, step, (None, None), graphed)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / STEPS)
    assert all(np.isfinite(float(v)) for v in losses.values())
    lines = ['train_step, ContraD SNDCGAN batch %d, %s: ms per step, median (min - max) of %d windows of %d steps' % (
        B, 'D- and G-step replayed from hipGraphs (--graph)' if graph else 'eager', WINDOWS, STEPS)]
    for name, _ in loaders:
        med, lo, hi = _stats(times[name])
        lines.append('  %-10s %7.3f  (%7.3f - %7.3f)' % (name, med, lo, hi))
    _emit(lines, out)


def _gather(out):
    from contrad_amd import ops
    dev = torch.device('cuda', 0)
    lines = ['gather alone (csrc/data.hip): us per launch, median (min - max) of %d windows of 200 launches; bytes = '
             'B*H*W*3 in + B*H*W*12 out' % WINDOWS]
    for n, B, H, W in ((50000, 512, 32, 32), (64, 16, 512, 512)):
        rs = np.random.RandomState(n)
        src = torch.from_numpy(rs.randint(0, 256, (n, H, W, 3)).astype(np.uint8)).to(dev)
        params = torch.tensor(np.stack([rs.randint(0, n, B), rs.randint(0, 2, B)], 1), dtype=torch.float32, device=dev)
        dst = torch.empty(B, 3, H, W, device=dev)
        nbytes = B * H * W * 15
        for _ in range(DISCARD):
            ops.gather_u8_nchw(src, params, H, W, out=dst)
        us = []
        for _ in range(WINDOWS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(200):
                ops.gather_u8_nchw(src, params, H, W, out=dst)
            t1.record()
            t1.synchronize()
            us.append(t0.elapsed_time(t1) / 200 * 1e3)
        med, lo, hi = _stats(us)
        lines.append('  B %4d x %3d x %3d (%.1f MB): %8.2f  (%8.2f - %8.2f)  -> %.3f TB/s at the median (back-to-back '
                     'launches: launch cost included)' % (B, H, W, nbytes / 1e6, med, lo, hi, nbytes / (med * 1e-6) / 1e12))
    _emit(lines, out)


def _emit(lines, out):
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--part', choices=('eager', 'graph', 'gather'), required=True)
    ap.add_argument('--out', default=None, help='file the table is appended to')
    ap.add_argument('--batch', type=int, default=None, help='override the batch of c10_b512.gin')
    ap.add_argument('--images', type=int, default=50000, help='size of the resident random set')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('data_feed_time.py measures on the GPU only')
    torch.cuda.set_device(0)
    if a.part == 'gather':
        _gather(a.out)
    else:
        _loop(a.part == 'graph', a.batch, a.images, a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
