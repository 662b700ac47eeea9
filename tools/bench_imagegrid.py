"""Dev tool: the image-side kernel (csrc/imagegrid.hip) against the ATen chain it replaces, and where the time of a sampling
run goes.

    python tools/bench_imagegrid.py kernels [OUT.txt]   # images_u8 vs to_uint8().permute().contiguous(); image_grid_u8
    python tools/bench_imagegrid.py sample  [OUT.txt]   # test_gan_sample.py --n_samples 10000 (sndcgan, fresh weights), by stage

Times are HIP-event medians over repeated windows with the min - max spread (one process, one configuration at a time):
``eager`` windows include the host's launch rate, ``graph`` windows replay 20 captured calls per graph launch and so show the
device time of the launches alone.  Bytes moved are the compulsory ones: 4 read and 1 written per value (padding: 1 written).
"""
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrad_amd import ops
from contrad_amd.hostio import to_uint8

dev = torch.device('cuda')


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
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    return g, inner


def line(name, t, nbytes):
    return '%-64s %9.1f us  (min %.1f, max %.1f)  %7.1f GB/s' % (name, t[0], t[1], t[2], nbytes / t[0] * 1e-3)


def both(name, fn, nbytes, emit):
    emit(line(name + ', eager', windows(fn), nbytes))
    g, inner = graphed(fn)
    t = windows(g.replay, iters=20)
    emit(line(name + ', graph', tuple(v / inner for v in t), nbytes))


def kernels(emit):
    for shape in ((500, 3, 32, 32), (16, 3, 512, 512)):
        x = torch.rand(shape, device=dev)
        nbytes = 5 * x.numel()
        tag = 'x'.join(map(str, shape))
        assert torch.equal(ops.images_u8(x), to_uint8(x).permute(0, 2, 3, 1).contiguous())
        both('images_u8 %s' % tag, lambda: ops.images_u8(x), nbytes, emit)
        both('to_uint8().permute().contiguous() %s' % tag, lambda: to_uint8(x).permute(0, 2, 3, 1).contiguous(), nbytes, emit)
    x = torch.rand(64, 3, 32, 32, device=dev)
    rows, cols, _ = ops.grid_canvas_shape(64, 32, 32, 8, 2)
    both('image_grid_u8 64x3x32x32 -> %dx%dx3' % (rows, cols), lambda: ops.image_grid_u8(x), 4 * x.numel() + 3 * rows * cols, emit)
    # the D2H copy that follows: uint8 batch vs float batch (pageable destination, synchronous, as the sample writer does)
    x = torch.rand(500, 3, 32, 32, device=dev)
    u = ops.images_u8(x)
    for name, t in (('D2H uint8 500x32x32x3', u), ('D2H float 500x3x32x32', x)):
        ts = []
        for _ in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.cpu()
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = ts[5:]
        emit('%-64s %9.1f us  (min %.1f, max %.1f)  host clock' % (name, statistics.median(ts), min(ts), max(ts)))


def sample(emit):
    """A sampling run of 10 000 images through contrad_amd.sample.main, then the same loop with the stages timed apart."""
    import numpy as np
    from contrad_amd import config, sample as S
    from contrad_amd.hostio import png_bytes
    from contrad_amd.models.gan import get_architecture
    import shutil
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(0)
        G, _ = get_architecture('sndcgan', (32, 32, 3))
        torch.save(G.state_dict(), os.path.join(tmp, 'gen.pt'))
        shutil.copy(os.path.join(config.CONFIG_ROOT, 'gan', 'cifar10', 'c10_b64.gin'), tmp)
        S.main([os.path.join(tmp, 'gen.pt'), 'sndcgan', '--n_samples', '1000', '--seed', '1'])       # warm: kernels loaded
        t0 = time.perf_counter()
        S.main([os.path.join(tmp, 'gen.pt'), 'sndcgan', '--n_samples', '10000', '--seed', '2'])
        emit('test_gan_sample.py sndcgan --n_samples 10000 --batch_size 500, end to end: %.2f s' % (time.perf_counter() - t0))
        G = S.load_generator(os.path.join(tmp, 'gen.pt'), 'sndcgan', dev)
        tg = tc = tp = tw = 0.0
        with torch.no_grad():
            for i in range(20):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                x = G(G.sample_latent(500)).contiguous()
                torch.cuda.synchronize(); t1 = time.perf_counter()
                u8 = ops.images_u8(x).cpu().numpy()
                t2 = time.perf_counter()
                blobs = [png_bytes(u8[j]) for j in range(500)]
                t3 = time.perf_counter()
                for j, b in enumerate(blobs):
                    with open(os.path.join(tmp, 's%d.png' % (i * 500 + j)), 'wb') as f:
                        f.write(b)
                t4 = time.perf_counter()
                tg, tc, tp, tw = tg + t1 - t0, tc + t2 - t1, tp + t3 - t2, tw + t4 - t3
        emit('  stages, serial, 20 batches of 500: generator %.3f s, images_u8 + D2H %.3f s, PNG encode (one thread) %.3f s, '
             'file writes %.3f s' % (tg, tc, tp, tw))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'kernels': kernels, 'sample': sample}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
