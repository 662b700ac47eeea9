"""Sliced Wasserstein distance (SWD) of generated images from real ones on Laplacian-pyramid patches: Karras et al.,
Progressive Growing of GANs (ICLR 2018), their sliced_wasserstein.py; the sliced distance itself is Rabin et al. 2011.  The one
sample-quality number of this project that reads no network (DESIGN.md sections 8 and 22): uint8 images in, one value per
resolution level out, comparable across encoders, architectures and repositories that share the definition.

The definition.  Two sets of n uint8 images [n, H, W, 3], H == W a power of two >= 16, taken as floats 0 ... 255.
  1. levels: res = H; while res >= 16: levels.append(res); res //= 2.
  2. Laplacian pyramid per image and channel: g = [1 4 6 4 1] / 16, F = outer(g, g); down(x) convolves with F under the
     mirror boundary (d c b | a b c d | c b a) and keeps [::2, ::2]; up(x) zero-inserts to twice the size (x at the even
     coordinates) and convolves with 4 F; pyr[0] = x, pyr[i] = down(pyr[i - 1]), pyr[i - 1] -= up(pyr[i]); the last level
     stays Gaussian.
  3. descriptors per level and set: ``nhoods`` patches of 7 x 7 x 3 per image around integer centres in [3, res - 4], the 147
     values in the order c * 49 + dy * 7 + dx; over all descriptors of the set each channel has its mean taken off and is
     divided by its population standard deviation; real and fake are normalised separately.
  4. distance per level: for each of ``dir_repeats`` repeats, 147 x ``dirs_per_repeat`` standard normal directions with unit
     columns; project both sets, sort every projection ascending, mean |A_sorted - B_sorted| over all entries; the level's
     value is the mean over the repeats times 1e3.  The result: the values per level and their plain average.
  5. every draw comes from ``numpy.random.RandomState(seed)`` on the host, in the order of ``draws``.

On the device (csrc/eval/swd.hip): the pyramid and the patch gather are kernels of their own; the gather writes the transposed
bank [148][n_pad] of features.py and the channels' float64 sums, so the normalisation is folded into the projection -- the GEMM
(``ops.conv2d_fwd``, as ``features.similarities``) takes dirs / sigma_c as its input rows and gives one projection per
contiguous row [directions][n_pad]; the constant -sum mu_c / sigma_c dir of a row, which a sort only shifts, is added in
float64 by the kernel that sums |A - B| (the conv engine's bias is per output column, here per descriptor, so it cannot carry
a per-direction constant).  No normalised copy of the bank is written.  One repeat is projected, sorted and summed at a time.
"""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import features, ops
from .evaluate.gan import WeightsMonitor, load_x_train, own_network
from .hooks import Hook

PATCH = 7
HALF = PATCH // 2
MIN_RES = 16
MAX_N = 16384                               # the command line's default cap (Karras et al. use 16384 images)


def levels_of(size):
    """[size, size / 2, ..., 16] for a power of two >= 16."""
    size = int(size)
    if size < MIN_RES or size & (size - 1):
        raise ValueError('swd: the image side must be a power of two and at least %d, got %d' % (MIN_RES, size))
    out = []
    while size >= MIN_RES:
        out.append(size)
        size //= 2
    return out


def check_settings(n, nhoods, dir_repeats, dirs_per_repeat):
    for name, v in (('n', n), ('nhoods', nhoods), ('dir_repeats', dir_repeats), ('dirs_per_repeat', dirs_per_repeat)):
        if int(v) < 1:
            raise ValueError('swd: %s must be at least 1, got %r' % (name, v))


def draws(seed, n, levels, nhoods=128, dir_repeats=4, dirs_per_repeat=128):
    """Every random number of one evaluation, from ``numpy.random.RandomState(seed)`` in this order: per level, finest first,
    ``rs.randint(3, res - 3, (n * nhoods, 2))`` for the real set (column 0: cx, column 1: cy; descriptor d belongs to image
    d // nhoods), the same for the fake set, then per repeat ``rs.randn(147, dirs_per_repeat)`` with every column scaled to
    unit length.  Returns a list with one dict per level: ``res``, ``real`` and ``fake`` (int32 [n * nhoods, 2]), ``dirs``
    (float64 [dir_repeats, 147, dirs_per_repeat])."""
    check_settings(n, nhoods, dir_repeats, dirs_per_repeat)
    rs = np.random.RandomState(int(seed))
    out = []
    for res in levels:
        real = rs.randint(HALF, res - HALF, (n * nhoods, 2)).astype(np.int32)
        fake = rs.randint(HALF, res - HALF, (n * nhoods, 2)).astype(np.int32)
        dirs = np.empty((dir_repeats, ops.SWD_DESC, dirs_per_repeat), np.float64)
        for r in range(dir_repeats):
            d = rs.randn(ops.SWD_DESC, dirs_per_repeat)
            dirs[r] = d / np.sqrt((d * d).sum(axis=0, keepdims=True))
        out.append({'res': int(res), 'real': real, 'fake': fake, 'dirs': dirs})
    return out


_draws = draws                              # (``swd_of`` has an argument of that name)


def check_sets(real_u8, fake_u8):
    """The refusals of ``swd_of``, in order -> (n, levels)."""
    features.check_u8(real_u8, 'real', 'swd')
    features.check_u8(fake_u8, 'fake', 'swd')
    for what, x in (('real', real_u8), ('fake', fake_u8)):
        if x.shape[1] != x.shape[2]:
            raise ValueError('swd: the %s images are %d x %d, square images expected' % (what, x.shape[1], x.shape[2]))
    levels = levels_of(real_u8.shape[1])
    if tuple(fake_u8.shape[1:]) != tuple(real_u8.shape[1:]):
        raise ValueError('swd: real images of %s against fake images of %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    if real_u8.shape[0] != fake_u8.shape[0]:
        raise ValueError('swd: %d real images against %d fake ones: equal counts expected' % (real_u8.shape[0], fake_u8.shape[0]))
    if fake_u8.device != real_u8.device:
        raise RuntimeError('swd: the real images are on %s, the fake ones on %s' % (real_u8.device, fake_u8.device))
    return int(real_u8.shape[0]), levels


def check_draws(D, n, levels, nhoods, dir_repeats, dirs_per_repeat):
    """Explicit draws must have the shapes of ``draws`` and centres inside [3, res - 4] (the kernel would clamp them)."""
    if len(D) != len(levels):
        raise ValueError('swd: draws for %d levels, the images have %d' % (len(D), len(levels)))
    for lv, res in zip(D, levels):
        if lv['res'] != res:
            raise ValueError('swd: draws of level %r where level %d is due' % (lv['res'], res))
        for what in ('real', 'fake'):
            p = np.asarray(lv[what])
            if p.shape != (n * nhoods, 2) or p.min() < HALF or p.max() > res - HALF - 1:
                raise ValueError('swd: the %s centres of level %d must be [%d, 2] integers in [%d, %d]'
                                 % (what, res, n * nhoods, HALF, res - HALF - 1))
        if np.asarray(lv['dirs']).shape != (dir_repeats, ops.SWD_DESC, dirs_per_repeat):
            raise ValueError('swd: the directions of level %d must be [%d, %d, %d]' % (res, dir_repeats, ops.SWD_DESC, dirs_per_repeat))


def pyramid(x_u8, n_levels):
    """The Laplacian pyramid of a uint8 set as fp32 planes [(n * 3, res, res)], finest first; the last level is Gaussian."""
    pyr = [ops.swd_u8_planes(x_u8.contiguous())]
    for i in range(1, n_levels):
        pyr.append(ops.swd_pyr_down(pyr[i - 1]))
        ops.swd_pyr_up_sub(pyr[i - 1], pyr[i])
    return pyr


def channel_stats(stats, count):
    """(mu [3], sigma [3]) in float64 from the gather's sums and sums of squares over ``count`` values per channel."""
    s = np.asarray(stats, np.float64)
    mu = s[:3] / count
    var = s[3:] / count - mu * mu
    return mu, np.sqrt(np.maximum(var, 0.0))


def projection_operands(dirs, mu, sigma):
    """The GEMM's input rows [dirs_per_repeat, 148] (fp32: dirs / sigma_c, column 147 zero) and the constant of every row in
    float64, -sum_k mu_c(k) / sigma_c(k) dirs[k][r], for one repeat's directions [147, dirs_per_repeat]."""
    inv = np.repeat(1.0 / sigma, PATCH * PATCH)[:, None]                       # [147, 1]
    w = dirs * inv
    rows = np.zeros((dirs.shape[1], ops.SWD_BANK_ROWS), np.float32)
    rows[:, :ops.SWD_DESC] = w.T
    shift = -(np.repeat(mu, PATCH * PATCH)[:, None] * w).sum(axis=0)
    return rows, shift


def _centres(p, dev):
    p = np.ascontiguousarray(np.asarray(p, np.int32))
    return torch.from_numpy(np.ascontiguousarray(p[:, 0])).to(dev), torch.from_numpy(np.ascontiguousarray(p[:, 1])).to(dev)


def swd_of(real_u8, fake_u8, seed=0, nhoods=128, dir_repeats=4, dirs_per_repeat=128, draws=None):
    """The sliced Wasserstein distance of two device-resident uint8 sets [n, H, W, 3] -> ``{'levels': [H, ..., 16], 'swd':
    [one value per level], 'avg', 'n', 'seed', 'nhoods', 'dir_repeats', 'dirs_per_repeat'}``.  ``draws``: what
    ``swd.draws`` returns (default: ``draws(seed, ...)``), so that two implementations can be handed the same numbers.
    Refusals come before any allocation: sets that are not CUDA uint8 [n, H, W, 3] (RuntimeError) or empty, images that are
    not square, whose side is no power of two or below 16, unequal counts (ValueError).  A channel without variance at some
    level raises ValueError (one host read per level)."""
    n, levels = check_sets(real_u8, fake_u8)
    check_settings(n, nhoods, dir_repeats, dirs_per_repeat)
    D = _draws(seed, n, levels, nhoods, dir_repeats, dirs_per_repeat) if draws is None else draws
    check_draws(D, n, levels, nhoods, dir_repeats, dirs_per_repeat)
    dev = real_u8.device
    n_desc = n * nhoods
    n_pad = ops.round_up(n_desc, 4)
    count = n_desc * PATCH * PATCH
    values = []
    with torch.no_grad():
        pyr = {'real': pyramid(real_u8, len(levels)), 'fake': pyramid(fake_u8, len(levels))}
        proj = {k: torch.empty((dirs_per_repeat, n_pad), device=dev, dtype=torch.float32) for k in pyr}
        total = torch.zeros((1,), device=dev, dtype=torch.float64)
        for li, (res, lv) in enumerate(zip(levels, D)):
            bank, stats = {}, torch.empty((2, 6), device=dev, dtype=torch.float64)
            for j, k in enumerate(('real', 'fake')):
                cx, cy = _centres(lv[k], dev)
                bank[k], _ = ops.swd_gather(pyr[k][li], cx, cy, nhoods, stats=stats[j])
                pyr[k][li] = None                                              # the level is not read again
            host = stats.cpu().numpy()                                         # the level's one host read
            norm = {}
            for j, k in enumerate(('real', 'fake')):
                mu, sigma = channel_stats(host[j], count)
                if not np.all(np.isfinite(sigma)) or np.any(sigma <= 0.0):
                    raise ValueError('swd: a channel of the %s set has no variance at level %d (sigma = %s)' % (k, res, sigma.tolist()))
                norm[k] = (mu, sigma)
            total.zero_()
            for r in range(dir_repeats):
                shift = {}
                for k in ('real', 'fake'):
                    rows, shift[k] = projection_operands(np.asarray(lv['dirs'][r], np.float64), *norm[k])
                    features.similarities(torch.from_numpy(rows).to(dev), bank[k], proj[k])
                    ops.swd_sort_rows(proj[k], n_desc)
                off = torch.from_numpy(shift['real'] - shift['fake']).to(dev)
                ops.swd_absdiff_sums(proj['real'], proj['fake'], n_desc, row_offset=off, out=total, accumulate=True)
            values.append(float(total.item()) / (dir_repeats * dirs_per_repeat * n_desc) * 1e3)
            del bank
    return {'levels': [int(r) for r in levels], 'swd': values, 'avg': float(np.mean(values)), 'n': n, 'seed': int(seed),
            'nhoods': int(nhoods), 'dir_repeats': int(dir_repeats), 'dirs_per_repeat': int(dirs_per_repeat)}


def csv_head(levels):
    return 'step,' + ','.join('swd_%d' % r for r in levels) + ',swd_avg'


def csv_line(step, out):
    return '%d,' % step + ','.join('%.6f' % v for v in out['swd']) + ',%.6f' % out['avg']


def log_line(step, out):
    return '[Steps %7d] [SWD x1e3 %s] [avg %.3f]' % (step, ' '.join('%d: %.3f' % (r, v) for r, v in zip(out['levels'], out['swd'])),
                                                   out['avg'])


class SWDMonitor(WeightsMonitor):
    """``--swd_data`` on rank 0: the sliced Wasserstein distance of the training generator's weights from the first ``n``
    real images at every evaluation, appended as ``step,swd_<res>...,swd_avg`` to ``swd_<eval_seed>.csv`` (evaluate/gan.py's
    ``WeightsMonitor``).  No encoder: it needs none of the ``--prdc_*`` flags.  The fakes come from fixed latents of the eval
    seed (``features.sample_u8``) and the draws from the same seed, so two evaluations differ by the weights alone.  The real
    set goes to the device once.  It records only: there is no ``*_best.pt`` choice."""

    def __init__(self, logdir, architecture, image_size, device, seed, data_path, n=8192, batch=500, P=None, nhoods=128,
                 dir_repeats=4, dirs_per_repeat=128):
        real = load_x_train(data_path, image_size, 'generator makes')
        if real.shape[1] != real.shape[2]:
            raise ValueError('swd: %s holds %d x %d images, square images expected' % (data_path, real.shape[1], real.shape[2]))
        self.levels = levels_of(real.shape[1])
        self.n, self.batch = min(int(n), len(real)), int(batch)
        check_settings(self.n, nhoods, dir_repeats, dirs_per_repeat)
        self.settings = dict(nhoods=int(nhoods), dir_repeats=int(dir_repeats), dirs_per_repeat=int(dirs_per_repeat))
        self.real = torch.from_numpy(real[:self.n]).to(device)
        super().__init__(logdir, device, seed, own_network('G', architecture, image_size, device, P),
                         [('swd_%d.csv', csv_head(self.levels), csv_line)], which='G')

    def evaluate(self):
        fake = features.sample_u8(self.G, self.n, self.batch, self.eval_seed)
        return swd_of(self.real, fake, seed=self.eval_seed, **self.settings)


# ---- the training scripts' hook ----
def _refusals(H, P):
    if H.swd_data and H.swd_n < 1:
        raise ValueError('--swd_n must be at least 1, got %r' % (H.swd_n,))


HOOK = Hook(
    flags=(('swd_data', None, dict(type=str, help='npz with x_train uint8 [n, H, W, 3]: rank 0 appends the sliced Wasserstein distance (Laplacian-pyramid '
                                                  'patches, no encoder) of the generator from these images, one value per resolution level and their '
                                                  'average, to swd_<seed>.csv at every evaluate_every; the training trajectory is unchanged')),
           ('swd_n', 8192, dict(type=int, help='with --swd_data: the first N images of x_train against N samples (default: 8192)'))),
    switch='swd_data', refusals=_refusals,
    build=lambda H, run: SWDMonitor(*run.head, H.swd_data, n=H.swd_n, P=run.P),
    log_lines=lambda monitor, step, out: [log_line(step, out)])
add_hook_arguments, check_hook_arguments = HOOK.add_arguments, HOOK.check


# ---- the command line (test_swd.py) ----
def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: sliced Wasserstein distance of generated images from real ones on '
                                        'Laplacian-pyramid patches (no encoder; one process, one GPU)')
    parser.add_argument('--real', required=True, type=str, help='npz with x_train uint8 [n, H, W, 3]')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--fake', default=None, type=str, help='npz with images uint8 [n, H, W, 3] (samples.npz of test_gan_sample.py)')
    src.add_argument('--gen', default=None, type=str, help='generator checkpoint to sample from at fixed latents of --seed')
    parser.add_argument('--gen_arch', default=None, type=str, help="with --gen: the generator's architecture")
    parser.add_argument('--n', default=None, type=int,
                        help='images per set, the first N of each file (default: min(len(real), len(fake), %d))' % MAX_N)
    parser.add_argument('--nhoods', default=128, type=int, help='patches per image and level (default: 128)')
    parser.add_argument('--dir_repeats', default=4, type=int, help='repeats of the random directions (default: 4)')
    parser.add_argument('--dirs', default=128, type=int, help='directions per repeat (default: 128)')
    parser.add_argument('--batch_size', default=500, type=int, help='with --gen: images per forward (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help='seed of the positions, the directions and, with --gen, the latents')
    P = parser.parse_args(argv)
    if P.gen and not P.gen_arch:
        parser.error('--gen needs --gen_arch')
    if P.fake and P.gen_arch:
        parser.error('--gen_arch does nothing without --gen')
    return P


def main(argv=None):
    """Prints one line and writes ``swd_<seed>.json`` next to the fakes (the generator checkpoint with ``--gen``); returns
    that path."""
    P = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('The sliced Wasserstein distance runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.batch_size < 1:
        raise ValueError('--batch_size must be at least 1, got %r' % (P.batch_size,))
    if P.n is not None and P.n < 1:
        raise ValueError('--n must be at least 1, got %r' % (P.n,))
    check_settings(1, P.nhoods, P.dir_repeats, P.dirs)
    real = features.load_images(P.real, 'x_train')
    if real.shape[1] != real.shape[2]:
        raise ValueError('%s holds %d x %d images, square images expected' % (P.real, real.shape[1], real.shape[2]))
    levels_of(real.shape[1])
    if P.fake:
        fake = features.load_images(P.fake, 'images')
        if tuple(fake.shape[1:]) != tuple(real.shape[1:]):
            raise ValueError('%s holds %s images, %s holds %s' % (P.real, tuple(real.shape[1:]), P.fake, tuple(fake.shape[1:])))
        n = min(len(real), len(fake), MAX_N) if P.n is None else P.n
        if n > min(len(real), len(fake)):
            raise ValueError('--n %d: %s holds %d images, %s holds %d' % (n, P.real, len(real), P.fake, len(fake)))
        fake = torch.from_numpy(fake[:n]).to(dev)
    else:
        from .models.gan import get_architecture
        n = min(len(real), MAX_N) if P.n is None else P.n
        if n > len(real):
            raise ValueError('--n %d: %s holds %d images' % (n, P.real, len(real)))
        G = features.load_frozen(get_architecture(P.gen_arch, tuple(real.shape[1:]))[0], P.gen, dev)
        fake = features.sample_u8(G, n, P.batch_size, seed)
    out = swd_of(torch.from_numpy(real[:n]).to(dev), fake, seed=seed, nhoods=P.nhoods, dir_repeats=P.dir_repeats,
                 dirs_per_repeat=P.dirs)
    print('[SWD x1e3 over %d images] %s [avg %.4f]' % (n, ' '.join('[%d: %.4f]' % (r, v) for r, v in zip(out['levels'], out['swd'])),
                                                     out['avg']), flush=True)
    path = os.path.join(Path(P.fake or P.gen).parent, 'swd_%d.json' % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    return path
