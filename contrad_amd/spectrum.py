"""Radial power spectrum of generated images against real ones: the azimuthally averaged power of the luma (Durall et al.,
Watch your Up-Convolution, CVPR 2020, and the later frequency-bias papers).  Like SWD it reads uint8 images alone (DESIGN.md
sections 8 and 23), so it means the same for every architecture, encoder and repository that shares the definition; unlike SWD
it looks at the up-sampling artefacts directly: a stride-2 transposed convolution's checkerboard lands on the Nyquist points
of the 2-D spectrum, a too-soft FIR up-sampler shows as a deficit in the high band.

The definition.  A set of n >= 1 uint8 images [n, S, S, 3], S a power of two, 16 <= S <= 512.
  1. luma, exact: Y = (77 R + 150 G + 29 B) / 256 on the values 0 ... 255 (the numerator is at most 65 280: no rounding in fp32).
  2. transform: F[u, v] = sum_{y, x} Y[y, x] exp(-2 pi i (u y + v x) / S), u along H and v along W, kept as the half spectrum
     u = 0 ... S - 1, v = 0 ... S / 2 (``numpy.fft.rfft2``'s layout).  The power is P = |F|^2 / S^4, so P[0, 0] is the squared mean.
  3. radial bins, in integers: fu = u if u <= S / 2 else u - S, likewise fv, r2 = fu^2 + fv^2; the bin k is the unique integer
     with (2 k - 1)^2 <= 4 r2 < (2 k + 1)^2, and k = 0 for r2 = 0 -- round(sqrt(r2)) without a floating-point tie (the right side
     is odd, 4 r2 even).  All frequencies are kept, the corners included: kmax = bin(S / 2, S / 2) = 11, 23, 45, 91, 181, 362 for
     S = 16 ... 512 and K = kmax + 1; the corner (S / 2, S / 2) is where a checkerboard lands.  A_i[k] is the mean of P_i over
     the full S x S grid's members of bin k: on the half spectrum, weight 1 for the columns v = 0 and v = S / 2 and weight 2
     otherwise, divided by the full-grid count.
  4. per set: mean[k] = mean_i A_i[k], and the mean 2-D map M[u, v] = mean_i P_i[u, v] on the half spectrum.  Everything after
     the transform -- the squares, the bin sums, the sums over images -- is formed and added in float64 in a fixed order.
  5. real against fake (the counts need not be equal): R[k] = 10 log10(mean_fake[k] / mean_real[k]);
     lsd_db = sqrt(mean_{k = 1 ... kmax} R[k]^2), the log-spectral distance without DC; hf_db = mean_{S / 4 < k <= kmax} R[k]
     (positive: too much fine energy); nyquist_db = 10 log10(M_fake / M_real) at (u, v) = (0, S / 2), (S / 2, 0), (S / 2, S / 2)
     -- alternating columns, alternating rows, checkerboard.  A bin or Nyquist point whose real or fake mean is 0 raises
     ValueError.  floor_db is the same lsd_db between the even-indexed and the odd-indexed real images: the noise floor to
     read lsd_db against.

On the device (csrc/spectral/spectrum.hip): the half-spectrum FFT (``ops.spec_rfft2``: the host passes the fp32 twiddle table,
the device calls no sine), the radial means (``ops.spec_radial``: the host passes the bin table and the reciprocal counts, the
device takes no square root) and the sum of the 2-D power over images (``ops.spec_mean_map``), fed in chunks of images so that
the fp32 spectrum of a chunk stays below 1 GiB.  The means over images and step 5 are float64 numpy on the host.

The figure of the command line (``--figure``): an 8-bit grey PNG of S rows and 3 S columns -- log10 M_real, log10 M_fake and
their difference, each half spectrum mirrored to S x S with DC in the centre (row S / 2, column S / 2).  The first two panels
share one linear scale: grey 0 at the smallest and 255 at the largest log10 value of the two maps together (entries that are 0
count as the smallest positive one).  The third shows log10(M_fake / M_real) clipped to [-1, 1] (-10 ... +10 dB) with 0 at grey
128 and 127 grey levels per unit.
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

MIN_SIDE, MAX_SIDE = 16, 512
MAX_N = 16384                               # the command line's default cap per set
SPEC_BYTES = 1 << 30                        # the default chunk keeps the fp32 half spectrum below this

_tables, _twiddles, _device = {}, {}, {}


def check_side(S):
    S = int(S)
    if S < MIN_SIDE or S > MAX_SIDE or S & (S - 1):
        raise ValueError('spectrum: the image side must be a power of two in [%d, %d], got %d' % (MIN_SIDE, MAX_SIDE, S))
    return S


def bin_table(S):
    """(bin_of int32 [S, S / 2 + 1], K, counts int64 [K]) of step 3, in integers; ``counts`` are the full S x S grid's.  Cached:
    do not write to the arrays."""
    S = check_side(S)
    if S not in _tables:
        u = np.arange(S, dtype=np.int64)
        fu = np.where(u <= S // 2, u, u - S)[:, None]
        fv = np.arange(S // 2 + 1, dtype=np.int64)[None, :]
        r4 = 4 * (fu * fu + fv * fv)
        k = (np.sqrt(r4.astype(np.float64)).astype(np.int64) + 1) // 2
        k = np.where((2 * k - 1) ** 2 > r4, k - 1, k)                        # (the float square root may be one off)
        k = np.where((2 * k + 1) ** 2 <= r4, k + 1, k)
        k[0, 0] = 0
        assert np.all(((2 * k - 1) ** 2 <= r4) & (r4 < (2 * k + 1) ** 2) | (r4 == 0))
        K = int(k[S // 2, S // 2]) + 1
        w = np.full(k.shape, 2, np.int64)
        w[:, 0] = w[:, S // 2] = 1
        counts = np.bincount(k.ravel(), weights=w.ravel(), minlength=K).astype(np.int64)
        _tables[S] = (np.ascontiguousarray(k.astype(np.int32)), K, counts)
    return _tables[S]


def twiddles(S):
    """fp32 [S / 2, 2]: (cos, -sin)(2 pi j / S) rounded from float64; the quarter turns are exact.  Cached."""
    S = check_side(S)
    if S not in _twiddles:
        a = 2.0 * np.pi * np.arange(S // 2, dtype=np.float64) / S
        t = np.stack([np.cos(a), -np.sin(a)], axis=1)
        t[0] = (1.0, 0.0)
        t[S // 4] = (0.0, -1.0)
        _twiddles[S] = np.ascontiguousarray(t.astype(np.float32))
    return _twiddles[S]


def device_tables(S, device):
    """(twiddles, bin_of, reciprocal counts) on ``device``, made once per (S, device)."""
    key = (int(S), str(device))
    if key not in _device:
        table, _K, counts = bin_table(S)
        _device[key] = (torch.from_numpy(twiddles(S)).to(device), torch.from_numpy(table).to(device),
                        torch.from_numpy(1.0 / counts.astype(np.float64)).to(device))
    return _device[key]


def check_set(x_u8, what='given'):
    """The refusals of ``spectrum_of``, in order -> (n, S)."""
    features.check_u8(x_u8, what, 'spectrum')
    if x_u8.shape[1] != x_u8.shape[2]:
        raise ValueError('spectrum: the %s images are %d x %d, square images expected' % (what, x_u8.shape[1], x_u8.shape[2]))
    return int(x_u8.shape[0]), check_side(x_u8.shape[1])


def default_chunk(S):
    return max(1, SPEC_BYTES // (S * (S // 2 + 1) * 8))


def spectrum_of(x_u8, chunk=None):
    """Steps 1 to 4 for a device-resident uint8 set [n, S, S, 3] -> ``{'S', 'n', 'K', 'profiles': A_i[k] as float64 [n, K] on
    the device, 'mean': float64 numpy [K], 'map': float64 numpy [S, S / 2 + 1]}``.  ``chunk``: images per transform (default:
    what keeps the fp32 spectrum below 1 GiB).  Refusals come before any allocation: a set that is not CUDA uint8
    [n, H, W, 3] (RuntimeError) or empty, images that are not square or whose side is no power of two in [16, 512], a chunk
    below 1 (ValueError)."""
    n, S = check_set(x_u8)
    chunk = default_chunk(S) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError('spectrum: chunk must be at least 1, got %r' % (chunk,))
    chunk = min(chunk, n)
    dev = x_u8.device
    _table, K, _counts = bin_table(S)
    with torch.no_grad():
        tw, bins, rcount = device_tables(S, dev)
        x_u8 = x_u8.contiguous()
        spec = torch.empty((chunk, S, S // 2 + 1, 2), device=dev, dtype=torch.float32)
        profiles = torch.empty((n, K), device=dev, dtype=torch.float64)
        total = torch.empty((S, S // 2 + 1), device=dev, dtype=torch.float64)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            ops.spec_rfft2(x_u8[i:i + m], tw, out=spec[:m])
            ops.spec_radial(spec[:m], bins, rcount, out=profiles[i:i + m])
            ops.spec_mean_map(spec[:m], out=total, accumulate=i > 0)
        mean = profiles.cpu().numpy().sum(axis=0) / n
        M = total.cpu().numpy() / n
    return {'S': S, 'n': n, 'K': K, 'profiles': profiles, 'mean': mean, 'map': M}


def nyquist_points(S):
    return ((0, S // 2), (S // 2, 0), (S // 2, S // 2))


def log_ratio_db(fake, real, what):
    fake, real = np.asarray(fake, np.float64), np.asarray(real, np.float64)
    if not (np.all(np.isfinite(fake)) and np.all(np.isfinite(real)) and np.all(fake > 0.0) and np.all(real > 0.0)):
        raise ValueError('spectrum: %s without power in the real or the fake set (real %s, fake %s)'
                         % (what, real[~(real > 0.0)].tolist(), fake[~(fake > 0.0)].tolist()))
    return 10.0 * np.log10(fake / real)


def lsd_of(R):
    return float(np.sqrt(np.mean(np.square(R[1:]))))


def floor_of(profiles):
    """lsd_db between the even-indexed and the odd-indexed images of per-image profiles [n, K] (None below two images)."""
    p = profiles.cpu().numpy() if torch.is_tensor(profiles) else np.asarray(profiles, np.float64)
    if p.shape[0] < 2:
        return None
    return lsd_of(log_ratio_db(p[1::2].sum(axis=0) / p[1::2].shape[0], p[0::2].sum(axis=0) / p[0::2].shape[0], 'a radial bin'))


def compare(real, fake):
    """Step 5 for two results of ``spectrum_of`` -> ``{'S', 'K', 'n_real', 'n_fake', 'R': [K], 'lsd_db', 'hf_db',
    'nyquist_db': [3], 'floor_db'}``.  ``floor_db`` comes from ``real['profiles']``, or is ``real['floor_db']`` where the
    profiles were not kept (None when neither is there)."""
    if real['S'] != fake['S']:
        raise ValueError('spectrum: real images of side %d against fake images of side %d' % (real['S'], fake['S']))
    S, K = real['S'], real['K']
    R = log_ratio_db(fake['mean'], real['mean'], 'a radial bin')
    pts = nyquist_points(S)
    nyq = log_ratio_db([fake['map'][p] for p in pts], [real['map'][p] for p in pts], 'a Nyquist point')
    floor = floor_of(real['profiles']) if real.get('profiles') is not None else real.get('floor_db')
    return {'S': S, 'K': K, 'n_real': int(real['n']), 'n_fake': int(fake['n']), 'R': [float(v) for v in R], 'lsd_db': lsd_of(R),
            'hf_db': float(np.mean(R[S // 4 + 1:])), 'nyquist_db': [float(v) for v in nyq], 'floor_db': floor}


def compare_or_nan(real, fake):
    """``compare`` for a monitor: where a radial bin or a Nyquist point has no power (a collapsed or saturated generator
    that emits constant images, say) the five numbers and ``R`` are nan instead of an exception, so that a hook that only
    records cannot end a training run.  Sets of two sizes are still refused."""
    try:
        return compare(real, fake)
    except ValueError:
        if real['S'] != fake['S']:
            raise
        nan = float('nan')
        return {'S': real['S'], 'K': real['K'], 'n_real': int(real['n']), 'n_fake': int(fake['n']), 'R': [nan] * real['K'],
                'lsd_db': nan, 'hf_db': nan, 'nyquist_db': [nan, nan, nan], 'floor_db': real.get('floor_db')}


CSV_HEAD = 'step,lsd_db,hf_db,nyq_h,nyq_v,nyq_d'


def csv_line(step, out):
    return '%d,%.6f,%.6f,' % (step, out['lsd_db'], out['hf_db']) + ','.join('%.6f' % v for v in out['nyquist_db'])


def log_line(step, out):
    return '[Steps %7d] [Spectrum LSD %.3f dB (floor %s)] [HF %+.3f dB] [Nyquist h %+.2f v %+.2f d %+.2f dB]' % (
        (step, out['lsd_db'], 'n/a' if out['floor_db'] is None else '%.3f' % out['floor_db'], out['hf_db']) + tuple(out['nyquist_db']))


class SpectrumMonitor(WeightsMonitor):
    """``--spectrum_data`` on rank 0: the radial power spectrum of the training generator's weights against the first ``n``
    real images at every evaluation, appended as ``step,lsd_db,hf_db,nyq_h,nyq_v,nyq_d`` to ``spectrum_<eval_seed>.csv``
    (evaluate/gan.py's ``WeightsMonitor``).  No encoder: it needs none of the ``--prdc_*`` flags.  The fakes come from fixed
    latents of the eval seed (``features.sample_u8``), so two evaluations differ by the weights alone.  The real
    side is one fixed curve: the real set is transformed once, here, and only its mean curve, its mean map and its noise
    floor are kept.  It records only: there is no ``*_best.pt`` choice, and an evaluation at which some bin or Nyquist point of
    the fakes has no power (``compare`` raises ValueError there) is recorded as a row of nan (``compare_or_nan``), not raised into
    the training loop.  A real set without power in some bin is refused here, in ``__init__``."""

    def __init__(self, logdir, architecture, image_size, device, seed, data_path, n=8192, batch=500, P=None):
        real = load_x_train(data_path, image_size, 'generator makes')
        if real.shape[1] != real.shape[2]:
            raise ValueError('spectrum: %s holds %d x %d images, square images expected' % (data_path, real.shape[1], real.shape[2]))
        check_side(real.shape[1])
        if int(n) < 1:
            raise ValueError('spectrum: n must be at least 1, got %r' % (n,))
        self.n, self.batch = min(int(n), len(real)), int(batch)
        out = spectrum_of(torch.from_numpy(real[:self.n]).to(device))
        self.real = {'S': out['S'], 'n': out['n'], 'K': out['K'], 'mean': out['mean'], 'map': out['map'],
                     'floor_db': floor_of(out['profiles'])}
        log_ratio_db(self.real['mean'], self.real['mean'], 'a radial bin of the real set')     # (refused once, before the run)
        corners = [self.real['map'][p] for p in nyquist_points(out['S'])]
        log_ratio_db(corners, corners, 'a Nyquist point of the real set')
        super().__init__(logdir, device, seed, own_network('G', architecture, image_size, device, P),
                         [('spectrum_%d.csv', CSV_HEAD, csv_line)], which='G')

    def evaluate(self):
        fake = features.sample_u8(self.G, self.n, self.batch, self.eval_seed)
        return compare_or_nan(self.real, spectrum_of(fake))


# ---- the training scripts' hook ----
def _refusals(H, P):
    if H.spectrum_data and H.spectrum_n < 1:
        raise ValueError('--spectrum_n must be at least 1, got %r' % (H.spectrum_n,))


HOOK = Hook(
    flags=(('spectrum_data', None, dict(type=str, help='npz with x_train uint8 [n, S, S, 3]: rank 0 appends the radial power spectrum of the generator against '
                                                       'these images (log-spectral distance, high-band level and the three Nyquist points in dB; no encoder) '
                                                       'to spectrum_<seed>.csv at every evaluate_every; the training trajectory is unchanged')),
           ('spectrum_n', 8192, dict(type=int, help='with --spectrum_data: the first N images of x_train against N samples (default: 8192)'))),
    switch='spectrum_data', refusals=_refusals,
    # (the real set is transformed once, in the constructor)
    build=lambda H, run: SpectrumMonitor(*run.head, H.spectrum_data, n=H.spectrum_n, P=run.P),
    log_lines=lambda monitor, step, out: [log_line(step, out)])
add_hook_arguments, check_hook_arguments = HOOK.add_arguments, HOOK.check


# ---- the command line (test_spectrum.py) ----
def full_map(M):
    """The half spectrum [S, S / 2 + 1] mirrored to [S, S] with DC at (S / 2, S / 2)."""
    S = M.shape[0]
    full = np.empty((S, S), np.float64)
    full[:, :S // 2 + 1] = M
    u = (S - np.arange(S)) % S
    full[:, S // 2 + 1:] = M[u][:, S // 2 - 1:0:-1]                            # F[u, v] = conj F[-u, -v]
    return np.fft.fftshift(full)


def figure(real_map, fake_map):
    """The grey image uint8 [S, 3 S, 3] that the module docstring describes."""
    a, b = full_map(real_map), full_map(fake_map)
    tiny = min(a[a > 0].min() if (a > 0).any() else 1.0, b[b > 0].min() if (b > 0).any() else 1.0)
    la, lb = np.log10(np.maximum(a, tiny)), np.log10(np.maximum(b, tiny))
    lo, hi = min(la.min(), lb.min()), max(la.max(), lb.max())
    scale = 255.0 / (hi - lo) if hi > lo else 0.0
    ratio = 128.0 + 127.0 * np.clip(lb - la, -1.0, 1.0)
    grey = np.concatenate([(la - lo) * scale, (lb - lo) * scale, ratio], axis=1)
    grey = np.clip(np.floor(grey + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))


def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: radial power spectrum of generated images against real ones '
                                        '(no encoder; one process, one GPU)')
    parser.add_argument('--real', required=True, type=str, help='npz with x_train uint8 [n, S, S, 3]')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--fake', default=None, type=str, help='npz with images uint8 [n, S, S, 3] (samples.npz of test_gan_sample.py)')
    src.add_argument('--gen', default=None, type=str, help='generator checkpoint to sample from at fixed latents of --seed')
    parser.add_argument('--gen_arch', default=None, type=str, help="with --gen: the generator's architecture")
    parser.add_argument('--n_real', default=None, type=int, help='the first N real images (default: min(len(real), %d))' % MAX_N)
    parser.add_argument('--n_fake', default=None, type=int,
                        help='the first N fakes of --fake, or N samples of --gen (default: min(len(fake), %d); with --gen: n_real)' % MAX_N)
    parser.add_argument('--batch_size', default=500, type=int, help='with --gen: images per forward (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help="the tag of the output files and, with --gen, the latents' seed")
    parser.add_argument('--figure', action='store_true',
                        help='also write spectrum_<seed>.png: log10 mean maps of real, of fake and their ratio, DC in the centre')
    P = parser.parse_args(argv)
    if P.gen and not P.gen_arch:
        parser.error('--gen needs --gen_arch')
    if P.fake and P.gen_arch:
        parser.error('--gen_arch does nothing without --gen')
    return P


def main(argv=None):
    """Prints one line and writes ``spectrum_<seed>.json`` next to the fakes (the generator checkpoint with ``--gen``), with
    ``--figure`` also ``spectrum_<seed>.png``; returns the json's path."""
    P = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('The power spectrum runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.batch_size < 1:
        raise ValueError('--batch_size must be at least 1, got %r' % (P.batch_size,))
    for name in ('n_real', 'n_fake'):
        if getattr(P, name) is not None and getattr(P, name) < 1:
            raise ValueError('--%s must be at least 1, got %r' % (name, getattr(P, name)))
    real = features.load_images(P.real, 'x_train')
    if real.shape[1] != real.shape[2]:
        raise ValueError('%s holds %d x %d images, square images expected' % (P.real, real.shape[1], real.shape[2]))
    check_side(real.shape[1])
    n_real = min(len(real), MAX_N) if P.n_real is None else P.n_real
    if n_real > len(real):
        raise ValueError('--n_real %d: %s holds %d images' % (n_real, P.real, len(real)))
    if P.fake:
        fake = features.load_images(P.fake, 'images')
        if tuple(fake.shape[1:]) != tuple(real.shape[1:]):
            raise ValueError('%s holds %s images, %s holds %s' % (P.real, tuple(real.shape[1:]), P.fake, tuple(fake.shape[1:])))
        n_fake = min(len(fake), MAX_N) if P.n_fake is None else P.n_fake
        if n_fake > len(fake):
            raise ValueError('--n_fake %d: %s holds %d images' % (n_fake, P.fake, len(fake)))
        fake = torch.from_numpy(fake[:n_fake]).to(dev)
    else:
        from .models.gan import get_architecture
        n_fake = n_real if P.n_fake is None else P.n_fake
        G = features.load_frozen(get_architecture(P.gen_arch, tuple(real.shape[1:]))[0], P.gen, dev)
        fake = features.sample_u8(G, n_fake, P.batch_size, seed)
    sr, sf = spectrum_of(torch.from_numpy(real[:n_real]).to(dev)), spectrum_of(fake)
    out = compare(sr, sf)
    out.update(seed=int(seed), mean_real=[float(v) for v in sr['mean']], mean_fake=[float(v) for v in sf['mean']])
    print('[Spectrum of %d fakes against %d reals at %d x %d] [LSD %.4f dB (floor %s)] [HF %+.4f dB] [Nyquist h %+.3f v %+.3f d %+.3f dB]'
          % ((n_fake, n_real, out['S'], out['S'], out['lsd_db'], 'n/a' if out['floor_db'] is None else '%.4f' % out['floor_db'],
              out['hf_db']) + tuple(out['nyquist_db'])), flush=True)
    where = Path(P.fake or P.gen).parent
    path = os.path.join(where, 'spectrum_%d.json' % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    if P.figure:
        from . import hostio
        hostio.write_png(os.path.join(where, 'spectrum_%d.png' % seed), figure(sr['map'], sf['map']))
    return path
