"""Latent-space tools: truncation, style mixing, walks and perceptual path length (Karras et al. 2019, 2020).  Everything
else in the repository looks at where a generator's samples land; this module looks at how G gets there and lets a user steer
it.  An ADDITION of this project: the reference has no truncation, interpolation or path length.

Path length.  n pairs of latents an exact ``eps`` apart on a path between two draws of the prior, both ends through G at one
shared noise list, both float images through the penultimate layer of a frozen encoder E, then

    d_i = |f^(x_i(t)) - f^(x_i(t + eps))|^2 / eps^2,    f^ = f / max(|f|, 1e-12),

and ``ppl`` = the mean of the d_i with lo <= d_i <= hi, lo = np.percentile(d, 1, 'lower'), hi = np.percentile(d, 99, 'higher')
(Karras' rule); ``ppl_raw`` is the mean of all.  The feature space is this project's frozen discriminator, not LPIPS: the number
is comparable only under one encoder file, and never with the papers' LPIPS-based PPL.

  * ``space='z'``: slerp between two Gaussian draws (StyleGAN2), lerp between two draws of SNDCGAN's uniform cube (which keeps
    the points in the prior's support).  ``space='w'``: StyleGAN2 only; both endpoints through the mapping network, lerp in W.
  * ``sampling='full'``: t ~ U(0, 1); ``'end'``: t = 0 (Karras' code for W).
  * t + eps is formed in float64, the slerp's angle is atan2, never acos, and both ends of a pair share every intermediate
    (``ops.latent_pair``); the distance takes the difference first, in float64 (``ops.pair_dist``): at eps = 1e-4 the
    similarity form 2 - 2 s of the other evaluators is pure cancellation, and the quotient by eps^2 is a factor of 1e8.
  * The images never pass through ``ops.images_u8``: quantisation erases an eps step.
  * ``DEFAULT_EPS`` = 1e-4 is the papers'; see DESIGN.md 24 for the eps sweep that it rests on.

Truncation and mixing (StyleGAN2 only: the other generators have no W).  ``truncated`` and ``mixed`` build per-layer latents
[B, n_latent, D] through ``ops.latent_styles`` for ``G(latents, input_is_latent=True)``.
"""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import ops
from .evaluate.gan import WeightsMonitor, fixed_latent, frozen_encoder, own_network, preserved_rng
from .hooks import Hook
from .hostio import upload

DEFAULT_EPS = 1e-4
MIN_N = 100                                 # the 1 % rule needs at least 100 values
STYLE_ARCHITECTURES = ('stylegan2', 'stylegan2_512')
NOTE = ('path length in the penultimate features of one frozen discriminator: comparable only between generators measured '
        'under the same encoder file, never with LPIPS-based PPL')


def has_w(G):
    return hasattr(G, 'style_dim') and hasattr(G, 'get_latent')


def need_w(G, what):
    if not has_w(G):
        raise ValueError('latent.%s: %s has no W (no mapping network): StyleGAN2 generators only' % (what, type(G).__name__))


def check_space(architecture, space):
    """The refusal that needs no device: W exists for the StyleGAN2 architectures alone."""
    if space not in ('z', 'w'):
        raise ValueError("space must be 'z' or 'w', got %r" % (space,))
    if space == 'w' and architecture not in STYLE_ARCHITECTURES:
        raise ValueError("space 'w' needs a mapping network: %s has no W (StyleGAN2 only)" % architecture)


def check_truncation(architecture, psi):
    if psi is not None and architecture not in STYLE_ARCHITECTURES:
        raise ValueError('truncation moves w towards its mean: %s has no W (StyleGAN2 only)' % architecture)


def check_ppl_arguments(n, eps, sampling='full', batch=1):
    if not (isinstance(eps, float) and np.isfinite(eps) and eps > 0.0):
        raise ValueError('eps must be a positive float, got %r' % (eps,))
    if int(n) < MIN_N:
        raise ValueError('n must be at least %d (the 1 %% rule drops the tails of at least 100 values), got %r' % (MIN_N, n))
    if sampling not in ('full', 'end'):
        raise ValueError("sampling must be 'full' or 'end', got %r" % (sampling,))
    if int(batch) < 1:
        raise ValueError('batch must be at least 1, got %r' % (batch,))


# ---- pairs ----
def endpoints(G, n, seed, sampling='end'):
    """(a, b, t): ``fixed_latent(G, 2 n, seed)`` cut into the two ends, and t as float64 numpy [n] from the same CPU generator
    behind them (``sampling='full'``: U(0, 1); ``'end'``: zeros, nothing drawn)."""
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    z = fixed_latent(G, 2 * n, seed, generator=g)
    t = torch.rand(n, generator=g, dtype=torch.float64).numpy() if sampling == 'full' else np.zeros(n, np.float64)
    return z[:n].contiguous(), z[n:].contiguous(), t


def pairs(G, n, seed, space='z', sampling='full', eps=DEFAULT_EPS):
    """-> (x0, x1, t): the two ends of ``n`` pairs, fp32 [n, D] on G's device, ``eps`` apart in t on the path between
    ``fixed_latent(G, 2 n, seed)[:n]`` and ``[n:]``, and t as fp32 on the device.  ``space='z'``: points of Z (slerp for a
    Gaussian prior, lerp for the uniform cube), to be given to ``G(z)``.  ``space='w'``: points of W (both endpoints through
    ``G.get_latent``, then lerp), to be given to ``G(w, input_is_latent=True)``; refused for a generator without W."""
    if space not in ('z', 'w'):
        raise ValueError("latent.pairs: space must be 'z' or 'w', got %r" % (space,))
    if space == 'w':
        need_w(G, "pairs(space='w')")
    if sampling not in ('full', 'end'):
        raise ValueError("latent.pairs: sampling must be 'full' or 'end', got %r" % (sampling,))
    if int(n) < 1:
        raise ValueError('latent.pairs: n must be at least 1, got %r' % (n,))
    a, b, t64 = endpoints(G, int(n), seed, sampling)
    t = upload(torch.from_numpy(t64).float().view(-1, 1), a.device).view(-1)
    gaussian = hasattr(G, 'style_dim')
    with torch.no_grad():
        if space == 'w':
            a, b = G.get_latent(a).contiguous(), G.get_latent(b).contiguous()
        x0, x1 = ops.latent_pair(a, b, t, float(eps), 1 if (space == 'z' and gaussian) else 0)
    return x0, x1, t


# ---- truncation and mixing ----
def psi_vector(G, psi, cutoff=None):
    """fp32 [n_latent] on the CPU: ``psi`` in the layers below ``cutoff`` (None: all) and 1 behind."""
    L = G.n_latent
    cutoff = L if cutoff is None else int(cutoff)
    if not 0 <= cutoff <= L:
        raise ValueError('latent: the truncation cutoff must lie in [0, %d], got %r' % (L, cutoff))
    v = torch.ones(L)
    v[:cutoff] = float(psi)
    return v


def _styles(G, w, w2, cross, psi, w_avg, cutoff):
    dev = w.device
    kw = {}
    if w2 is not None:
        cross = torch.as_tensor(cross).float().view(-1)
        if cross.numel() == 1:
            cross = cross.expand(w.shape[0])
        if cross.numel() != w.shape[0] or bool((cross < 0).any()) or bool((cross > G.n_latent).any()):
            raise ValueError('latent.mixed: one crossover layer in [0, %d] per row expected' % G.n_latent)
        kw.update(w2=w2.contiguous(), cross=upload(cross.contiguous().view(-1, 1), dev).view(-1))
    if psi is not None:
        if w_avg is None:
            raise ValueError('latent: truncation needs w_avg (G.mean_latent(n))')
        kw.update(w_avg=w_avg.contiguous().view(-1), psi=upload(psi_vector(G, psi, cutoff).view(-1, 1), dev).view(-1))
    return ops.latent_styles(w.contiguous(), G.n_latent, **kw)


def truncated(G, z, psi, w_avg, cutoff=None):
    """Per-layer latents [B, n_latent, D] of ``z`` with the truncation trick: ``w_avg + psi (w - w_avg)`` in the layers below
    ``cutoff`` (None: all), w itself behind.  psi = 1 gives the bits of ``G(z)``'s latents, psi = 0 those of ``w_avg``."""
    need_w(G, 'truncated')
    with torch.no_grad():
        return _styles(G, G.get_latent(z), None, None, psi, w_avg, cutoff)


def mixed(G, z_a, z_b, cross, psi=None, w_avg=None, cutoff=None):
    """Per-layer latents [B, n_latent, D]: the layers ``l < cross`` take ``z_a``'s w, the others ``z_b``'s (``cross``: one
    layer count or one per row); optionally truncated as in ``truncated``.  Each batch passes the mapping network on its own,
    as ``G(z)`` would send it: ``cross = n_latent`` then gives the bits of the unmixed latents."""
    need_w(G, 'mixed')
    if tuple(z_a.shape) != tuple(z_b.shape):
        raise ValueError('latent.mixed: z_a %s and z_b %s differ in shape' % (tuple(z_a.shape), tuple(z_b.shape)))
    with torch.no_grad():
        return _styles(G, G.get_latent(z_a), G.get_latent(z_b), cross, psi, w_avg, cutoff)


# ---- path length ----
def percentile_filter(d):
    """Karras' rule on float64 values -> (kept mask, lo, hi)."""
    d = np.asarray(d, np.float64)
    lo, hi = np.percentile(d, 1, method='lower'), np.percentile(d, 99, method='higher')
    return (lo <= d) & (d <= hi), float(lo), float(hi)


def summarise(d, eps, space, sampling, seed):
    d = np.asarray(d, np.float64)
    out = {'n': int(d.size), 'eps': float(eps), 'space': space, 'sampling': sampling, 'seed': int(seed), 'note': NOTE}
    if not np.all(np.isfinite(d)):
        out.update(ppl=float('nan'), ppl_raw=float('nan'), kept=0)
        return out
    keep, _lo, _hi = percentile_filter(d)
    out.update(ppl=float(d[keep].mean()), ppl_raw=float(d.mean()), kept=int(keep.sum()))
    return out


def shared_noise(G, seed, device):
    """One ``make_noise()`` list from the CUDA stream seeded with ``seed`` (the caller holds ``preserved_rng``); None for a
    generator without per-layer noise."""
    if not hasattr(G, 'make_noise'):
        return None
    torch.cuda.manual_seed(int(seed))
    return G.make_noise()


def images_of(G, x, space, noise):
    """The float images of latents ``x``: z through G, w through ``input_is_latent``; ``noise`` shared by all rows."""
    if space == 'w':
        return G(x, input_is_latent=True, noise=noise).contiguous().float()
    if noise is not None:
        return G(x, noise=noise).contiguous().float()
    return G(x).contiguous().float()


def pair_features(G, E, n, seed, space='z', sampling='full', eps=DEFAULT_EPS, batch=64):
    """The raw penultimate rows of both ends, fp32 [n, d] each, as ``ppl_of`` forms them."""
    if G.training or E.training:
        raise RuntimeError('latent.ppl_of: G and E must be in eval mode')
    dev = next(G.parameters()).device
    f0 = f1 = None
    with torch.no_grad(), preserved_rng(dev):
        noise = shared_noise(G, seed, dev)
        x0, x1, _t = pairs(G, n, seed, space, sampling, eps)
        for i in range(0, n, batch):
            # two calls of identical batch layout: StyleGAN2's minibatch-stddev groups of the two ends correspond
            r0 = E.penultimate(images_of(G, x0[i:i + batch], space, noise)).reshape(min(batch, n - i), -1)
            r1 = E.penultimate(images_of(G, x1[i:i + batch], space, noise)).reshape(min(batch, n - i), -1)
            if f0 is None:
                f0 = torch.empty(n, r0.shape[1], device=dev)
                f1 = torch.empty(n, r0.shape[1], device=dev)
            f0[i:i + batch].copy_(r0)
            f1[i:i + batch].copy_(r1)
    return f0, f1


def ppl_of(G, E, n, seed, space='z', sampling='full', eps=DEFAULT_EPS, batch=64):
    """Perceptual path length of ``G`` (eval mode) in the penultimate features of the frozen encoder ``E`` over ``n`` pairs of
    the fixed latents of ``seed`` -> ``{'ppl', 'ppl_raw', 'kept', 'n', 'eps', 'space', 'sampling', 'seed', 'note'}`` (module
    docstring).  The global random streams are left as they were.  Refusals come before the first launch: eps <= 0, n < 100, an
    unknown sampling, batch < 1 (ValueError), ``space='w'`` for a generator without W (ValueError), a network in train mode."""
    eps = float(eps)
    check_ppl_arguments(n, eps, sampling, batch)
    n, batch = int(n), int(batch)
    f0, f1 = pair_features(G, E, n, seed, space, sampling, eps, batch)
    d = ops.pair_dist(f0, f1, scale=1.0 / (eps * eps)).cpu().numpy()
    return summarise(d, eps, space, sampling, seed)


CSV_HEAD = 'step,ppl,ppl_raw,kept'


def csv_line(step, out):
    return '%d,%.6f,%.6f,%d' % (step, out['ppl'], out['ppl_raw'], out['kept'])


def log_line(step, out):
    return '[Steps %7d] [PPL %s %.4f (raw %.4f, kept %d of %d, eps %g)]' % (step, out['space'], out['ppl'], out['ppl_raw'],
                                                                           out['kept'], out['n'], out['eps'])


class PPLMonitor(WeightsMonitor):
    """``--ppl_encoder`` on rank 0: the path length of the training generator's weights at every evaluation, appended as
    ``step,ppl,ppl_raw,kept`` to ``ppl_<eval_seed>.csv`` (evaluate/gan.py's ``WeightsMonitor``).  Its encoder is loaded once
    and frozen; latents, t and noise come from the eval seed, so two evaluations differ by the weights alone.  It needs no
    real data and none of the other hooks' flags.  It records only: a non-finite distance is recorded as a row of nan
    (``summarise``), not raised into the training loop."""

    def __init__(self, logdir, architecture, image_size, device, seed, encoder_path, encoder_arch=None, n=2000, space='z',
                 eps=DEFAULT_EPS, batch=64, P=None):
        check_space(architecture, space)
        check_ppl_arguments(n, float(eps), 'full', batch)
        self.n, self.space, self.eps, self.batch = int(n), space, float(eps), int(batch)
        self.E = frozen_encoder(encoder_arch or architecture, image_size, encoder_path, device)
        super().__init__(logdir, device, seed, own_network('G', architecture, image_size, device, P),
                         [('ppl_%d.csv', CSV_HEAD, csv_line)], which='G')

    def evaluate(self):
        return ppl_of(self.G, self.E, self.n, self.eval_seed, self.space, 'full', self.eps, self.batch)


# ---- the training scripts' hook ----
def _refusals(H, P):
    if H.ppl_encoder:
        if H.ppl_n < MIN_N:
            raise ValueError('--ppl_n must be at least %d (the 1 %% rule), got %r' % (MIN_N, H.ppl_n))
        check_space(P.architecture, H.ppl_space)


HOOK = Hook(
    flags=(('ppl_encoder', None, dict(type=str, help='discriminator checkpoint used as the frozen feature encoder: rank 0 appends the perceptual path length of '
                                                     'the generator in its penultimate features (no real data) to ppl_<seed>.csv at every evaluate_every; '
                                                     'comparable only under one encoder file, never with LPIPS-based PPL; the training trajectory is unchanged')),
           ('ppl_encoder_arch', None, dict(type=str, help="with --ppl_encoder: the encoder's architecture (default: the run's)")),
           ('ppl_n', 2000, dict(type=int, help='with --ppl_encoder: the number of pairs (default: 2000)')),
           ('ppl_space', 'z', dict(type=str, help="with --ppl_encoder: 'z' (default) or 'w' (StyleGAN2 only)"))),
    switch='ppl_encoder', needs='FILE.pt', refusals=_refusals,
    build=lambda H, run: PPLMonitor(*run.head, H.ppl_encoder, encoder_arch=H.ppl_encoder_arch, n=H.ppl_n, space=H.ppl_space, P=run.P),
    log_lines=lambda monitor, step, out: [log_line(step, out)])
add_hook_arguments, check_hook_arguments = HOOK.add_arguments, HOOK.check


# ---- figures ----
def walk_latents(G, n_pairs, steps, seed, space='z'):
    """[n_pairs * steps, D]: row p * steps + s is the point at t = s / (steps - 1) between the p-th pair of fixed latents (the
    paths of ``pairs``: slerp or lerp in Z, lerp in W)."""
    if n_pairs < 1 or steps < 2:
        raise ValueError('latent.walk_latents: at least one pair and two steps expected, got %r, %r' % (n_pairs, steps))
    if space == 'w':
        need_w(G, "walk_latents(space='w')")
    a, b, _t = endpoints(G, n_pairs, seed)
    with torch.no_grad():
        if space == 'w':
            a, b = G.get_latent(a).contiguous(), G.get_latent(b).contiguous()
        mode = 1 if (space == 'z' and hasattr(G, 'style_dim')) else 0
        t = torch.linspace(0.0, 1.0, steps, dtype=torch.float64).float().repeat(n_pairs)
        t = upload(t.view(-1, 1), a.device).view(-1)
        x0, _x1 = ops.latent_pair(a.repeat_interleave(steps, 0).contiguous(), b.repeat_interleave(steps, 0).contiguous(), t, 0.0, mode)
    return x0


def walk_sheet(G, n_pairs=8, steps=9, seed=0, space='z', psi=None, w_avg=None, padding=2):
    """The interpolation sheet, uint8 [rows, columns, 3] on the device: one row per pair, columns at equal steps of t, all
    cells at one noise list (``ops.image_grid_u8``).  ``psi`` / ``w_avg``: truncate every cell (StyleGAN2)."""
    if G.training:
        raise RuntimeError('latent.walk_sheet: G must be in eval mode')
    dev = next(G.parameters()).device
    with torch.no_grad(), preserved_rng(dev):
        noise = shared_noise(G, seed, dev)
        x = walk_latents(G, n_pairs, steps, seed, space)
        if psi is not None:
            need_w(G, 'walk_sheet(psi)')
            w = x if space == 'w' else G.get_latent(x)
            x, space = _styles(G, w, None, None, psi, w_avg, None), 'w'
        return ops.image_grid_u8(images_of(G, x, space, noise), nrow=steps, padding=padding)


def mix_sheet(G, n_a=4, n_b=6, cross=4, seed=0, psi=None, w_avg=None, padding=2):
    """The style-mixing sheet, uint8 on the device: (n_a + 1) rows of (n_b + 1) cells.  The top row shows the sources B, the
    left column the sources A, cell (i, j) the layers ``l < cross`` of A_i over the layers behind of B_j; the corner is black."""
    need_w(G, 'mix_sheet')
    if G.training:
        raise RuntimeError('latent.mix_sheet: G must be in eval mode')
    if n_a < 1 or n_b < 1:
        raise ValueError('latent.mix_sheet: at least one source on each side expected, got %r, %r' % (n_a, n_b))
    dev = next(G.parameters()).device
    with torch.no_grad(), preserved_rng(dev):
        noise = shared_noise(G, seed, dev)
        w = G.get_latent(fixed_latent(G, n_a + n_b, seed))
        wa, wb = w[:n_a], w[n_a:].contiguous()
        rows = [_styles(G, wb, None, None, psi, w_avg, None)]                                  # the sources B
        for i in range(n_a):
            a = wa[i:i + 1].expand(n_b, -1).contiguous()
            rows.append(_styles(G, a[:1], None, None, psi, w_avg, None))                       # source A_i
            rows.append(_styles(G, a, wb, cross, psi, w_avg, None))
        img = images_of(G, torch.cat(rows, 0), 'w', noise)
        corner = torch.zeros((1,) + tuple(img.shape[1:]), device=dev)
        return ops.image_grid_u8(torch.cat([corner, img], 0).contiguous(), nrow=n_b + 1, padding=padding)


# ---- the command lines ----
def _open_device(subject):
    if not torch.cuda.is_available():
        raise RuntimeError('%s on the MI355X HIP path only (no CPU fallback)' % subject)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    return dev


def ppl_parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: perceptual path length of G in the features of a frozen discriminator '
                                        '(no real data; one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (generator) model checkpoint')
    parser.add_argument('architecture', type=str, help="The generator's architecture")
    parser.add_argument('--encoder', required=True, type=str, help='discriminator checkpoint used as the frozen feature encoder')
    parser.add_argument('--encoder_arch', default=None, type=str, help="the encoder's architecture (default: the generator's)")
    parser.add_argument('--n', default=10000, type=int, help='number of pairs (default: 10000, at least %d)' % MIN_N)
    parser.add_argument('--space', default='z', type=str, choices=('z', 'w'), help="'z' (default) or 'w' (StyleGAN2 only)")
    parser.add_argument('--sampling', default='full', type=str, choices=('full', 'end'), help='t ~ U(0, 1) (default) or t = 0')
    parser.add_argument('--eps', default=DEFAULT_EPS, type=float, help='the step in t (default: %g)' % DEFAULT_EPS)
    parser.add_argument('--batch_size', default=64, type=int, help='pairs per forward (default: 64)')
    parser.add_argument('--seed', default=None, type=int, help="the tag of the output file and the latents' seed (default: drawn)")
    return parser.parse_args(argv)


def ppl_main(argv=None):
    """Prints one line and writes ``ppl_<space>_<seed>.json`` beside the generator; returns its path."""
    from . import features
    from .models.gan import get_architecture
    from .sample import image_size_of
    P = ppl_parse_args(argv)
    check_ppl_arguments(P.n, P.eps, P.sampling, P.batch_size)               # (refusals that need no device come first)
    check_space(P.architecture, P.space)
    dev = _open_device('Path length runs')
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    image_size = image_size_of(Path(P.model_path).parent)
    G = features.load_frozen(get_architecture(P.architecture, image_size)[0], P.model_path, dev)
    E = features.load_frozen(get_architecture(P.encoder_arch or P.architecture, image_size)[1], P.encoder, dev)
    out = ppl_of(G, E, P.n, seed, P.space, P.sampling, P.eps, P.batch_size)
    print('[PPL %s/%s of %d pairs at eps %g] [%.6f] [raw %.6f, kept %d]' % (P.space, P.sampling, out['n'], out['eps'], out['ppl'],
                                                                            out['ppl_raw'], out['kept']), flush=True)
    path = os.path.join(Path(P.model_path).parent, 'ppl_%s_%d.json' % (P.space, seed))
    with open(path, 'w') as f:
        json.dump(out, f)
    return path


def add_truncation_arguments(parser, cutoff=True):
    parser.add_argument('--truncation', default=None, type=float, metavar='PSI',
                        help='StyleGAN2 only: w_avg + PSI (w - w_avg) (default: no truncation)')
    parser.add_argument('--truncation_n', default=4096, type=int, help='with --truncation: draws behind w_avg (default: 4096)')
    if cutoff:
        parser.add_argument('--truncation_cutoff', default=None, type=int, metavar='L',
                            help='with --truncation: truncate the layers below L only (default: all)')


def check_truncation_arguments(P):
    """Refusals that need no device."""
    check_truncation(P.architecture, P.truncation)
    if P.truncation is None:
        return
    if not np.isfinite(P.truncation):
        raise ValueError('--truncation must be finite, got %r' % (P.truncation,))
    if P.truncation_n < 1:
        raise ValueError('--truncation_n must be at least 1, got %r' % (P.truncation_n,))
    if getattr(P, 'truncation_cutoff', None) is not None and P.truncation_cutoff < 0:
        raise ValueError('--truncation_cutoff must not be negative, got %r' % (P.truncation_cutoff,))


def walk_parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: interpolation and style-mixing sheets of G (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (generator) model checkpoint')
    parser.add_argument('architecture', type=str, help='Architecture')
    parser.add_argument('--pairs', default=8, type=int, help='rows of the interpolation sheet (default: 8)')
    parser.add_argument('--steps', default=9, type=int, help='columns of the interpolation sheet (default: 9)')
    parser.add_argument('--space', default='z', type=str, choices=('z', 'w'), help="walk in 'z' (default) or 'w' (StyleGAN2 only)")
    parser.add_argument('--mix', action='store_true', help='StyleGAN2 only: also write the style-mixing sheet mix_<seed>.png')
    parser.add_argument('--cross', default=None, type=int, metavar='L',
                        help='with --mix: the layers below L come from the row source (default: half of them)')
    add_truncation_arguments(parser, cutoff=False)
    parser.add_argument('--seed', default=None, type=int, help="the tag of the output files and the latents' seed (default: drawn)")
    parser.add_argument('--latents', default=None, type=str, metavar='NPZ',
                        help='StyleGAN2 only: walk between projected codes instead of draws -- the w (n, n_latent, D) of a '
                             'project_<seed>.npz (test_gan_project.py); row r of the sheet is the lerp in W+ from chosen code r to '
                             'chosen code r + 1 (--pairs, --space and --truncation do not apply)')
    parser.add_argument('--latent_rows', default=None, type=int, nargs='+', metavar='I',
                        help='with --latents: the codes to walk through, in order (default: all of them)')
    return parser.parse_args(argv)


def load_projected(path, rows=None):
    """The chosen codes of a ``project_<seed>.npz`` as float32 numpy [k, n_latent, D], k >= 2 (no device needed)."""
    with np.load(path) as f:
        if 'w' not in f.files:
            raise ValueError('%s holds no w (a project_<seed>.npz of test_gan_project.py expected)' % path)
        w = np.asarray(f['w'])
    if w.ndim != 3 or w.dtype != np.float32:
        raise ValueError('%s: w must be float32 (n, n_latent, D), got %s %s' % (path, w.dtype, w.shape))
    rows = list(range(len(w))) if rows is None else [int(r) for r in rows]
    if len(rows) < 2:
        raise ValueError('--latents walks between consecutive codes: at least two rows expected, got %r' % (rows,))
    for r in rows:
        if not 0 <= r < len(w):
            raise ValueError('--latent_rows %d: %s holds %d codes' % (r, path, len(w)))
    return np.ascontiguousarray(w[rows])


def walk_sheet_between(G, codes, steps=9, seed=0, padding=2):
    """The sheet of the lerps in W+ between consecutive ``codes`` [k, n_latent, D] (on the device): k - 1 rows, columns at equal
    steps of t, all cells at the one ``shared_noise`` list of ``seed``.  The first and last cell of a row are the codes' own
    bits (``ops.latent_pair``'s lerp at t = 0 and 1)."""
    need_w(G, 'walk_sheet_between')
    if G.training:
        raise RuntimeError('latent.walk_sheet_between: G must be in eval mode')
    if codes.dim() != 3 or codes.shape[0] < 2 or tuple(codes.shape[1:]) != (G.n_latent, G.style_dim) or steps < 2:
        raise ValueError('latent.walk_sheet_between: at least two codes of (%d, %d) and two steps expected' % (G.n_latent, G.style_dim))
    dev = next(G.parameters()).device
    k = codes.shape[0]
    flat = codes.to(dev).float().reshape(k, -1)
    with torch.no_grad(), preserved_rng(dev):
        noise = shared_noise(G, seed, dev)
        t = upload(torch.linspace(0.0, 1.0, steps, dtype=torch.float64).float().repeat(k - 1).view(-1, 1), dev).view(-1)
        x0, _x1 = ops.latent_pair(flat[:-1].repeat_interleave(steps, 0).contiguous(), flat[1:].repeat_interleave(steps, 0).contiguous(),
                                  t, 0.0, 0)
        return ops.image_grid_u8(images_of(G, x0.view(-1, G.n_latent, G.style_dim), 'w', noise), nrow=steps, padding=padding)


def walk_main(argv=None):
    """Writes ``walk_<seed>.png`` and, with ``--mix``, ``mix_<seed>.png`` beside the generator; returns their paths."""
    from .hostio import write_png
    from .sample import load_generator
    P = walk_parse_args(argv)
    if P.pairs < 1 or P.steps < 2:
        raise ValueError('--pairs must be at least 1 and --steps at least 2, got %r, %r' % (P.pairs, P.steps))
    check_space(P.architecture, P.space)
    check_truncation_arguments(P)
    if P.mix and P.architecture not in STYLE_ARCHITECTURES:
        raise ValueError('--mix exchanges per-layer styles: %s has no W (StyleGAN2 only)' % P.architecture)
    if P.cross is not None and not P.mix:
        raise ValueError('--cross does nothing without --mix')
    if P.cross is not None and P.cross < 0:
        raise ValueError('--cross must not be negative, got %r' % (P.cross,))
    codes = None
    if P.latent_rows is not None and P.latents is None:
        raise ValueError('--latent_rows does nothing without --latents FILE.npz')
    if P.latents is not None:
        if P.architecture not in STYLE_ARCHITECTURES:
            raise ValueError('--latents holds W+ codes: %s has no W (StyleGAN2 only)' % P.architecture)
        codes = load_projected(P.latents, P.latent_rows)
    dev = _open_device('Latent walks run')
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    G = load_generator(P.model_path, P.architecture, dev)
    if codes is not None:
        path = os.path.join(Path(P.model_path).parent, 'walk_%d.png' % seed)
        write_png(path, walk_sheet_between(G, torch.from_numpy(codes), P.steps, seed).cpu().numpy())
        print('Wrote %s' % path, flush=True)
        return [path]
    w_avg = None
    if P.truncation is not None:
        with preserved_rng(dev):
            torch.manual_seed(seed)
            w_avg = G.mean_latent(P.truncation_n)
    where = Path(P.model_path).parent
    paths = [os.path.join(where, 'walk_%d.png' % seed)]
    write_png(paths[0], walk_sheet(G, P.pairs, P.steps, seed, P.space, P.truncation, w_avg).cpu().numpy())
    if P.mix:
        cross = G.n_latent // 2 if P.cross is None else P.cross
        if cross > G.n_latent:
            raise ValueError('--cross %d: the generator has %d layers' % (cross, G.n_latent))
        paths.append(os.path.join(where, 'mix_%d.png' % seed))
        write_png(paths[1], mix_sheet(G, 4, 6, cross, seed, P.truncation, w_avg).cpu().numpy())
    print('Wrote %s' % ', '.join(paths), flush=True)
    return paths
