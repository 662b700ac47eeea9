"""StyleGAN2 projector: real images into W / W+ and the noise maps (Karras et al. 2020, appendix D), under a pixel-pyramid
loss.  An ADDITION of this project: the reference has no projector, and ``recover.py`` (section 20) stops
at SNDCGAN.  With this a trained ``gen_ema.pt`` gives the W-space code of a photograph, the latent-recovery memorisation check
(Webster et al. 2019) runs on the StyleGAN2 architectures, and ``test_gan_walk.py --latents`` walks between real images.

    python test_gan_project.py <run>/gen_ema.pt stylegan2 --data afhq.npz --n 100 --holdout --noise fixed
    python test_gan_project.py <run>/gen_ema.pt stylegan2 --synthetic --n 8 --steps 200 --space wplus --level_weights 1 1 1

Definition.  Targets x* (N, 3, H, W) in [0, 1]; x = G.synthesize(latents, noise) = 0.5 * skip + 0.5 on the differentiable path
(not clamped), G in eval mode and frozen.  Variables: w -- (N, D) broadcast to all layers (``space='w'``) or (N, n_latent, D)
(``'wplus'``) -- and, with ``noise='opt'``, one map (N, 1, R, R) per layer and image; with ``noise='fixed'`` the maps are one
``latent.shared_noise`` list, shared by all images and not optimised.  Start: w = w_avg of ``w_avg_n`` draws (the arithmetic of
``Generator.mean_latent``), w_std = sqrt(mean_n sum_d (w_n - w_avg)_d^2) in float64, maps standard normal.

    loss[n] = sum_l lam_l pix_l[n] + reg_weight sum_layers reg[n, layer]
    pix_l[n] = mean((pool_l(x[n]) - pool_l(x*[n]))^2),  pool_l the 2^l x 2^l mean          (ops.proj_image_end)
    reg = sum_j mean(m_j roll(m_j, 1, W))^2 + mean(m_j roll(m_j, 1, H))^2 over the pooled levels of a map   (ops.proj_noise_reg)

Step s of S, t = s / S: w_in = w + gauss * w_std * noise_factor * max(0, 1 - t / noise_ramp)^2; forward, loss ends, backward;
lr = lr0 * schedule(t); Adam (``optim.FusedAdam``) on w and the maps; every map normalised per image to zero mean and unit mean
square (``ops.proj_noise_normalize_``; a map of zero variance becomes zeros where the paper's code would divide by zero).

The report takes the images of the final (w, noise) on the forward-only eval path, which clamps: ``pix`` is their level-0 mean
squared error, ``pix_opt`` the objective's own level-0 term at the last step.

The defaults (1000 steps, lr 0.1, noise_factor 0.05, rampdown 0.25, rampup 0.05, noise_ramp 0.75, reg_weight 1e5) are the
paper's, tuned there against LPIPS; under a pixel loss they are PROVISIONAL: nobody has measured them.  LPIPS is out of scope (its
VGG weights are a download).  Eager only.
"""
import json
import math
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import features, hostio, latent, ops, recover
from . import project_nodes as PN
from .evaluate.gan import preserved_rng
from .hostio import THROTTLE
from .optim import FusedAdam

DEFAULT_STEPS, DEFAULT_LR, DEFAULT_BETAS = 1000, 0.1, (0.9, 0.999)
DEFAULT_NOISE_FACTOR, DEFAULT_RAMPDOWN, DEFAULT_RAMPUP, DEFAULT_NOISE_RAMP = 0.05, 0.25, 0.05, 0.75
DEFAULT_REG_WEIGHT, DEFAULT_W_AVG_N = 1e5, 10000
SPACES, NOISE_MODES = ('w', 'wplus'), ('opt', 'fixed')
NOTE = ('pix = mean squared error per image between the target and the clamped image of the projected (w, noise) (StyleGAN2 '
        'projector of Karras et al. 2020, appendix D, under a pixel-pyramid loss instead of LPIPS).  The defaults (steps, lr, '
        'noise_factor, ramps, reg_weight) are the paper\'s, tuned against LPIPS: under a pixel loss they are provisional and '
        'nobody has measured them.  With --noise opt the maps can encode the image, which shrinks the gap between training and '
        'held-out images: --noise fixed is the cleaner yardstick of memorisation.  ' + recover.NOTE)


def schedule(t, rampdown=DEFAULT_RAMPDOWN, rampup=DEFAULT_RAMPUP):
    """The paper's learning-rate factor at t = step / steps: 0.5 - 0.5 cos(pi min(1, (1 - t) / rampdown)), times
    min(1, t / rampup).  0 at t = 0.  Host floats only."""
    ramp = min(1.0, (1.0 - t) / rampdown)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return ramp * min(1.0, t / rampup)


def perturbation(t, w_std, noise_factor=DEFAULT_NOISE_FACTOR, noise_ramp=DEFAULT_NOISE_RAMP):
    """The standard deviation of the latent perturbation at t: w_std * noise_factor * max(0, 1 - t / noise_ramp)^2."""
    return w_std * noise_factor * max(0.0, 1.0 - t / noise_ramp) ** 2


def check_arguments(space, noise, level_weights, reg_weight, lr0, steps=1, n=1, batch=1, w_avg_n=1):
    """Refusals that need no device."""
    if space not in SPACES:
        raise ValueError('space must be one of %s, got %r' % (SPACES, space))
    if noise not in NOISE_MODES:
        raise ValueError('noise must be one of %s, got %r' % (NOISE_MODES, noise))
    lam = [float(v) for v in level_weights]
    if not 1 <= len(lam) <= ops.PROJ_MAX_LEVELS or not all(np.isfinite(v) and v >= 0 for v in lam) or not any(v > 0 for v in lam):
        raise ValueError('level_weights: 1 to %d finite non-negative weights, one of them positive, got %r'
                         % (ops.PROJ_MAX_LEVELS, list(level_weights)))
    if not (np.isfinite(reg_weight) and reg_weight >= 0) or not (np.isfinite(lr0) and lr0 >= 0):
        raise ValueError('reg_weight and lr must be finite and not negative, got %r, %r' % (reg_weight, lr0))
    if int(steps) < 1 or int(n) < 1 or int(batch) < 1 or int(w_avg_n) < 1:
        raise ValueError('steps, n, batch_size and w_avg_n must be at least 1')
    return lam


def w_statistics(G, n):
    """(w_avg (1, D) fp32 on the device, w_std as a host float) of ``n`` draws of the prior from the CUDA stream: the mean by
    ``Generator.mean_latent``'s arithmetic (float64 column sums, rounded once), w_std = sqrt(mean_n sum_d (w_n - w_avg)_d^2)
    in float64 about that rounded mean."""
    latent.need_w(G, 'w_statistics')
    z = torch.randn(int(n), G.style_dim, device=G.device)
    with torch.no_grad():
        w = G.get_latent(z).double()
        w_avg = w.mean(0, keepdim=True).float()
        w_std = float(((w - w_avg.double()) ** 2).sum(1).mean().sqrt())
    return w_avg, w_std


class Projector(object):
    """Adam on w (and the noise maps) towards given images for one batch size ``n``.  ``G``: an eval-mode StyleGAN2 generator on
    the device; it is not modified and none of its parameters receives a gradient."""

    def __init__(self, G, n, space='w', noise='opt', level_weights=(1.0,), reg_weight=DEFAULT_REG_WEIGHT, lr0=DEFAULT_LR,
                 betas=DEFAULT_BETAS, noise_factor=DEFAULT_NOISE_FACTOR, rampdown=DEFAULT_RAMPDOWN, rampup=DEFAULT_RAMPUP,
                 noise_ramp=DEFAULT_NOISE_RAMP, w_avg=None, w_std=0.0):
        latent.need_w(G, 'Projector')
        self.lam = check_arguments(space, noise, level_weights, reg_weight, lr0, n=n)
        if G.training:
            raise RuntimeError('Projector: G must be in eval mode')
        if G.device.type != 'cuda':
            raise RuntimeError('the projector runs on the MI355X HIP path only (no CPU fallback)')
        if G.size % (1 << (len(self.lam) - 1)):
            raise ValueError('%d pyramid levels need an image side divisible by %d' % (len(self.lam), 1 << (len(self.lam) - 1)))
        self.G, self.n, self.dev = G, int(n), G.device
        self.space, self.noise_mode = space, noise
        self.reg_weight, self.lr0, self.betas = float(reg_weight), float(lr0), (float(betas[0]), float(betas[1]))
        self.noise_factor, self.rampdown, self.rampup, self.noise_ramp = float(noise_factor), float(rampdown), float(rampup), float(noise_ramp)
        self.w_avg = None if w_avg is None else w_avg.detach().to(self.dev).reshape(1, G.style_dim)
        self.w_std = float(w_std)
        N, L, D, S = self.n, G.n_latent, G.style_dim, G.size
        wshape = (N, D) if space == 'w' else (N, L, D)
        self.w = torch.zeros(wshape, device=self.dev, requires_grad=True)
        self.gauss = torch.zeros(wshape, device=self.dev)
        self.sides = [2 ** ((i + 5) // 2) for i in range(G.num_layers)]
        self.maps = None
        self.target = torch.zeros(N, 3, S, S, device=self.dev)
        self.gx = torch.empty_like(self.target)
        self.pix_rows = torch.zeros(len(self.lam), N, device=self.dev)
        self.partial = torch.empty(ops.proj_image_end_partial_floats(len(self.lam), N, S, S), device=self.dev)
        self.reg_rows = torch.zeros(G.num_layers, N, device=self.dev)
        self.scratch = torch.empty(max(ops.proj_noise_reg_scratch_floats(N, R) for R in self.sides), device=self.dev)
        self.lam_t = hostio.upload(torch.tensor(self.lam).view(-1, 1), self.dev)
        self.opt = None
        self.has_targets = False

    # ---- per batch ----
    def set_targets(self, x):
        if tuple(x.shape) != tuple(self.target.shape):
            raise RuntimeError('Projector: targets of %s expected, got %s' % (tuple(self.target.shape), tuple(x.shape)))
        with torch.no_grad():
            self.target.copy_(x)
        self.has_targets = True

    def start(self, w0=None, noise=None):
        """New chain.  ``w0``: the start (default: w_avg in every row and layer).  ``noise``: the list of maps -- (N, 1, R, R)
        each with ``noise='opt'`` (default: drawn from the CUDA stream), (1, 1, R, R) each with ``'fixed'`` (required)."""
        with torch.no_grad():
            if w0 is None:
                if self.w_avg is None:
                    raise ValueError('Projector.start: no w0 and no w_avg')
                w0 = self.w_avg if self.space == 'w' else self.w_avg.unsqueeze(1)
            self.w.copy_(w0.expand_as(self.w))
            self.w.grad = None
            lead = self.n if self.noise_mode == 'opt' else 1
            if noise is None:
                if self.noise_mode == 'fixed':
                    raise ValueError("Projector.start: noise='fixed' takes its list from the caller (latent.shared_noise)")
                noise = [torch.randn(lead, 1, R, R, device=self.dev) for R in self.sides]
            if [tuple(m.shape) for m in noise] != [(lead, 1, R, R) for R in self.sides]:
                raise ValueError('Projector.start: noise maps of %s expected' % [(lead, 1, R, R) for R in self.sides])
            self.maps = [m.detach().clone().contiguous().requires_grad_(self.noise_mode == 'opt') for m in noise]
            self.reg_rows.zero_()
        params = [self.w] + (self.maps if self.noise_mode == 'opt' else [])
        self.opt = FusedAdam(params, lr=self.lr0, betas=self.betas)

    def latents(self, w=None):
        """(N, n_latent, D) of the current (or a given) w, in both spaces."""
        w = self.w.detach() if w is None else w
        return w.unsqueeze(1).repeat(1, self.G.n_latent, 1) if self.space == 'w' else w

    # ---- one step ----
    def step(self, s, steps, gauss=None):
        """Step ``s`` of ``steps``.  ``gauss``: the step's Gaussian draw in w's shape (default: drawn by torch into the static
        tensor)."""
        if not self.has_targets or self.opt is None:
            raise RuntimeError('set_targets() and start() first')
        t = float(s) / float(steps)
        sigma = perturbation(t, self.w_std, self.noise_factor, self.noise_ramp)
        if gauss is None:
            self.gauss.normal_()
        else:
            self.gauss.copy_(gauss)
        opt_noise = self.noise_mode == 'opt'
        w_in = self.w + self.gauss * sigma
        x = self.G.synthesize(self.latents(w_in), self.maps, noise_grad=opt_noise)
        PN.image_end(x, self.target, self.lam, pix=self.pix_rows, gx=self.gx, partial=self.partial)
        self.w.grad = None
        for m in self.maps:
            m.grad = None
        x.backward(self.gx)
        if opt_noise:
            for i, m in enumerate(self.maps):
                PN.noise_reg_(m, m.grad, self.reg_weight, reg=self.reg_rows[i], scratch=self.scratch[:ops.proj_noise_reg_scratch_floats(self.n, self.sides[i])])
        self.opt.param_groups[0]['lr'] = self.lr0 * schedule(t, self.rampdown, self.rampup)
        self.opt.step()
        if opt_noise:
            for m in self.maps:
                ops.proj_noise_normalize_(m.data)

    def loss_rows(self):
        """(loss, pix rows (L, N), reg (N,)) of the last step's forward (new tensors)."""
        reg = self.reg_rows.sum(0)
        return (self.lam_t * self.pix_rows).sum(0) + self.reg_weight * reg, self.pix_rows.clone(), reg

    def images(self):
        """The images of the current (w, noise) on the forward-only eval path, clamped to [0, 1] (a new tensor)."""
        with torch.no_grad():
            return self.G(self.latents(), input_is_latent=True, noise=[m.detach() for m in self.maps]).contiguous().float()

    def project(self, x, steps, w0=None, noise=None):
        """``steps`` steps towards ``x`` -> dict of new tensors: ``w`` (N, n_latent, D), ``pix`` (the clamped final images'
        level-0 error), ``pix_opt`` (the objective's level-0 term at the last step), ``reg``, ``images``, ``noise``."""
        self.set_targets(x)
        self.start(w0, noise)
        for s in range(int(steps)):
            THROTTLE.begin()                      # the host stays at most one step ahead (hostio.py)
            self.step(s, steps)
            THROTTLE.end()
        _loss, pix_rows, reg = self.loss_rows()
        img = self.images()
        pix = ops.proj_image_end(img, self.target, (1.0,))[0][0]
        return {'w': self.latents().clone(), 'pix': pix, 'pix_opt': pix_rows[0].clone(), 'reg': reg, 'images': img,
                'noise': [m.detach().clone() for m in self.maps]}


def project_images(G, images_u8, idx, space='w', noise='opt', level_weights=(1.0,), reg_weight=DEFAULT_REG_WEIGHT, lr0=DEFAULT_LR,
                   steps=DEFAULT_STEPS, batch_size=8, w_avg_n=DEFAULT_W_AVG_N, seed=0, save_noise=False, **kw):
    """Projects ``images_u8[idx]`` (device-resident uint8 [n, H, W, 3]) in batches of ``batch_size``; the last batch repeats its
    last image.  Everything random (the draws behind w_avg, the shared or initial noise maps, the perturbations) comes from the
    CUDA stream seeded with ``seed``; the global streams are left as they were.  -> dict of CPU tensors ``w``
    (n, n_latent, D), ``pix``, ``pix_opt``, ``reg`` (n,), ``images`` (n, 3, H, W) and, with ``save_noise``, ``noise`` (a list)."""
    features.check_u8(images_u8, 'target', 'projector')
    idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
    n = idx.numel()
    if n < 1 or int(idx.min()) < 0 or int(idx.max()) >= images_u8.shape[0]:
        raise ValueError('projector: indices outside the %d images, or none' % images_u8.shape[0])
    check_arguments(space, noise, level_weights, reg_weight, lr0, steps, n, batch_size, w_avg_n)
    dev = images_u8.device
    _, H, W, _ = images_u8.shape
    B = min(int(batch_size), n)
    out = {'w': torch.empty(n, G.n_latent, G.style_dim), 'pix': torch.empty(n), 'pix_opt': torch.empty(n), 'reg': torch.empty(n),
           'images': torch.empty(n, 3, H, W)}
    with preserved_rng(dev):
        torch.cuda.manual_seed(int(seed))
        w_avg, w_std = w_statistics(G, w_avg_n)
        shared = latent.shared_noise(G, seed, dev) if noise == 'fixed' else None
        proj = Projector(G, B, space, noise, level_weights, reg_weight, lr0, w_avg=w_avg, w_std=w_std, **kw)
        if save_noise:
            lead = 1 if noise == 'fixed' else n
            out['noise'] = [torch.empty(lead, 1, R, R) for R in proj.sides]
        x = torch.empty(B, 3, H, W, device=dev)
        for i in range(0, n, B):
            keep = min(B, n - i)
            rows = torch.cat([idx[i:i + keep], idx[i + keep - 1:i + keep].expand(B - keep)])
            features.to_float_nchw(images_u8, rows.to(dev), x)
            res = proj.project(x, steps, noise=shared)
            for k in ('w', 'pix', 'pix_opt', 'reg', 'images'):
                out[k][i:i + keep].copy_(res[k][:keep])
            if save_noise:
                for dst, src in zip(out['noise'], res['noise']):
                    if noise == 'fixed':
                        dst.copy_(src)
                    else:
                        dst[i:i + keep].copy_(src[:keep])
    return out


# ---- command line ----
def parse_args(argv=None):
    prov = ' (the paper\'s value, tuned against LPIPS: provisional under a pixel loss)'
    parser = ArgumentParser(description='Testing script: StyleGAN2 projector -- Adam on w (and the noise maps) towards given images '
                                        'under a pixel-pyramid loss, and the error on training against held-out images '
                                        '(one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (generator) checkpoint; the *.gin next to it names the dataset')
    parser.add_argument('architecture', type=str, help='Architecture (one with a mapping network: StyleGAN2)')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--data', default=None, type=str, help='npz with x_train (and x_test for --holdout) uint8 [n, H, W, 3]')
    src.add_argument('--synthetic', action='store_true', help='seeded synthetic set instead of a dataset')
    parser.add_argument('--n', default=100, type=int, help='images to project per split: the first N (default: 100)')
    parser.add_argument('--holdout', action='store_true', help='also project the first N images of x_test and compare')
    parser.add_argument('--space', default='w', type=str, choices=SPACES, help="one w for all layers (default) or one per layer ('wplus')")
    parser.add_argument('--noise', default='opt', type=str, choices=NOISE_MODES,
                        help="optimise one noise map per layer and image (default) or keep one shared list fixed ('fixed': the "
                             'cleaner yardstick of memorisation, the maps cannot encode the image)')
    parser.add_argument('--steps', default=DEFAULT_STEPS, type=int, help='steps per image (default: %d%s)' % (DEFAULT_STEPS, prov))
    parser.add_argument('--lr', default=DEFAULT_LR, type=float, help='peak learning rate (default: %g%s)' % (DEFAULT_LR, prov))
    parser.add_argument('--level_weights', default=[1.0], type=float, nargs='+',
                        help='weights of the pyramid levels 0, 1, ... (at most %d; default: 1 = plain MSE)' % ops.PROJ_MAX_LEVELS)
    parser.add_argument('--reg_weight', default=DEFAULT_REG_WEIGHT, type=float,
                        help='weight of the noise regulariser (default: %g%s)' % (DEFAULT_REG_WEIGHT, prov))
    parser.add_argument('--w_avg_n', default=DEFAULT_W_AVG_N, type=int, help='draws behind w_avg and w_std (default: %d)' % DEFAULT_W_AVG_N)
    parser.add_argument('--batch_size', default=8, type=int, help='Batch size (default: 8)')
    parser.add_argument('--seed', default=None, type=int, help='seed of every draw and file-name tag (default: drawn)')
    parser.add_argument('--save_noise', action='store_true', help='also write the noise maps into the npz')
    parser.add_argument('--rows', default=16, type=int, help='best and worst pairs shown in the figure (default: 16; 0: no png)')
    return parser.parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    # every refusal of the arguments comes before any CUDA call
    check_arguments(P.space, P.noise, P.level_weights, P.reg_weight, P.lr, P.steps, P.n, P.batch_size, P.w_avg_n)
    if P.rows < 0:
        raise ValueError('--rows must not be negative')
    from .models.gan import get_architecture
    from .sample import image_size_of
    image_size = tuple(image_size_of(Path(P.model_path).parent))
    with preserved_rng():
        G0 = get_architecture(P.architecture, image_size)[0]
    latent.need_w(G0, 'project')
    if image_size[0] % (1 << (len(P.level_weights) - 1)):
        raise ValueError('%d pyramid levels need an image side divisible by %d' % (len(P.level_weights), 1 << (len(P.level_weights) - 1)))
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.synthetic:
        from .lineval import synthetic_set
        data = synthetic_set(seed, 10, P.n, P.n, size=image_size[0])
        sets = {'train': data['x_train'], 'test': data['x_test']}
    else:
        with np.load(P.data) as f:
            have = set(f.files)
        for key in ['x_train'] + (['x_test'] if P.holdout else []):
            if key not in have:
                raise ValueError('%s holds no %s' % (P.data, key))
        sets = {'train': features.load_images(P.data, 'x_train')}
        if P.holdout:
            sets['test'] = features.load_images(P.data, 'x_test')
    splits = ['train'] + (['test'] if P.holdout else [])
    for s in splits:
        if P.n > len(sets[s]):
            raise ValueError('--n %d beyond the %d images of x_%s' % (P.n, len(sets[s]), s))
        if tuple(sets[s].shape[1:]) != image_size:
            raise ValueError('x_%s holds %s images, the run paints %s' % (s, tuple(sets[s].shape[1:]), image_size))
    if P.rows and 2 * P.rows > P.n * len(splits):
        raise ValueError('--rows %d: the figure shows 2 x rows of the %d projected images' % (P.rows, P.n * len(splits)))
    if not torch.cuda.is_available():
        raise RuntimeError('the projector runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    G = features.load_frozen(G0, P.model_path, dev)

    res, targets = {}, {}
    for j, s in enumerate(splits):
        u8 = torch.from_numpy(np.ascontiguousarray(sets[s][:P.n])).to(dev)
        res[s] = project_images(G, u8, torch.arange(P.n), space=P.space, noise=P.noise, level_weights=P.level_weights,
                                reg_weight=P.reg_weight, lr0=P.lr, steps=P.steps, batch_size=P.batch_size, w_avg_n=P.w_avg_n,
                                seed=seed, save_noise=P.save_noise)
        targets[s] = u8
    out = {'model_path': P.model_path, 'architecture': P.architecture, 'data': P.data, 'synthetic': bool(P.synthetic), 'n': P.n,
           'holdout': bool(P.holdout), 'space': P.space, 'noise': P.noise, 'steps': P.steps, 'lr': P.lr, 'betas': list(DEFAULT_BETAS),
           'level_weights': [float(v) for v in P.level_weights], 'reg_weight': P.reg_weight, 'w_avg_n': P.w_avg_n,
           'noise_factor': DEFAULT_NOISE_FACTOR, 'rampdown': DEFAULT_RAMPDOWN, 'rampup': DEFAULT_RAMPUP, 'noise_ramp': DEFAULT_NOISE_RAMP,
           'batch_size': P.batch_size, 'seed': seed, 'save_noise': bool(P.save_noise), 'rows': P.rows, 'image_size': list(image_size)}
    out.update(recover.statistics(res['train']['pix'].numpy(), res['test']['pix'].numpy() if P.holdout else None))
    out['note'] = NOTE
    text = 'projection into %s, noise %s (%d steps, lr %g): [train median pix %.6f, PSNR %.2f dB]' % (
        P.space, P.noise, P.steps, P.lr, out['train']['median'], out['train']['psnr_median'])
    if P.holdout:
        text += ' [test median pix %.6f] [auc %.4f, z %.2f, median gap %.4f]' % (
            out['test']['median'], out['auc'], out['z_score'], out['median_gap'])
    print(text, flush=True)

    where = str(Path(P.model_path).parent)
    with open(os.path.join(where, 'project_%d.json' % seed), 'w') as f:
        json.dump(out, f)
    cat = lambda k: np.concatenate([res[s][k].numpy() for s in splits])         # noqa: E731
    arrays = dict(w=cat('w'), pix=cat('pix'), pix_opt=cat('pix_opt'), reg=cat('reg'),
                  index=np.concatenate([np.arange(P.n, dtype=np.int64) for _ in splits]),
                  split=np.concatenate([np.full(P.n, j, np.int64) for j, _ in enumerate(splits)]))
    if P.save_noise:
        for i in range(len(res['train']['noise'])):
            if P.noise == 'fixed':
                arrays['noise_%d' % i] = res['train']['noise'][i].numpy()
            else:
                arrays['noise_%d' % i] = np.concatenate([res[s]['noise'][i].numpy() for s in splits])
    recover.write_npz(os.path.join(where, 'project_%d.npz' % seed), **arrays)
    if P.rows:
        tgt = torch.cat([features.to_float_nchw(targets[s], torch.arange(P.n, device=dev), torch.empty(P.n, 3, *image_size[:2], device=dev))
                         for s in splits])
        recon = torch.cat([res[s]['images'] for s in splits]).to(dev)
        order = np.argsort(cat('pix').astype(np.float64), kind='stable')
        chosen = np.concatenate([order[:P.rows], order[-P.rows:]])
        hostio.write_png(os.path.join(where, 'project_%d.png' % seed), recover.pair_grid(tgt, recon, chosen).cpu().numpy())
    return os.path.join(where, 'project_%d.json' % seed)


if __name__ == '__main__':
    main()
