"""Latent recovery: project given images onto a generator by optimising the latent, on the cDDLS sampler's launch chain.
An ADDITION of this project: the reference has no counterpart.  Every other diagnostic here looks at
samples and asks how good they are; this one takes an image and asks whether G can produce it -- the "projector" of GAN
code bases, and the generator-side half of a memorisation check (Webster et al., "Detecting Overfitting of Deep Generative
Networks via Latent Recovery", CVPR 2019): a generator that memorised its training set recovers training images with lower
error than held-out ones.

    python test_gan_recover.py <run>/gen.pt sndcgan --data cifar10.npz --n 1000 --holdout --graph
    python test_gan_recover.py <run>/gen.pt sndcgan --synthetic --n 64 --steps 50 --lambda_feat 1 --dis <run>/dis.pt

Definition.  Targets x* (N, 3, H, W) in [0, 1]; x = G(z) with G in eval mode (the sampler's G chain; no z2, no eps);
P = 3 H W; phi = the D half's feature tensor (sndcgan: the NHWC-flat post-LeakyReLU map, F = 512 hb wb; snresnet18: the 512
pooled features):

    pix[n]  = (1 / P) sum (x[n] - x*[n])^2
    feat[n] = (1 / F) sum (phi(x)[n] - phi(x*)[n])^2
    loss[n] = pix[n] + lambda_feat * feat[n]

minimised by Adam on z with a clamp to SNDCGAN's latent support, t = step + 1 read from device memory:

    m <- b1 m + (1 - b1) g,   v <- b2 v + (1 - b2) g^2,
    z <- clamp(z - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + adam_eps), -1, 1)

One step is a fixed chain of launches on static buffers that ``--graph`` captures at its second use and replays:

    G forward -> [D trunk forward -> loss form (residual rows) -> seed -> D trunk backward] -> image end (recovery form)
    -> G backward -> latent update (Adam form; advances the device-resident step counter)

20 launches with pixels only (the default, lambda_feat = 0: no D half is built or run).  The three element-wise ends are
forms of the sampler's kernels (csrc/cddls.hip); the logit head of D is neither prepared nor run.

The defaults (lr 0.05, betas (0.9, 0.999), adam_eps 1e-8, 500 steps) are PROVISIONAL: nobody has measured which settings
recover best on trained networks.  The statistics depend on them and are comparable only at equal settings.
"""
import json
import math
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import features, hostio, ops
from .captured import EagerFirst, capture
from .cddls import IMPLEMENTED, _d_half, _GHalf
from .hostio import THROTTLE

DEFAULT_LR, DEFAULT_BETAS, DEFAULT_ADAM_EPS, DEFAULT_STEPS = 0.05, (0.9, 0.999), 1e-8, 500
NOTE = ('pix = mean squared error per image between the target and G(z) after Adam on z (latent recovery, Webster et al. 2019).  '
        'auc = P(pix_train < pix_test) + P(equal) / 2 (Mann-Whitney U / (n m)); z_score = its normal approximation with the tie '
        'correction; median_gap = (median_test - median_train) / median_test.  auc 0.5, z_score 0 and median_gap 0 mean no sign '
        'of memorisation; larger values mean training images are recovered better than held-out ones.  All numbers depend on '
        'steps, lr, restarts and lambda_feat and are comparable only at equal settings; the defaults are provisional.')


class LatentRecovery(_GHalf):
    """Adam on z towards given images for one batch size, on static buffers.  Shares the sampler's G half (cddls._GHalf:
    ``_prep_g``, ``_g_forward``, ``_g_backward``) and, for ``lambda_feat > 0``, the trunk of the matching D half reading
    ``gout`` directly (no compose launch, no logit head).  ``G`` / ``D``: eval-mode modules on the device."""

    def __init__(self, G, n, D=None, lambda_feat=0.0, lr=DEFAULT_LR, betas=DEFAULT_BETAS, adam_eps=DEFAULT_ADAM_EPS,
                 graph=False):
        from .models.gan.sndcgan import G_SNDCGAN
        lambda_feat = float(lambda_feat)
        if lambda_feat < 0 or lr < 0 or adam_eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or int(n) < 1:
            raise ValueError('latent recovery: n >= 1, lambda_feat, lr, adam_eps >= 0 and betas in [0, 1) expected')
        if lambda_feat > 0 and D is None:
            raise ValueError('latent recovery: lambda_feat > 0 needs D (the feature loss is read from its trunk)')
        self.half = _d_half(D) if lambda_feat > 0 else None
        if not isinstance(G, G_SNDCGAN) or (lambda_feat > 0 and self.half is None):
            raise NotImplementedError('latent recovery is implemented for: %s' % ', '.join(IMPLEMENTED))
        if G.training or (self.half is not None and D.training):
            raise RuntimeError('latent recovery runs on networks in eval mode')
        self.hb, self.wb = G.s_hb, G.s_wb
        if self.half is not None:
            from .cddls import _DHalfSNResNet18
            if self.half is _DHalfSNResNet18 and (8 * self.hb, 8 * self.wb) != (32, 32):
                raise NotImplementedError('latent recovery with D_SNResNet18: 32x32 images (its 4x4 average pool)')
            if self.half is not _DHalfSNResNet18 and (D.s_hb, D.s_wb) != (self.hb, self.wb):
                raise RuntimeError('G paints %dx%d images, D reads %dx%d' % (8 * self.hb, 8 * self.wb, 8 * D.s_hb, 8 * D.s_wb))
        dev = next(G.parameters()).device
        if dev.type != 'cuda' or (self.half is not None and next(D.parameters()).device != dev):
            raise RuntimeError('latent recovery runs on the MI355X HIP path only (no CPU fallback)')
        self.G, self.D, self.n, self.dev = G, (D if self.half is not None else None), int(n), dev
        self.lambda_feat, self.lr, self.betas, self.adam_eps = lambda_feat, float(lr), (float(betas[0]), float(betas[1])), float(adam_eps)
        self.use_graph = bool(graph)
        self.graph, self.first, self._scratch = None, EagerFirst(), {}
        self.feat = 512 * self.hb * self.wb                     # G's first map, flat
        self.P = 3 * 64 * self.hb * self.wb
        with torch.no_grad():
            if self.half is not None:
                self.half.prep(self, head=False)
            self._prep_g()
            self._alloc()

    def _alloc(self):
        N, dev, hb, wb = self.n, self.dev, self.hb, self.wb
        H, W = 8 * hb, 8 * wb

        def buf(*shape):
            return torch.zeros(shape, device=dev, dtype=torch.float32)
        self.z, self.g_z, self.m, self.v = (buf(N, self.G.nz) for _ in range(4))
        self.gout, self.target, self.g_lin = (buf(N, 3, H, W) for _ in range(3))
        self.h0, self.g_h0 = buf(N, self.feat), buf(N, self.feat)
        gshapes = [(N, hb, wb, 512), (N, 2 * hb, 2 * wb, 256), (N, 4 * hb, 4 * wb, 128), (N, H, W, 64)]
        self.g_acts = [buf(*s) for s in gshapes]
        self.g_grads = [buf(*s) for s in gshapes]
        self.loss3 = buf(3, N)                                  # rows: pix, feat, loss
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)      # {step, arrival counter of the latent update}
        self.g_x = None
        if self.half is not None:
            self.x = self.gout                                  # the D half reads G's output itself
            self.g_x = buf(N, 3, H, W)
            self.half.alloc(self, buf)
            self.F = self.d_feats.numel() // N
            self.phi_target, self.resid = buf(N, self.F), buf(N, self.F)
            self.zero_row = buf(self.F)
        self.has_targets = False

    # ---- per batch ----
    def set_targets(self, x):
        """Stores x* (N, 3, H, W) float32 in [0, 1]; with a D half, phi* = its trunk on x* through the step's own launches,
        so a z whose G(z) equals x* bitwise has residual exactly 0."""
        if tuple(x.shape) != tuple(self.target.shape):
            raise RuntimeError('latent recovery: targets of %s expected, got %s' % (tuple(self.target.shape), tuple(x.shape)))
        with torch.no_grad():
            self.target.copy_(x)
            if self.half is not None:
                self.x = self.target
                self.half.forward_trunk(self)
                self.phi_target.copy_(self.d_feats.reshape(self.n, self.F))
                self.x = self.gout
        self.has_targets = True

    def start(self, z0):
        """New chain: ``z`` = z0, zero moments, step counter 0."""
        with torch.no_grad():
            self.z.copy_(z0)
            self.m.zero_()
            self.v.zero_()
            self.state.zero_()

    # ---- one step ----
    def _loss(self):
        if self.half is None:
            ops.cddls_recover_loss(self.gout, self.target, 0.0, out=self.loss3)
        else:
            ops.cddls_recover_loss(self.gout, self.target, self.lambda_feat, phi=self.d_feats, phi_target=self.phi_target,
                                   resid=self.resid, out=self.loss3)

    def _body(self):
        with torch.no_grad():
            self._g_forward()
            if self.half is not None:
                self.half.forward_trunk(self)
                self._loss()
                self.half.backward_trunk(self, self.half.seed_rows(self, self.resid, self.zero_row))
            ops.cddls_recover_image_end(self.gout, self.target, self.g_lin, self.P, gx=self.g_x)
            self._g_backward()
            ops.cddls_recover_update(self.z, self.g_z, self.m, self.v, self.lr, self.betas, self.adam_eps, self.state)

    def step(self):
        """One Adam step on z."""
        if not self.has_targets:
            raise RuntimeError('set_targets() first')
        if not self.use_graph or not self.first.may_capture():
            return self._body()
        if self.graph is None:
            self.graph, _ = capture(self._body, tuple(m for m in (self.G, self.D) if m is not None), self._scratch)
        self.graph.replay()

    def losses(self):
        """(pix, feat, loss) of the current z, each (N,) (new tensors): G forward, the D trunk when there is a feature
        term, the loss form."""
        if not self.has_targets:
            raise RuntimeError('set_targets() first')
        with torch.no_grad():
            self._g_forward()
            if self.half is not None:
                self.half.forward_trunk(self)
            self._loss()
            return tuple(self.loss3.clone())

    def images(self):
        """G(z) of the current state, NCHW in [0, 1] (a new tensor)."""
        with torch.no_grad():
            self._g_forward()
            return self.gout.clone()

    def recover(self, x, z0, n_steps):
        """``n_steps`` Adam steps from ``z0`` towards ``x`` -> (z, pix, feat) of the final state (new tensors)."""
        self.set_targets(x)
        self.start(z0)
        for _ in range(n_steps):
            THROTTLE.begin()                      # the host stays at most one step ahead (hostio.py)
            self.step()
            THROTTLE.end()
        pix, feat, _ = self.losses()
        return self.z.clone(), pix, feat

    def linear_region(self):
        """Test hook, the sampler's: the ReLU / LeakyReLU regions the last forward ran on (no logit head: no 'hidden')."""
        return {'g': self._g_regions(), 'd': self.half.regions(self) if self.half is not None else []}


def recover_images(G, D, images_u8, idx, lambda_feat=0.0, lr=DEFAULT_LR, betas=DEFAULT_BETAS, adam_eps=DEFAULT_ADAM_EPS,
                   steps=DEFAULT_STEPS, batch_size=500, restarts=1, seed=0, graph=False):
    """Recovers ``images_u8[idx]`` (device-resident uint8 [n, H, W, 3]; ``idx``: int64 indices) in batches of ``batch_size``.
    z0 is drawn by ``uniform_(-1, 1)`` from a torch CPU generator seeded with ``seed`` (as ``sample_latent`` draws), one
    full batch per chain, batches in order, restarts innermost.  With ``restarts > 1`` the chains run one after another and
    each image keeps the state of its lowest ``loss`` (the first one on a tie).  -> dict of CPU tensors ``z`` (n, nz),
    ``pix``, ``feat``, ``loss`` (n,) and the reconstructions ``images`` (n, 3, H, W) float32."""
    features.check_u8(images_u8, 'target', 'latent recovery')
    idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
    n = idx.numel()
    if n < 1 or int(idx.min()) < 0 or int(idx.max()) >= images_u8.shape[0]:
        raise ValueError('latent recovery: indices outside the %d images, or none' % images_u8.shape[0])
    if steps < 1 or restarts < 1 or batch_size < 1:
        raise ValueError('latent recovery: steps, restarts and batch_size must be at least 1')
    dev = images_u8.device
    _, H, W, _ = images_u8.shape
    B = min(int(batch_size), n)
    rec = LatentRecovery(G, B, D=D, lambda_feat=lambda_feat, lr=lr, betas=betas, adam_eps=adam_eps, graph=graph)
    gen = torch.Generator().manual_seed(int(seed))
    x = torch.empty(B, 3, H, W, device=dev)
    out = {'z': torch.empty(n, G.nz), 'pix': torch.empty(n), 'feat': torch.empty(n), 'loss': torch.empty(n),
           'images': torch.empty(n, 3, H, W)}
    for i in range(0, n, B):
        keep = min(B, n - i)
        rows = torch.cat([idx[i:i + keep], idx[i + keep - 1:i + keep].expand(B - keep)])       # the last batch repeats its last image
        features.to_float_nchw(images_u8, rows.to(dev), x)
        best = None
        for _ in range(restarts):
            z0 = torch.empty(B, G.nz).uniform_(-1, 1, generator=gen)
            z, pix, feat = rec.recover(x, hostio.upload(z0, dev), steps)
            cur = {'z': z, 'pix': pix, 'feat': feat, 'loss': rec.loss3[2].clone(), 'images': rec.gout.clone()}
            if best is None:
                best = cur
            else:
                better = cur['loss'] < best['loss']
                for k in best:
                    best[k] = torch.where(better.view((-1,) + (1,) * (best[k].dim() - 1)), cur[k], best[k])
        for k in out:
            out[k][i:i + keep].copy_(best[k][:keep])
    return out


# ---- statistics (host, float64) ----
def split_stats(pix):
    """mean, median, p10, p90 of the per-image errors and the PSNR of the median (images in [0, 1])."""
    p = np.asarray(pix, np.float64).reshape(-1)
    med = float(np.median(p))
    return {'n': int(p.size), 'mean': float(p.mean()), 'median': med, 'p10': float(np.percentile(p, 10)),
            'p90': float(np.percentile(p, 90)), 'psnr_median': (10.0 * math.log10(1.0 / med) if med > 0 else float('inf'))}


def auc_train_below_test(train, test):
    """(auc, z_score): auc = P(train < test) + P(equal) / 2 = U / (n m) by midranks; z_score = (U - n m / 2) / sigma with
    sigma^2 = (n m / 12) ((n + m + 1) - sum(t^3 - t) / ((n + m)(n + m - 1))) over the tie groups (0 when sigma is 0)."""
    a, b = np.asarray(train, np.float64).reshape(-1), np.asarray(test, np.float64).reshape(-1)
    n, m = a.size, b.size
    if n < 1 or m < 1:
        raise ValueError('latent recovery: both splits need at least one image')
    both = np.concatenate([a, b])
    vals, inv, counts = np.unique(both, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts).astype(np.float64)
    midrank = ends - (counts - 1) / 2.0                       # 1-based average rank of every tie group
    r_test = midrank[inv[n:]].sum()
    u = r_test - m * (m + 1) / 2.0                            # pairs with test above train, ties half
    N = n + m
    ties = float(((counts.astype(np.float64) ** 3) - counts).sum())
    var = n * m / 12.0 * ((N + 1) - (ties / (N * (N - 1)) if N > 1 else 0.0))
    z = (u - n * m / 2.0) / math.sqrt(var) if var > 0 else 0.0
    return float(u / (n * m)), float(z)


def statistics(pix_train, pix_test=None):
    out = {'train': split_stats(pix_train), 'note': NOTE}
    if pix_test is not None:
        out['test'] = split_stats(pix_test)
        out['auc'], out['z_score'] = auc_train_below_test(pix_train, pix_test)
        mt = out['test']['median']
        out['median_gap'] = (mt - out['train']['median']) / mt if mt > 0 else 0.0
    return out


# ---- the figure ----
def pair_grid(targets, recon, order):
    """uint8 canvas: one cell pair per entry of ``order`` -- the target, then its reconstruction -- eight pairs per line
    (``ops.image_grid_u8``).  ``targets`` / ``recon``: float NCHW on the device."""
    order = torch.as_tensor(order, dtype=torch.int64, device=targets.device)
    cells = torch.stack([targets.index_select(0, order), recon.index_select(0, order)], 1)
    return ops.image_grid_u8(cells.reshape((-1,) + tuple(targets.shape[1:])).contiguous(), nrow=16)


def figure_shape(rows, H, W, padding=2):
    """Shape of the figure of ``rows`` best and ``rows`` worst pairs."""
    lines = -(-(4 * rows) // 16)
    cols = min(4 * rows, 16)
    return (lines * (H + padding) + padding, cols * (W + padding) + padding, 3)


def write_npz(path, **arrays):
    """``np.savez`` with a fixed time stamp on every member: two runs with one seed write the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


# ---- command line ----
def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: latent recovery -- project images onto G by Adam on z and compare the '
                                        'error on training and held-out images (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (generator) checkpoint; the *.gin next to it names the dataset')
    parser.add_argument('architecture', type=str, help='Architecture')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--data', default=None, type=str, help='npz with x_train (and x_test for --holdout) uint8 [n, H, W, 3]')
    src.add_argument('--synthetic', action='store_true', help='seeded synthetic set instead of a dataset')
    parser.add_argument('--n', default=1000, type=int, help='images to recover per split: the first N (default: 1000)')
    parser.add_argument('--holdout', action='store_true', help='also recover the first N images of x_test and compare')
    parser.add_argument('--steps', default=DEFAULT_STEPS, type=int, help='Adam steps per chain (default: %d, provisional)' % DEFAULT_STEPS)
    parser.add_argument('--lr', default=DEFAULT_LR, type=float, help='learning rate (default: %g, provisional)' % DEFAULT_LR)
    parser.add_argument('--betas', default=DEFAULT_BETAS, type=float, nargs=2)
    parser.add_argument('--adam_eps', default=DEFAULT_ADAM_EPS, type=float)
    parser.add_argument('--restarts', default=1, type=int, help='chains per image, the best loss is kept (default: 1)')
    parser.add_argument('--lambda_feat', default=0.0, type=float, help='weight of the feature loss in the trunk of --dis (default: 0)')
    parser.add_argument('--dis', default=None, type=str, help='discriminator checkpoint of the feature loss')
    parser.add_argument('--batch_size', default=500, type=int, help='Batch size (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help='seed of the initial latents and file-name tag (default: drawn)')
    parser.add_argument('--graph', action='store_true', help='replay the step from a captured hipGraph')
    parser.add_argument('--rows', default=16, type=int, help='best and worst pairs shown in the figure (default: 16; 0: no png)')
    return parser.parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    # every refusal of the arguments comes before any CUDA call
    if P.architecture not in IMPLEMENTED:
        raise NotImplementedError("latent recovery of architecture '%s' (implemented: %s; the clamp of z to [-1, 1] belongs "
                                  "to SNDCGAN's uniform latent)" % (P.architecture, ', '.join(IMPLEMENTED)))
    if P.lambda_feat < 0 or (P.lambda_feat > 0 and not P.dis):
        raise ValueError('--lambda_feat > 0 needs --dis (the discriminator whose trunk gives the features), and must not be negative')
    if P.steps < 1 or P.restarts < 1 or P.batch_size < 1 or P.n < 1 or P.rows < 0:
        raise ValueError('--steps, --restarts, --batch_size and --n must be at least 1, --rows non-negative')
    from .sample import image_size_of
    image_size = tuple(image_size_of(Path(P.model_path).parent))
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
        raise ValueError('--rows %d: the figure shows 2 x rows of the %d recovered images' % (P.rows, P.n * len(splits)))
    if not torch.cuda.is_available():
        raise RuntimeError('latent recovery runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    from .models.gan import get_architecture
    G0, D0 = get_architecture(P.architecture, image_size)
    G = features.load_frozen(G0, P.model_path, dev)
    D = features.load_frozen(D0, P.dis, dev) if P.lambda_feat > 0 else None

    res, targets = {}, {}
    for j, s in enumerate(splits):
        u8 = torch.from_numpy(np.ascontiguousarray(sets[s][:P.n])).to(dev)
        res[s] = recover_images(G, D, u8, torch.arange(P.n), lambda_feat=P.lambda_feat, lr=P.lr, betas=tuple(P.betas),
                                adam_eps=P.adam_eps, steps=P.steps, batch_size=P.batch_size, restarts=P.restarts,
                                seed=seed + 7919 * j, graph=P.graph)
        targets[s] = u8
    out = {'model_path': P.model_path, 'architecture': P.architecture, 'data': P.data, 'synthetic': bool(P.synthetic), 'n': P.n,
           'holdout': bool(P.holdout), 'steps': P.steps, 'lr': P.lr, 'betas': list(P.betas), 'adam_eps': P.adam_eps,
           'restarts': P.restarts, 'lambda_feat': P.lambda_feat, 'dis': P.dis, 'batch_size': P.batch_size, 'seed': seed,
           'graph': bool(P.graph), 'rows': P.rows, 'image_size': list(image_size)}
    out.update(statistics(res['train']['pix'].numpy(), res['test']['pix'].numpy() if P.holdout else None))
    text = 'latent recovery (%d steps, lr %g): [train median pix %.6f, PSNR %.2f dB]' % (
        P.steps, P.lr, out['train']['median'], out['train']['psnr_median'])
    if P.holdout:
        text += ' [test median pix %.6f] [auc %.4f, z %.2f, median gap %.4f]' % (
            out['test']['median'], out['auc'], out['z_score'], out['median_gap'])
    print(text, flush=True)

    where = str(Path(P.model_path).parent)
    with open(os.path.join(where, 'recover_%d.json' % seed), 'w') as f:
        json.dump(out, f)
    cat = lambda k: np.concatenate([res[s][k].numpy() for s in splits])         # noqa: E731
    write_npz(os.path.join(where, 'recover_%d.npz' % seed), z=cat('z'), pix=cat('pix'), feat=cat('feat'),
              index=np.concatenate([np.arange(P.n, dtype=np.int64) for _ in splits]),
              split=np.concatenate([np.full(P.n, j, np.int64) for j, _ in enumerate(splits)]))
    if P.rows:
        tgt = torch.cat([features.to_float_nchw(targets[s], torch.arange(P.n, device=dev), torch.empty(P.n, 3, *image_size[:2], device=dev))
                         for s in splits])
        recon = torch.cat([res[s]['images'] for s in splits]).to(dev)
        order = np.argsort(cat('pix').astype(np.float64), kind='stable')
        chosen = np.concatenate([order[:P.rows], order[-P.rows:]])
        hostio.write_png(os.path.join(where, 'recover_%d.png' % seed), pair_grid(tgt, recon, chosen).cpu().numpy())
    return os.path.join(where, 'recover_%d.json' % seed)


if __name__ == '__main__':
    main()
