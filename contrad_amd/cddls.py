"""Conditional sampling from an unconditional ContraD GAN by Langevin dynamics in latent space (cDDLS): the reference's
``test_gan_sample_cddls.py`` on the MI355X path.  Same CLI (``logdir linear_path architecture --lbd --n_steps --eps
--sigma_n --n_samples --n_classes --batch_size``), same arithmetic (``_sample_cddls``), same output tree
(``logdir/samples_cDDLS_<tag>/<y>/<index>.png``) plus one ``samples.npz`` (uint8 images, labels).

Both networks are frozen for the whole run, so everything constant is done ONCE per sampler: the eval-mode spectral-norm
weight prep of D's trunk and logit head (the two projection heads are never read), the Winograd filters of D's forward
and data gradient and of G's forward and backward at this batch size, G's packed weights, the eval-mode BatchNorm
statistics.  One Langevin step is then a fixed chain of launches on static buffers -- no autograd graph, no allocation --
that ``--graph`` captures once and replays ``n_steps - 1`` times:

    G forward (kept activations) -> x = G(z) + eps z2 -> D trunk + logit head forward -> [energy]
    -> logit-head dgrads (seed -1) -> feature seed (+ class row, lrelu') -> 6 trunk dgrads + RGB dgrad
    -> image end (gradient through tanh, z2 update) -> G backward (conv forward kernels on the same packed weights,
    eval BatchNorm+ReLU backward, 1x1 dgrad) -> latent update (advances the device-resident step counter)

The noise comes from the in-kernel counter-based generator of csrc/cddls.hip: a draw depends on (seed, stream, step,
element) only, the step is read from device memory, so eager and ``--graph`` runs write bitwise-equal images.

Scope: ``sndcgan`` (any image size the modules accept).  The reference's ``clamp(z, -1, 1)`` belongs to SNDCGAN's uniform
latent; other architectures raise NotImplementedError.
"""
import math
import os
from argparse import ArgumentParser

import numpy as np
import torch

from . import ops
from .captured import EagerFirst, capture
from .hostio import THROTTLE, to_uint8, write_png
from .models.gan.sndcgan import _D_CONVS, _SLOPE, _flat_views

IMPLEMENTED = ('sndcgan',)
STREAM_INIT = 2          # stream id of the initial z2 (csrc/cddls.hip: CD_STREAM_INIT; 0 and 1 are drawn inside the update kernels)


def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: Sampling from G via cDDLS (one process, one GPU)')
    parser.add_argument('logdir', type=str, help='Path to the logdir that contains the (best) checkpoints of G and D')
    parser.add_argument('linear_path', type=str, help='Path to the checkpoint trained from linear evaluation')
    parser.add_argument('architecture', type=str, help='Architecture')
    # Options for Langevin sampling
    parser.add_argument('--lbd', default=1.0, type=float)
    parser.add_argument('--n_steps', default=1000, type=int)
    parser.add_argument('--eps', default=0.01, type=float)
    parser.add_argument('--sigma_n', default=0.1, type=float)
    parser.add_argument('--n_samples', default=10000, type=int, help='Number of samples to generate (default: 10000)')
    parser.add_argument('--n_classes', default=10, type=int, help='Number of classes (default: 10)')
    parser.add_argument('--batch_size', default=500, type=int, help='Batch size (default: 500)')
    # additions
    parser.add_argument('--seed', default=None, type=int, help='RNG seed and directory tag (default: drawn)')
    parser.add_argument('--graph', action='store_true', help='replay the Langevin step from a captured hipGraph')
    parser.add_argument('--log_energy', action='store_true', help='print the mean energy of the first and last step')
    return parser.parse_args(argv)


def batch_plan(n_samples, n_classes, batch_size):
    """The reference's loop (test_gan_sample_cddls.py:134-148) as a list of (class, batch, offset, images kept): index =
    y * (n_samples // n_classes) + i * batch_size + j, and a batch stops where the index reaches n_samples.  Declared
    deviation: a class's last batch also stops at the class's own share (the reference writes its surplus images under
    indices that belong to the next class), so exactly n_classes * (n_samples // n_classes) images are kept."""
    class_samples = n_samples // n_classes
    n_batches = int(math.ceil(class_samples / batch_size))
    plan = []
    for y in range(n_classes):
        for i in range(n_batches):
            offset = y * class_samples + i * batch_size
            plan.append((y, i, offset, max(0, min(batch_size, class_samples - i * batch_size, n_samples - offset))))
    return plan


def permute_class_row(w_row, hb, wb):
    """A classifier row over the NCHW-flattened penultimate features (512, hb, wb) in the trunk's NHWC order."""
    return w_row.reshape(512, hb * wb).t().reshape(-1)


class CDDLSSampler(object):
    """Langevin sampler for one batch size on static buffers.  ``G`` / ``D``: eval-mode SNDCGAN modules on the device;
    ``weight`` / ``bias``: the linear-evaluation head (n_classes, d_penul) / (n_classes,)."""

    def __init__(self, G, D, weight, bias, n, lbd=1.0, eps=0.01, sigma_n=0.1, seed=0, graph=False, energy=False):
        from .models.gan.sndcgan import D_SNDCGAN, G_SNDCGAN
        if not isinstance(G, G_SNDCGAN) or not isinstance(D, D_SNDCGAN):
            raise NotImplementedError('cDDLS sampling is implemented for: %s' % ', '.join(IMPLEMENTED))
        if G.training or D.training:
            raise RuntimeError('cDDLS samples from networks in eval mode')
        dev = next(D.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('cDDLS sampling runs on the MI355X HIP path only (no CPU fallback)')
        self.G, self.D, self.n, self.dev = G, D, int(n), dev
        self.lbd, self.eps, self.sigma_n, self.seed = float(lbd), float(eps), float(sigma_n), int(seed)
        self.use_graph, self.want_energy = bool(graph), bool(energy)
        self.graph, self.first, self._scratch = None, EagerFirst(), {}
        self.hb, self.wb = D.s_hb, D.s_wb
        self.feat, self.dh = 512 * self.hb * self.wb, D.d_hidden
        self.weight, self.bias = weight.detach(), bias.detach()
        if tuple(self.weight.shape[1:]) != (self.feat,):
            raise RuntimeError('the linear head reads %d features, D has %d' % (self.weight.shape[1], self.feat))
        with torch.no_grad():
            self._prep_d()
            self._prep_g()
            self._alloc()

    # ---- constant work ----
    def _prep_d(self):
        D, dev, N = self.D, self.dev, self.n
        head = D._head()
        self.d_layers = [D.main[2 * i] for i in range(7)] + [head.l1, head.l2]
        T = self.hb * self.wb
        specs = [ops.SnSpec(m.weight_orig, m.weight_u, m.weight_v) for m in self.d_layers[:7]]
        specs.append(ops.SnSpec(head.l1.weight_orig, head.l1.weight_u, head.l1.weight_v, view_kct=(self.dh, 512, T)))
        specs.append(ops.SnSpec(head.l2.weight_orig, head.l2.weight_u, head.l2.weight_v))
        sizes = [s.T * s.C * s.K for s in specs[:7]] + [self.feat * self.dh, self.dh * 4]
        self.d_wbuf, v = _flat_views(sizes, dev)
        self.d_wps = [v[i].view(s.T * s.C, s.K) for i, s in enumerate(specs[:7])]
        self.d_wps += [v[7].view(self.feat, self.dh), v[8].view(self.dh, 4)]
        ldws = [s.K for s in specs[:7]] + [self.dh, 4]
        offs, scr_n = ops.sn_scratch_floats(specs)
        scratch = torch.empty(scr_n, device=dev, dtype=torch.float32)
        sigma = torch.empty(len(specs), device=dev, dtype=torch.float32)
        ops.sn_weight_prep(specs, self.d_wps, ldws, False, scratch, offs, sigma)      # eval: stored u, v, no iteration
        self.d_filters = None
        if ops.FILTER_PREP:
            reqs, hw = [], (8 * self.hb, 8 * self.wb)
            for i in range(1, 7):
                ci, co, k, s, p = _D_CONVS[i]
                d = ops.fwd_desc((N, hw[0], hw[1], ci), self.d_wps[i], co, k, k, s, p)
                reqs += [(0, d, self.d_wps[i]), (1, d, self.d_wps[i])]
                hw = (d.Ho, d.Wo)
            self.d_filters = ops.filter_prep(reqs, dev)

    def _prep_g(self):
        G, dev, N = self.G, self.dev, self.n
        self.g_wps = G._weights()
        self.g_filters = None
        if ops.FILTER_PREP:
            reqs, H, W = [], self.hb, self.wb
            for j in range(3):
                ci, co, k, s, p = G._CONVT[j]
                H, W = 2 * H, 2 * W
                d = ops.dgrad_desc((N, H, W, co), self.g_wps[1 + j], ci, k, k, s, p)
                reqs += [(1, d, self.g_wps[1 + j]), (0, d, self.g_wps[1 + j])]       # forward = dgrad, backward = fwd
            self.g_filters = ops.filter_prep(reqs, dev)
        # eval-mode BatchNorm through the batch-statistics apply kernel: "one sample" whose sums give mean =
        # running_mean - conv bias (the transposed conv runs without its bias) and variance = running_var
        self.g_bns = [G.norm_init] + [G.main[3 * j + 1] for j in range(3)]
        self.g_stats = []
        for bn, cb in zip(self.g_bns, [None] + [G.main[3 * j].bias for j in range(3)]):
            mean = bn.running_mean if cb is None else bn.running_mean - cb
            self.g_stats.append(torch.stack([mean, bn.running_var + mean * mean]).contiguous())

    def _alloc(self):
        N, dev, hb, wb = self.n, self.dev, self.hb, self.wb
        H, W = 8 * hb, 8 * wb

        def buf(*shape):
            return torch.zeros(shape, device=dev, dtype=torch.float32)
        self.z, self.g_z = buf(N, self.G.nz), buf(N, self.G.nz)
        self.z2, self.gout, self.x, self.g_x, self.g_lin = (buf(N, 3, H, W) for _ in range(5))
        self.h0, self.g_h0 = buf(N, self.feat), buf(N, self.feat)
        gshapes = [(N, hb, wb, 512), (N, 2 * hb, 2 * wb, 256), (N, 4 * hb, 4 * wb, 128), (N, H, W, 64)]
        self.g_acts = [buf(*s) for s in gshapes]
        self.g_grads = [buf(*s) for s in gshapes]
        dshapes, hw = [], (H, W)
        for ci, co, k, s, p in _D_CONVS:
            hw = (ops.out_size(hw[0], k, s, p), ops.out_size(hw[1], k, s, p))
            dshapes.append((N, hw[0], hw[1], co))
        self.d_acts = [buf(*s) for s in dshapes]
        self.d_grads = [buf(*s) for s in dshapes]
        self.hidden, self.g_hidden = buf(N, 1, 1, self.dh), buf(N, 1, 1, self.dh)
        self.logits = buf(N, 1, 1, 1)
        self.neg_one = torch.full((N, 1, 1, 1), -1.0, device=dev)      # d(-(d + lbd l)) / d d
        self.c_row, self.bias_term = buf(self.feat), buf(1)
        self.energy = buf(N)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)      # {step, arrival counter of the latent update}
        self.cls = None

    # ---- per class / per batch ----
    def set_class(self, y):
        with torch.no_grad():
            self.c_row.copy_(permute_class_row(self.weight[y], self.hb, self.wb)).mul_(-self.lbd)
            self.bias_term.copy_(self.bias[y:y + 1]).mul_(-self.lbd)
        self.cls = int(y)

    def start(self, z0, first_step=0, z2=None):
        """New chain: ``z`` = z0, the step counter = ``first_step``, ``z2`` = the generator's stream 2 at that step (or
        the given tensor)."""
        with torch.no_grad():
            self.z.copy_(z0)
            self.state.copy_(torch.tensor([first_step, 0, 0, 0], dtype=torch.int32))
            if z2 is not None:
                self.z2.copy_(z2)
            else:
                ops.cddls_normal_fill(self.z2.numel(), self.seed, STREAM_INIT, step_dev=self.state, out=self.z2.view(-1))

    # ---- one Langevin step ----
    def _g_forward(self):
        G, N, f, w = self.G, self.n, self.feat, self.g_wps
        ops.conv2d_fwd(self.z.view(N, 1, 1, G.nz), w[0], G.linear.bias, f, 1, 1, 1, 0, out=self.h0.view(N, 1, 1, f))
        bn = self.g_bns[0]
        ops.bn_relu_apply(self.h0, self.g_acts[0].view(N, f), self.g_stats[0], 1.0, bn.weight, bn.bias, bn.eps,
                          self.hb * self.wb)
        for j in range(3):
            ci, co, k, s, p = G._CONVT[j]
            y = self.g_acts[j + 1]
            ops.conv2d_dgrad(self.g_acts[j], w[1 + j], tuple(y.shape), k, k, s, p, out=y, filters=self.g_filters)
            bn, y2 = self.g_bns[j + 1], ops.as_rows(y)
            ops.bn_relu_apply(y2, y2, self.g_stats[j + 1], 1.0, bn.weight, bn.bias, bn.eps)
        ops.rgb_conv_dgrad(self.g_acts[3], w[4], G.main[9].bias, 3, 3, act=1, out_scale=0.5, out_shift=0.5, out=self.gout)

    def _d_forward(self):
        N, w, L = self.n, self.d_wps, self.d_layers
        ops.rgb_conv_fwd(self.x, w[0], L[0].bias, 64, 3, 2.0, -1.0, _SLOPE, 1.0, out=self.d_acts[0])
        for i in range(1, 7):
            ci, co, k, s, p = _D_CONVS[i]
            ops.conv2d_fwd(self.d_acts[i - 1], w[i], L[i].bias, co, k, k, s, p, _SLOPE, 1.0, out=self.d_acts[i],
                           filters=self.d_filters)
        ops.conv2d_fwd(self.d_acts[6].view(N, 1, 1, self.feat), w[7], L[7].bias, self.dh, 1, 1, 1, 0, _SLOPE, 1.0,
                       out=self.hidden)
        ops.conv2d_fwd(self.hidden, w[8], L[8].bias, 1, 1, 1, 1, 0, out=self.logits)

    def _d_backward(self):
        N, w = self.n, self.d_wps
        ops.conv2d_dgrad(self.neg_one, w[8], (N, 1, 1, self.dh), 1, 1, 1, 0, act_ref=self.hidden, slope=_SLOPE, gain=1.0,
                         out=self.g_hidden)
        g = self.d_grads[6]
        ops.conv2d_dgrad(self.g_hidden, w[7], (N, 1, 1, self.feat), 1, 1, 1, 0, out=g.view(N, 1, 1, self.feat))
        ops.cddls_feature_seed(g, self.c_row, self.d_acts[6], _SLOPE, out=g)
        for i in range(6, 0, -1):
            ci, co, k, s, p = _D_CONVS[i]
            a = self.d_acts[i - 1]
            g = ops.conv2d_dgrad(g, w[i], tuple(a.shape), k, k, s, p, act_ref=a, slope=_SLOPE, gain=1.0,
                                 out=self.d_grads[i - 1], filters=self.d_filters)
        ops.rgb_conv_dgrad(g, w[0], None, 3, 3, act=0, out_scale=2.0, out_shift=0.0, out=self.g_x)

    def _g_backward(self):
        G, N, f, w = self.G, self.n, self.feat, self.g_wps
        # a transposed conv's backward is the conv forward kernel on the same packed weights
        ops.rgb_conv_fwd(self.g_lin, w[4], None, 64, 3, 1.0, 0.0, 1.0, 1.0, out=self.g_grads[3])
        for j in range(2, -1, -1):
            ci, co, k, s, p = G._CONVT[j]
            bn, g2 = self.g_bns[j + 1], ops.as_rows(self.g_grads[j + 1])
            ops.bn_relu_bwd_eval(g2, ops.as_rows(self.g_acts[j + 1]), g2, bn.weight, bn.running_var, bn.eps)
            ops.conv2d_fwd(self.g_grads[j + 1], w[1 + j], None, ci, k, k, s, p, out=self.g_grads[j], filters=self.g_filters)
        bn = self.g_bns[0]
        ops.bn_relu_bwd_eval(self.g_grads[0].view(N, f), self.g_acts[0].view(N, f), self.g_h0, bn.weight, bn.running_var,
                             bn.eps, perm_hw=self.hb * self.wb)
        ops.conv2d_dgrad(self.g_h0.view(N, 1, 1, f), w[0], (N, 1, 1, G.nz), 1, 1, 1, 0, out=self.g_z.view(N, 1, 1, G.nz))

    def _body(self, noise=None, noise2=None):
        with torch.no_grad():
            self._g_forward()
            ops.cddls_compose(self.gout, self.z2, self.eps, out=self.x)
            self._d_forward()
            if self.want_energy:
                ops.cddls_energy(self.logits.view(self.n, 1), self.d_acts[6], self.c_row, self.bias_term, self.z2,
                                 out=self.energy)
            self._d_backward()
            ops.cddls_image_end(self.g_x, self.gout, self.z2, self.g_lin, self.eps, self.sigma_n, noise=noise2,
                                seed=self.seed, state=self.state)
            self._g_backward()
            ops.cddls_latent_update(self.z, self.g_z, self.eps, self.sigma_n, noise=noise, seed=self.seed, state=self.state)

    def step(self, noise=None, noise2=None):
        """One Langevin step.  ``noise`` (N, nz) / ``noise2`` (N, 3, H, W): explicit normals instead of the generator's
        (eager only)."""
        if self.cls is None:
            raise RuntimeError('set_class() first')
        explicit = noise is not None or noise2 is not None           # such a step neither counts as the eager one nor captures
        if not self.use_graph or not self.first.may_capture(counts=not explicit):
            return self._body(noise, noise2)
        if self.graph is None:
            self.graph, _ = capture(self._body, (self.D,), self._scratch)
        self.graph.replay()

    def images(self):
        """clamp(G(z) + eps z2, 0, 1) of the current state, NCHW (a new tensor)."""
        with torch.no_grad():
            self._g_forward()
            return ops.cddls_compose(self.gout, self.z2, self.eps, clamp01=True)

    def sample(self, y, z0, n_steps, first_step=0):
        """The reference's ``_sample_cddls`` for class ``y`` from latents ``z0`` -> (images, mean energy of the first and
        of the last step, or None without ``energy``)."""
        self.set_class(y)
        self.start(z0, first_step)
        e_first = None
        for k in range(n_steps):
            THROTTLE.begin()                      # the host stays at most one step ahead (hostio.py)
            self.step()
            THROTTLE.end()
            if k == 0 and self.want_energy:
                e_first = self.energy.mean().item()
        e = (e_first, self.energy.mean().item()) if (self.want_energy and n_steps > 0) else None
        return self.images(), e

    def linear_region(self):
        """Test hook: the ReLU / LeakyReLU regions the last step ran on, as bool masks in the reference's layouts (G:
        after norm_init (N, f) NCHW-flat, then three NCHW maps; D: seven NCHW maps; the logit head's hidden (N, dh))."""
        N = self.n
        g = [(self.g_acts[0] > 0).permute(0, 3, 1, 2).reshape(N, self.feat)]
        g += [(a > 0).permute(0, 3, 1, 2) for a in self.g_acts[1:]]
        d = [(a > 0).permute(0, 3, 1, 2) for a in self.d_acts]
        return {'g': g, 'd': d, 'hidden': (self.hidden > 0).view(N, self.dh)}


def load_networks(logdir, linear_path, architecture, n_classes, dev):
    """(G, D, head weight, head bias) from ``gen_best.pt`` / ``dis_best.pt`` in ``logdir`` and the lin-eval checkpoint."""
    from .lineval import _dataset_name
    from .models.gan import get_architecture
    from .data import TRAIN_GAN_IMAGE_SIZES as IMAGE_SIZES
    dataset = _dataset_name(logdir)
    if dataset is None:
        raise RuntimeError('%s holds no *.gin file naming the dataset' % logdir)
    if dataset not in IMAGE_SIZES:
        raise NotImplementedError("cDDLS sampling for dataset '%s' (implemented: %s)" % (dataset, sorted(IMAGE_SIZES)))
    G, D = get_architecture(architecture, IMAGE_SIZES[dataset])
    G.load_state_dict(torch.load(os.path.join(logdir, 'gen_best.pt'), map_location='cpu'))
    D.load_state_dict(torch.load(os.path.join(logdir, 'dis_best.pt'), map_location='cpu'))
    sd = torch.load(linear_path, map_location='cpu')['state_dict']
    weight, bias = sd['linear.weight'].float(), sd['linear.bias'].float()
    if tuple(weight.shape) != (n_classes, D.d_penul):
        raise RuntimeError('linear.weight is %s, expected (%d, %d)' % (tuple(weight.shape), n_classes, D.d_penul))
    G.to(dev).eval()
    D.to(dev).eval()
    for p in list(G.parameters()) + list(D.parameters()):
        p.requires_grad_(False)
    return G, D, weight.to(dev), bias.to(dev)


def main(argv=None):
    P = parse_args(argv)
    if P.architecture not in IMPLEMENTED:
        raise NotImplementedError("cDDLS sampling of architecture '%s' (implemented: %s; the clamp of z to [-1, 1] "
                                  "belongs to SNDCGAN's uniform latent)" % (P.architecture, ', '.join(IMPLEMENTED)))
    if not torch.cuda.is_available():
        raise RuntimeError('cDDLS sampling runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    torch.manual_seed(seed); np.random.seed(seed)
    G, D, weight, bias = load_networks(P.logdir, P.linear_path, P.architecture, P.n_classes, dev)

    subdir = os.path.join(P.logdir, 'samples_cDDLS_%d' % seed)
    os.makedirs(subdir, exist_ok=True)
    print('Sampling in %s' % subdir, flush=True)
    sampler = CDDLSSampler(G, D, weight, bias, P.batch_size, lbd=P.lbd, eps=P.eps, sigma_n=P.sigma_n, seed=seed,
                           graph=P.graph, energy=P.log_energy)
    all_images, all_labels = [], []
    for b, (y, i, offset, keep) in enumerate(batch_plan(P.n_samples, P.n_classes, P.batch_size)):
        os.makedirs(os.path.join(subdir, str(y)), exist_ok=True)
        z0 = G.sample_latent(P.batch_size)
        # one seed, disjoint step ranges: batch b draws the counters of steps b * (n_steps + 1) ...
        images, e = sampler.sample(y, z0, P.n_steps, first_step=b * (P.n_steps + 1))
        if e is not None:
            print('class %d batch %d: mean energy %.4f (first step) -> %.4f (last step)' % (y, i, e[0], e[1]), flush=True)
        u8 = to_uint8(images[:keep]).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        for j in range(keep):
            write_png(os.path.join(subdir, str(y), '%d.png' % (offset + j)), u8[j])
        all_images.append(u8)
        all_labels.append(np.full(keep, y, np.int64))
    np.savez(os.path.join(subdir, 'samples.npz'), images=np.concatenate(all_images), labels=np.concatenate(all_labels))
    return subdir


if __name__ == '__main__':
    main()
