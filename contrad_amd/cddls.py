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
       [snresnet18: pooled seed -> per block, last to first: dgrads of conv2, conv1 and the shortcut conv, residual join
        -> RGB dgrad]
    -> image end (gradient through tanh, z2 update) -> G backward (conv forward kernels on the same packed weights,
    eval BatchNorm+ReLU backward, 1x1 dgrad) -> latent update (advances the device-resident step counter)

The noise comes from the in-kernel counter-based generator of csrc/cddls.hip: a draw depends on (seed, stream, step,
element) only, the step is read from device memory, so eager and ``--graph`` runs write bitwise-equal images.

Scope: ``sndcgan`` (any image size the modules accept) and ``snresnet18`` (G_SNDCGAN with D_SNResNet18, 32 x 32).  The
reference's ``clamp(z, -1, 1)`` belongs to SNDCGAN's uniform latent; other architectures raise NotImplementedError.
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

IMPLEMENTED = ('sndcgan', 'snresnet18')
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


class _DHalfSNDCGAN(object):
    """The D half of a Langevin step on D_SNDCGAN: seven plain convs, the logit head on the 8192 NHWC-flat features.
    Stateless: everything it prepares lives on the sampler ``S``.  ``forward`` / ``backward`` are the sampler's; latent
    recovery (recover.py) runs the trunk alone (``prep(S, head=False)``, ``forward_trunk``, ``seed_rows``,
    ``backward_trunk``) and never touches the logit head."""

    @staticmethod
    def geometry(S):
        S.hb, S.wb = S.D.s_hb, S.D.s_wb

    @staticmethod
    def class_row(S, w_row):
        return permute_class_row(w_row, S.hb, S.wb)

    @staticmethod
    def prep(S, head=True):
        D, dev, N = S.D, S.dev, S.n
        S.d_layers = [D.main[2 * i] for i in range(7)]
        T = S.hb * S.wb
        specs = [ops.SnSpec(m.weight_orig, m.weight_u, m.weight_v) for m in S.d_layers[:7]]
        sizes = [s.T * s.C * s.K for s in specs[:7]]
        ldws = [s.K for s in specs[:7]]
        if head:
            h = D._head()
            S.d_layers += [h.l1, h.l2]
            specs.append(ops.SnSpec(h.l1.weight_orig, h.l1.weight_u, h.l1.weight_v, view_kct=(S.dh, 512, T)))
            specs.append(ops.SnSpec(h.l2.weight_orig, h.l2.weight_u, h.l2.weight_v))
            sizes += [S.feat * S.dh, S.dh * 4]
            ldws += [S.dh, 4]
        S.d_wbuf, v = _flat_views(sizes, dev)
        S.d_wps = [v[i].view(s.T * s.C, s.K) for i, s in enumerate(specs[:7])]
        if head:
            S.d_wps += [v[7].view(S.feat, S.dh), v[8].view(S.dh, 4)]
        offs, scr_n = ops.sn_scratch_floats(specs)
        scratch = torch.empty(scr_n, device=dev, dtype=torch.float32)
        sigma = torch.empty(len(specs), device=dev, dtype=torch.float32)
        ops.sn_weight_prep(specs, S.d_wps, ldws, False, scratch, offs, sigma)      # eval: stored u, v, no iteration
        S.d_filters = None
        if ops.FILTER_PREP:
            reqs, hw = [], (8 * S.hb, 8 * S.wb)
            for i in range(1, 7):
                ci, co, k, s, p = _D_CONVS[i]
                d = ops.fwd_desc((N, hw[0], hw[1], ci), S.d_wps[i], co, k, k, s, p)
                reqs += [(0, d, S.d_wps[i]), (1, d, S.d_wps[i])]
                hw = (d.Ho, d.Wo)
            S.d_filters = ops.filter_prep(reqs, dev)

    @staticmethod
    def alloc(S, buf):
        N, hw, dshapes = S.n, (8 * S.hb, 8 * S.wb), []
        for ci, co, k, s, p in _D_CONVS:
            hw = (ops.out_size(hw[0], k, s, p), ops.out_size(hw[1], k, s, p))
            dshapes.append((N, hw[0], hw[1], co))
        S.d_acts = [buf(*s) for s in dshapes]
        S.d_grads = [buf(*s) for s in dshapes]
        S.d_feats = S.d_acts[6]                     # the penultimate features, (N, hb, wb, 512) NHWC

    @staticmethod
    def forward_trunk(S):
        w, L = S.d_wps, S.d_layers
        ops.rgb_conv_fwd(S.x, w[0], L[0].bias, 64, 3, 2.0, -1.0, _SLOPE, 1.0, out=S.d_acts[0])
        for i in range(1, 7):
            ci, co, k, s, p = _D_CONVS[i]
            ops.conv2d_fwd(S.d_acts[i - 1], w[i], L[i].bias, co, k, k, s, p, _SLOPE, 1.0, out=S.d_acts[i],
                           filters=S.d_filters)

    @staticmethod
    def forward(S):
        N, w, L = S.n, S.d_wps, S.d_layers
        _DHalfSNDCGAN.forward_trunk(S)
        ops.conv2d_fwd(S.d_acts[6].view(N, 1, 1, S.feat), w[7], L[7].bias, S.dh, 1, 1, 1, 0, _SLOPE, 1.0,
                       out=S.hidden)
        ops.conv2d_fwd(S.hidden, w[8], L[8].bias, 1, 1, 1, 1, 0, out=S.logits)

    @staticmethod
    def backward(S):
        N, w = S.n, S.d_wps
        ops.conv2d_dgrad(S.neg_one, w[8], (N, 1, 1, S.dh), 1, 1, 1, 0, act_ref=S.hidden, slope=_SLOPE, gain=1.0,
                         out=S.g_hidden)
        g = S.d_grads[6]
        ops.conv2d_dgrad(S.g_hidden, w[7], (N, 1, 1, S.feat), 1, 1, 1, 0, out=g.view(N, 1, 1, S.feat))
        ops.cddls_feature_seed(g, S.c_row, S.d_acts[6], _SLOPE, out=g)
        _DHalfSNDCGAN.backward_trunk(S, g)

    @staticmethod
    def seed_rows(S, rows, zero_row):
        """The trunk gradient seeded from per-sample rows at the features (N, feat): rows * lrelu'(a6)."""
        return ops.cddls_feature_seed(rows, zero_row, S.d_acts[6], _SLOPE, out=S.d_grads[6])

    @staticmethod
    def backward_trunk(S, g):
        w = S.d_wps
        for i in range(6, 0, -1):
            ci, co, k, s, p = _D_CONVS[i]
            a = S.d_acts[i - 1]
            g = ops.conv2d_dgrad(g, w[i], tuple(a.shape), k, k, s, p, act_ref=a, slope=_SLOPE, gain=1.0,
                                 out=S.d_grads[i - 1], filters=S.d_filters)
        ops.rgb_conv_dgrad(g, w[0], None, 3, 3, act=0, out_scale=2.0, out_shift=0.0, out=S.g_x)

    @staticmethod
    def regions(S):
        return [(a > 0).permute(0, 3, 1, 2) for a in S.d_acts]


class _DHalfSNResNet18(object):
    """The D half on D_SNResNet18 (32 x 32): the stem, eight residual blocks, the 4 x 4 mean, the logit head on the 512
    pooled features.  The backward walks the blocks last to first; the residual join and the pooled seed are index forms
    of the feature-seed kernel (csrc/cddls.hip).  Stateless like _DHalfSNDCGAN."""

    @staticmethod
    def geometry(S):
        S.hb, S.wb = S.G.s_hb, S.G.s_wb
        if (8 * S.hb, 8 * S.wb) != (32, 32):
            raise NotImplementedError('cDDLS sampling with D_SNResNet18: 32x32 images (its 4x4 average pool)')

    @staticmethod
    def class_row(S, w_row):
        return w_row                                # pooled features are in channel order already

    @staticmethod
    def _blocks(D):
        return [blk for li in range(1, 5) for blk in getattr(D, 'layer%d' % li)]

    @staticmethod
    def prep(S, head=True):
        D, dev, N = S.D, S.dev, S.n
        blocks = _DHalfSNResNet18._blocks(D)
        # (conv module, cin, cout, k, stride, pad, input map) of the trunk convs behind the stem, in execution order
        S.d_blocks, convs, hw, cin = [], [], 32, 64
        for blk in blocks:
            p, s = blk.planes, blk.stride
            ho = ops.out_size(hw, 3, s, 1)
            ent = {'c1': len(convs) + 1, 'c2': len(convs) + 2, 'sc': None, 'in': (N, hw, hw, cin), 'out': (N, ho, ho, p),
                   'planes': p, 'stride': s}
            convs += [(blk.conv1, cin, p, 3, s, 1, hw), (blk.conv2, p, p, 3, 1, 1, ho)]
            if len(blk.shortcut):
                ent['sc'] = len(convs) + 1
                convs.append((blk.shortcut[0], cin, p, 1, s, 0, hw))
            S.d_blocks.append(ent)
            hw, cin = ho, p
        S.d_layers = [D.conv1] + [c[0] for c in convs]
        if head:
            h = D._head()
            S.d_layers += [h.l1, h.l2]
        specs = [ops.SnSpec(m.weight_orig, m.weight_u, m.weight_v) for m in S.d_layers]
        ldws = [ops.round_up(s.K, 4) for s in specs]
        S.d_wbuf, v = _flat_views([s.T * s.C * ld for s, ld in zip(specs, ldws)], dev)
        S.d_wps = [v[i].view(s.T * s.C, ld) for i, (s, ld) in enumerate(zip(specs, ldws))]
        offs, scr_n = ops.sn_scratch_floats(specs)
        scratch = torch.empty(scr_n, device=dev, dtype=torch.float32)
        sigma = torch.empty(len(specs), device=dev, dtype=torch.float32)
        ops.sn_weight_prep(specs, S.d_wps, ldws, False, scratch, offs, sigma)      # eval: stored u, v, no iteration
        S.d_filters = None
        if ops.FILTER_PREP:
            reqs = []
            for i, (m, ci, co, k, s, p, h) in enumerate(convs, 1):
                d = ops.fwd_desc((N, h, h, ci), S.d_wps[i], co, k, k, s, p)
                reqs += [(0, d, S.d_wps[i]), (1, d, S.d_wps[i])]
            S.d_filters = ops.filter_prep(reqs, dev)

    @staticmethod
    def alloc(S, buf):
        N = S.n
        S.d_stem = buf(N, 32, 32, 64)
        S.d_c1 = [buf(*b['out']) for b in S.d_blocks]                       # conv1 outputs (post-LeakyReLU)
        S.d_sc = [buf(*b['out']) if b['sc'] is not None else None for b in S.d_blocks]
        S.d_outs = [buf(*b['out']) for b in S.d_blocks]                     # block outputs (post-LeakyReLU)
        S.d_acts = [S.d_stem] + [t for pair in zip(S.d_c1, S.d_outs) for t in pair]     # the 17 LeakyReLU outputs
        S.d_pre = buf(N * 32 * 32 * 64)                                     # a join's pre-activation, any block
        S.d_gbufs = [buf(N * 32 * 32 * 64) for _ in range(3)]               # rotating gradient storage, any level
        S.d_feats = buf(N, 512)                                             # the penultimate features (4 x 4 mean)
        S.g_feats = buf(N, 512)

    @staticmethod
    def _view(flat, shape):
        return flat[:math.prod(shape)].view(shape)

    @staticmethod
    def forward_trunk(S):
        w, L, view = S.d_wps, S.d_layers, _DHalfSNResNet18._view
        ops.rgb_conv_fwd(S.x, w[0], L[0].bias, 64, 3, 2.0, -1.0, _SLOPE, 1.0, out=S.d_stem)
        h = S.d_stem
        for j, b in enumerate(S.d_blocks):
            i1, i2, isc, p, s = b['c1'], b['c2'], b['sc'], b['planes'], b['stride']
            ops.conv2d_fwd(h, w[i1], L[i1].bias, p, 3, 3, s, 1, _SLOPE, 1.0, out=S.d_c1[j], filters=S.d_filters)
            sc = h
            if isc is not None:
                sc = ops.conv2d_fwd(h, w[isc], L[isc].bias, p, 1, 1, s, 0, out=S.d_sc[j], filters=S.d_filters)
            pre = view(S.d_pre, b['out'])
            ops.conv2d_fwd(S.d_c1[j], w[i2], L[i2].bias, p, 3, 3, 1, 1, 1.0, 1.0, out=pre, addend=sc, filters=S.d_filters)
            h = ops.fused_bias_act(pre, None, None, 3, 0, _SLOPE, 1.0, out=S.d_outs[j])
        torch.mean(h, (1, 2), out=S.d_feats)

    @staticmethod
    def forward(S):
        N, w, L = S.n, S.d_wps, S.d_layers
        _DHalfSNResNet18.forward_trunk(S)
        n = len(w)
        ops.conv2d_fwd(S.d_feats.view(N, 1, 1, 512), w[n - 2], L[n - 2].bias, S.dh, 1, 1, 1, 0, _SLOPE, 1.0, out=S.hidden)
        ops.conv2d_fwd(S.hidden, w[n - 1], L[n - 1].bias, 1, 1, 1, 1, 0, out=S.logits)

    @staticmethod
    def backward(S):
        N, w, view, n = S.n, S.d_wps, _DHalfSNResNet18._view, len(S.d_wps)
        ops.conv2d_dgrad(S.neg_one, w[n - 1], (N, 1, 1, S.dh), 1, 1, 1, 0, act_ref=S.hidden, slope=_SLOPE, gain=1.0,
                         out=S.g_hidden)
        ops.conv2d_dgrad(S.g_hidden, w[n - 2], (N, 1, 1, 512), 1, 1, 1, 0, out=S.g_feats.view(N, 1, 1, 512))
        _DHalfSNResNet18.backward_trunk(S, _DHalfSNResNet18.seed_rows(S, S.g_feats, S.c_row))

    @staticmethod
    def seed_rows(S, rows, row):
        """The gradient at the last join's pre-activation from per-sample rows (N, 512) at the pooled features plus one
        broadcast row: ((rows + row) / 16) * lrelu'(a), into the first of the rotating buffers."""
        return ops.cddls_pooled_seed(rows, row, S.d_outs[-1], _SLOPE,
                                     out=_DHalfSNResNet18._view(S.d_gbufs[0], S.d_blocks[-1]['out']))

    @staticmethod
    def backward_trunk(S, gp):
        w, view = S.d_wps, _DHalfSNResNet18._view
        P, Q, R = S.d_gbufs
        # gp: the gradient at the pre-activation of the join the walk stands at (seed_rows wrote it into P)
        for j in range(len(S.d_blocks) - 1, -1, -1):
            b = S.d_blocks[j]
            i1, i2, isc, p, s = b['c1'], b['c2'], b['sc'], b['planes'], b['stride']
            x_in = S.d_outs[j - 1] if j else S.d_stem
            t = ops.conv2d_dgrad(gp, w[i2], b['out'], 3, 3, 1, 1, act_ref=S.d_c1[j], slope=_SLOPE, gain=1.0,
                                 out=view(Q, b['out']), filters=S.d_filters)
            gm = ops.conv2d_dgrad(t, w[i1], b['in'], 3, 3, s, 1, out=view(R, b['in']), filters=S.d_filters)
            gs = gp                                 # identity shortcut: its branch gradient is the join's own
            if isc is not None:
                gs = ops.conv2d_dgrad(gp, w[isc], b['in'], 1, 1, s, 0, out=view(Q, b['in']), filters=S.d_filters)
            gp = ops.cddls_join_bwd(gm, gs, x_in, _SLOPE, out=gm)
            P, R = R, P
        ops.rgb_conv_dgrad(gp, w[0], None, 3, 3, act=0, out_scale=2.0, out_shift=0.0, out=S.g_x)

    @staticmethod
    def regions(S):
        return [(a > 0).permute(0, 3, 1, 2) for a in S.d_acts]


def _d_half(D):
    from .models.gan.sndcgan import D_SNDCGAN
    from .models.gan.snresnet import D_SNResNet18
    if isinstance(D, D_SNDCGAN):
        return _DHalfSNDCGAN
    if isinstance(D, D_SNResNet18):
        return _DHalfSNResNet18
    return None


class _GHalf(object):
    """The G half of a step on G_SNDCGAN in eval mode, on static buffers: the constant prep, the forward that keeps its
    activations and the hand-written backward to ``g_z``.  Shared by CDDLSSampler and recover.LatentRecovery, which set
    ``G``, ``dev``, ``n``, ``hb``, ``wb``, ``feat`` and allocate ``z``, ``g_z``, ``h0``, ``g_h0``, ``gout``, ``g_lin``,
    ``g_acts``, ``g_grads``."""

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
        # eval-mode BatchNorm through the as-is form of the apply kernel (ops.bn_relu_apply_eval): mean = running_mean -
        # conv bias (the transposed conv runs without its bias), made once here; the variance is running_var itself, the
        # tensor the backward kernel reads, so the step's backward is the derivative of its forward
        self.g_bns = [G.norm_init] + [G.main[3 * j + 1] for j in range(3)]
        self.g_means = [ops.bn_eval_mean(bn, cb).clone()
                        for bn, cb in zip(self.g_bns, [None] + [G.main[3 * j].bias for j in range(3)])]

    def _g_forward(self):
        G, N, f, w = self.G, self.n, self.feat, self.g_wps
        ops.conv2d_fwd(self.z.view(N, 1, 1, G.nz), w[0], G.linear.bias, f, 1, 1, 1, 0, out=self.h0.view(N, 1, 1, f))
        bn = self.g_bns[0]
        ops.bn_relu_apply_eval(self.h0, self.g_acts[0].view(N, f), self.g_means[0], bn.running_var, bn.weight, bn.bias,
                               bn.eps, self.hb * self.wb)
        for j in range(3):
            ci, co, k, s, p = G._CONVT[j]
            y = self.g_acts[j + 1]
            ops.conv2d_dgrad(self.g_acts[j], w[1 + j], tuple(y.shape), k, k, s, p, out=y, filters=self.g_filters)
            bn, y2 = self.g_bns[j + 1], ops.as_rows(y)
            ops.bn_relu_apply_eval(y2, y2, self.g_means[j + 1], bn.running_var, bn.weight, bn.bias, bn.eps)
        ops.rgb_conv_dgrad(self.g_acts[3], w[4], G.main[9].bias, 3, 3, act=1, out_scale=0.5, out_shift=0.5, out=self.gout)

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

    def _g_regions(self):
        """The ReLU regions of the last forward in the reference's layouts: after norm_init (N, f) NCHW-flat, then three
        NCHW maps."""
        g = [(self.g_acts[0] > 0).permute(0, 3, 1, 2).reshape(self.n, self.feat)]
        return g + [(a > 0).permute(0, 3, 1, 2) for a in self.g_acts[1:]]


class CDDLSSampler(_GHalf):
    """Langevin sampler for one batch size on static buffers.  ``G`` / ``D``: eval-mode modules on the device (G_SNDCGAN
    with D_SNDCGAN or D_SNResNet18); ``weight`` / ``bias``: the linear-evaluation head (n_classes, d_penul) / (n_classes,).
    The G half, the element-wise ends, the noise and the step counter are shared; the D half (prep, buffers, forward,
    backward, linear regions) is _DHalfSNDCGAN or _DHalfSNResNet18, chosen by the type of ``D``."""

    def __init__(self, G, D, weight, bias, n, lbd=1.0, eps=0.01, sigma_n=0.1, seed=0, graph=False, energy=False):
        from .models.gan.sndcgan import G_SNDCGAN
        self.half = _d_half(D)
        if not isinstance(G, G_SNDCGAN) or self.half is None:
            raise NotImplementedError('cDDLS sampling is implemented for: %s' % ', '.join(IMPLEMENTED))
        if G.training or D.training:
            raise RuntimeError('cDDLS samples from networks in eval mode')
        self.weight, self.bias = weight.detach(), bias.detach()
        if tuple(self.weight.shape[1:]) != (D.d_penul,):
            raise RuntimeError('the linear head reads %d features, D has %d' % (self.weight.shape[1], D.d_penul))
        dev = next(D.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('cDDLS sampling runs on the MI355X HIP path only (no CPU fallback)')
        self.G, self.D, self.n, self.dev = G, D, int(n), dev
        self.lbd, self.eps, self.sigma_n, self.seed = float(lbd), float(eps), float(sigma_n), int(seed)
        self.use_graph, self.want_energy = bool(graph), bool(energy)
        self.graph, self.first, self._scratch = None, EagerFirst(), {}
        self.half.geometry(self)
        self.feat, self.dh, self.d_feat = 512 * self.hb * self.wb, D.d_hidden, D.d_penul     # feat: G's first map, flat
        with torch.no_grad():
            self._prep_d()
            self._prep_g()
            self._alloc()

    # ---- constant work ----
    def _prep_d(self):
        self.half.prep(self)

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
        self.half.alloc(self, buf)
        self.hidden, self.g_hidden = buf(N, 1, 1, self.dh), buf(N, 1, 1, self.dh)
        self.logits = buf(N, 1, 1, 1)
        self.neg_one = torch.full((N, 1, 1, 1), -1.0, device=dev)      # d(-(d + lbd l)) / d d
        self.c_row, self.bias_term = buf(self.d_feat), buf(1)
        self.energy = buf(N)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)      # {step, arrival counter of the latent update}
        self.cls = None

    # ---- per class / per batch ----
    def set_class(self, y):
        with torch.no_grad():
            self.c_row.copy_(self.half.class_row(self, self.weight[y])).mul_(-self.lbd)
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
    def _d_forward(self):
        self.half.forward(self)

    def _d_backward(self):
        self.half.backward(self)

    def _body(self, noise=None, noise2=None):
        with torch.no_grad():
            self._g_forward()
            ops.cddls_compose(self.gout, self.z2, self.eps, out=self.x)
            self._d_forward()
            if self.want_energy:
                ops.cddls_energy(self.logits.view(self.n, 1), self.d_feats, self.c_row, self.bias_term, self.z2,
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
        after norm_init (N, f) NCHW-flat, then three NCHW maps; D: NCHW maps in execution order -- seven for sndcgan, 17
        for snresnet18 (stem, then conv1 and join of every block); the logit head's hidden (N, dh))."""
        return {'g': self._g_regions(), 'd': self.half.regions(self), 'hidden': (self.hidden > 0).view(self.n, self.dh)}


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
