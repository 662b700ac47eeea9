"""Counterpart of the reference's ``augment`` package for the hot-path pipelines: ``get_augment('simclr')`` and
``get_augment('simclr_hq')`` (augment/__init__.py:13-28,106-122).

The reference composes ~25 PyTorch ops per call (two grid_samples, HSV round trip, blends); here the random
parameters are drawn on the HOST in the reference's exact RNG order (numpy global RNG for geometry / op order /
blur sigma, torch CPU generator for masks and colour factors -- SURVEY.md 8a row A7), shipped as one small
(B, 16) tensor, and a single fused HIP kernel does crop+flip+jitter+gray (plus a separable blur for *_hq).

The augmentations of the baseline training modes follow the same split -- ``sample()`` on the host in the reference's draw
order, ``apply()`` on the device, an autograd Function when the input requires grad: ``none``, ``hflip`` / ``hfrt``
(augment/spatial.py:14-40,70-93: an index map and its adjoint gather) and ``diffaug`` (third_party/diffaug.py: one fused
launch per direction on CIFAR-sized images); kernels in csrc/baseline_aug.hip, DESIGN.md section 12.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..hostio import upload
from ..config import configurable, get_bindings

__all__ = ['get_augment', 'SimCLRAugment', 'simclr', 'simclr_hq', 'simclr_hq_cutout', 'NoAugment', 'HorizontalFlipLayer',
           'HorizontalFlipRandomCrop', 'DiffAugLayer', 'diffaug']


def _jitter_range(value, center=1.0, clip_first_on_zero=True):
    """Scalar branch of ColorJitterLayer._check_input (augment/color_jitter.py:25-42)."""
    if value < 0:
        raise ValueError('jitter strength must be non negative')
    lo, hi = center - value, center + value
    if clip_first_on_zero:
        lo = max(lo, 0)
    if lo == hi == center:
        return None
    return [lo, hi]


class _SimCLRFn(torch.autograd.Function):
    """Differentiable (w.r.t. the images) fused augmentation for the generator step: gradient flows through the
    bilinear crop/flip gather, the contrast stage, -- as an identity, like RandomHSVFunction.backward
    (augment/color_jitter.py:97-104) -- through the HSV jitter, and through the masked Gaussian blur of simclr_hq
    (its reflect-padding transpose)."""

    @staticmethod
    def forward(ctx, x, Pd, contrast_first, has_contrast, blur, cutout):
        out = ops.simclr_augment(x, Pd, contrast_first, has_contrast)
        if blur is not None:
            radius, g = blur
            out = ops.gaussian_blur_masked(out, Pd, g, radius)
            ctx.save_for_backward(x, Pd, g)
        else:
            ctx.save_for_backward(x, Pd)
        if cutout is not None:
            ops.cutout_masked_(out, Pd, cutout)
        ctx.cfg = (contrast_first, has_contrast, None if blur is None else blur[0], cutout)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        cf, hc, radius, cutout = ctx.cfg
        if cutout is not None:
            g = ops.cutout_masked_(g.contiguous().clone(), ctx.saved_tensors[1], cutout)
        if radius is not None:
            x, Pd, gk = ctx.saved_tensors
            g = ops.gaussian_blur_masked_bwd(g, Pd, gk, radius)
        else:
            x, Pd = ctx.saved_tensors
        return ops.simclr_augment_bwd(x, Pd, g, cf, hc), None, None, None, None, None


class SimCLRAugment(nn.Module):
    """RandomResizeCrop -> HorizontalFlip -> RandomApply(ColorJitter, 0.8) -> RandomApply(Gray, 0.2)
    [-> RandomApply(GaussianBlur, 0.5)] [-> RandomApply(CutOut, 0.5)] as one module; maps NCHW float [0,1] to the same
    shape."""

    def __init__(self, scale, ratio=(3. / 4., 4. / 3.), brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1,
                 p_jitter=0.8, p_gray=0.2, p_blur=None, sigma_range=None, p_cutout=None, cutout_length=None):
        super().__init__()
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.r_v = _jitter_range(brightness)
        self.r_c = _jitter_range(contrast)
        self.r_s = _jitter_range(saturation)
        self.r_h = _jitter_range(hue, center=0, clip_first_on_zero=False)
        if self.r_h is not None and not (-0.5 <= self.r_h[0] <= self.r_h[1] <= 0.5):
            raise ValueError('hue values should be between (-0.5, 0.5)')
        self.p_jitter, self.p_gray, self.p_blur = p_jitter, p_gray, p_blur
        self.sigma_range = sigma_range
        self.p_cutout, self.cutout_length = p_cutout, cutout_length
        if p_cutout is not None and (cutout_length is None or cutout_length % 2 == 0):
            raise ValueError("Currently CutOut only accepts odd lengths: length % 2 == 1")        # spatial.py:156-157

    supports_out = True          # forward(x, out=...): the last stage writes into the caller's buffer (no-grad path)

    # ---- host-side sampling, reference draw order ----
    def sample(self, B, dim2, dim3):
        """Returns (params (B,12) CPU float tensor, contrast_first, sigma or None)."""
        P = torch.zeros(B, ops.AUG_NPARAM)
        width, height = dim2, dim3          # the reference's naming of shape[2], shape[3] (spatial.py:113)
        area = height * width
        target_area = np.random.uniform(*self.scale, B * 10) * area
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        aspect_ratio = np.exp(np.random.uniform(*log_ratio, B * 10))
        w = np.round(np.sqrt(target_area * aspect_ratio))
        h = np.round(np.sqrt(target_area / aspect_ratio))
        keep = (0 < w) * (w <= width) * (0 < h) * (h <= height)
        w, h = w[keep], h[keep]
        if len(w) > B:
            pick = np.random.choice(len(w), B, replace=False)
            w, h = w[pick], h[pick]
        n = len(w)
        bias_w = np.random.randint(w - width, width - w + 1) / width
        bias_h = np.random.randint(h - height, height - h + 1) / height
        P[:, 0] = 1.0
        P[:, 1] = 1.0
        P[:n, 0] = torch.tensor(w / width)
        P[:n, 1] = torch.tensor(h / height)
        P[:n, 2] = torch.tensor(bias_w)
        P[:n, 3] = torch.tensor(bias_h)
        P[:, 4] = torch.bernoulli(torch.ones(B) * 0.5) * 2 - 1
        P[:, 5] = torch.bernoulli(torch.full((B,), self.p_jitter))
        contrast_first = bool(np.random.rand() > 0.5)

        def draw_contrast():
            P[:, 6] = torch.empty(B, 1, 1, 1).uniform_(*self.r_c).view(B) if self.r_c else 1.0

        def draw_hsv():
            f_h, f_s, f_v = torch.zeros(B, 1, 1), torch.ones(B, 1, 1), torch.ones(B, 1, 1)
            if self.r_h:
                f_h.uniform_(*self.r_h)
            if self.r_s:
                f_s.uniform_(*self.r_s)
            if self.r_v:
                f_v.uniform_(*self.r_v)
            P[:, 7], P[:, 8], P[:, 9] = f_h.view(B), f_s.view(B), f_v.view(B)

        if contrast_first:
            draw_contrast(); draw_hsv()
        else:
            draw_hsv(); draw_contrast()
        P[:, 10] = torch.bernoulli(torch.full((B,), self.p_gray))
        sigma = None
        if self.p_blur is not None:
            P[:, 11] = torch.bernoulli(torch.full((B,), self.p_blur))
            sigma = float(np.random.uniform(*self.sigma_range))
        P[:, 15] = float(contrast_first)    # also carried in the block: a captured hipGraph reads it from there
        if self.p_cutout is not None:        # RandomApply mask, then CutOut's two randint draws (spatial.py:166-170)
            P[:, 12] = torch.bernoulli(torch.full((B,), self.p_cutout))
            P[:, 13] = torch.randint(dim2, (B, 1)).view(B).float()
            P[:, 14] = torch.randint(dim3, (B, 1)).view(B).float()
        return P, contrast_first, sigma

    @staticmethod
    def blur_kernel(H, sigma):
        """GaussianBlur's kernel size (augment/__init__.py:69-71) and kornia's normalised 1-D Gaussian."""
        radius = int((H // 10) / 2)
        xs = torch.arange(2 * radius + 1, dtype=torch.float32) - radius
        g = torch.exp(-xs.pow(2) / (2 * sigma ** 2))
        return radius, g / g.sum()

    def apply(self, inputs, P, contrast_first, sigma=None, out=None):
        """Deterministic device part."""
        Pd = upload(P, inputs.device)      # (B,12) parameter block (asynchronous pinned upload, contrad_amd/hostio.py)
        if inputs.requires_grad and torch.is_grad_enabled():
            blur = None
            if sigma is not None:
                radius, g = self.blur_kernel(inputs.shape[2], sigma)
                if radius > 0:
                    blur = (radius, g.to(inputs.device))
            if out is not None:
                raise RuntimeError('augmentation: out= is a forward-only option')
            return _SimCLRFn.apply(inputs.contiguous().float(), Pd, contrast_first, self.r_c is not None, blur,
                                   self.cutout_length if self.p_cutout is not None else None)
        x = inputs.detach().contiguous().float()
        radius = 0
        if sigma is not None:
            radius, g = self.blur_kernel(x.shape[2], sigma)
        # ``out``: the LAST stage writes there (a caller's slice of a larger batch buffer: no concatenation afterwards)
        res = ops.simclr_augment(x, Pd, contrast_first, self.r_c is not None, out=None if radius > 0 else out)
        if radius > 0:
            res = ops.gaussian_blur_masked(res, Pd, g.to(x.device), radius, out=out)
        if self.p_cutout is not None:
            ops.cutout_masked_(res, Pd, self.cutout_length)
        return res

    def forward(self, inputs, out=None):
        if not inputs.is_cuda:
            raise RuntimeError('contrad_amd augmentation runs on the MI355X HIP path only (no CPU fallback)')
        B, _, d2, d3 = inputs.shape
        P, contrast_first, sigma = self.sample(B, d2, d3)
        return self.apply(inputs, P, contrast_first, sigma, out=out)


def _kwargs_from_bindings():
    cj = get_bindings('ColorJitterLayer')
    rc = get_bindings('RandomResizeCropLayer')
    return dict(scale=rc['scale'], ratio=rc.get('ratio', (3. / 4., 4. / 3.)),
                brightness=cj['brightness'], contrast=cj['contrast'], saturation=cj['saturation'], hue=cj['hue'])


def simclr():
    return SimCLRAugment(**_kwargs_from_bindings())


def simclr_hq():
    gb = get_bindings('GaussianBlur')
    return SimCLRAugment(p_blur=0.5, sigma_range=gb['sigma_range'], **_kwargs_from_bindings())


def simclr_hq_cutout():
    gb = get_bindings('GaussianBlur')
    return SimCLRAugment(p_blur=0.5, sigma_range=gb['sigma_range'], p_cutout=0.5,
                         cutout_length=get_bindings('CutOut')['length'], **_kwargs_from_bindings())


class NoAugment(nn.Module):
    """augment/__init__.py:31-37: the identity (``--aug=none``)."""

    def forward(self, input):
        return input


class _HfrtFn(torch.autograd.Function):
    """Flip + integer-shift index map with reflection; the backward is its adjoint gather (csrc/baseline_aug.hip)."""

    @staticmethod
    def forward(ctx, x, Pd, max_pixels):
        ctx.save_for_backward(Pd)
        ctx.max_pixels = max_pixels
        return ops.hfrt(x, Pd, max_pixels)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        Pd, = ctx.saved_tensors
        return ops.hfrt(g.contiguous(), Pd, ctx.max_pixels, adjoint=True), None, None


class _FlipShift(nn.Module):
    """What hfrt and hflip share: the device part of a flip + whole-pixel shift (ops.hfrt) with ``self.max_pixels``;
    subclasses draw the parameter rows (``sample``) and say which image sizes they take (``check_size``)."""

    max_pixels = 0

    def check_size(self, H, W):
        raise NotImplementedError

    def apply(self, inputs, P):
        """Deterministic device part."""
        self.check_size(inputs.shape[2], inputs.shape[3])
        Pd = upload(P, inputs.device)
        if inputs.requires_grad and torch.is_grad_enabled():
            return _HfrtFn.apply(inputs.contiguous().float(), Pd, self.max_pixels)
        return ops.hfrt(inputs.detach().contiguous().float(), Pd, self.max_pixels)

    def forward(self, input):
        if not input.is_cuda:
            raise RuntimeError('contrad_amd augmentation runs on the MI355X HIP path only (no CPU fallback)')
        return self.apply(input, self.sample(input.shape[0]))


class HorizontalFlipRandomCrop(_FlipShift):
    """augment/spatial.py:14-40 (``--aug=hfrt``): random horizontal flip and a shift by whole pixels in [-max_pixels,
    max_pixels] on both axes, nearest-neighbour sampling with reflection padding.  The reference's normalised shift
    k / (width / 2) is exactly k pixels when the images are width x width, so the layer is an index map; other sizes and
    padding modes are refused."""

    def __init__(self, max_pixels=None, width=None, padding_mode=None):
        super().__init__()
        b = get_bindings('HorizontalFlipRandomCrop') if None in (max_pixels, width, padding_mode) else {}
        self.max_pixels = int(b['max_pixels'] if max_pixels is None else max_pixels)
        self.width = int(b['width'] if width is None else width)
        self.padding_mode = b['padding_mode'] if padding_mode is None else padding_mode
        if self.padding_mode != 'reflection':
            raise NotImplementedError("HorizontalFlipRandomCrop: padding_mode '%s' (only 'reflection', the reference's "
                                      "configured value, is an index map)" % self.padding_mode)
        if not 0 <= self.max_pixels < self.width:
            raise ValueError('HorizontalFlipRandomCrop: max_pixels must be in [0, width)')

    def sample(self, B):
        """(B, HFRT_NPARAM) CPU block {sign, kx, ky, 0} from the torch CPU generator in the reference's order: the flip
        signs, then the (B, 2) shifts, column 0 = x (spatial.py:30-32)."""
        P = torch.zeros(B, ops.HFRT_NPARAM)
        P[:, 0] = torch.bernoulli(torch.ones(B) * 0.5) * 2 - 1
        P[:, 1:3] = torch.randint(-self.max_pixels, self.max_pixels + 1, (B, 2)).float()
        return P

    def check_size(self, H, W):
        if H != self.width or W != self.width:
            raise RuntimeError('HorizontalFlipRandomCrop(width=%d) got %dx%d images: the shifts are whole pixels only '
                               'on width x width images' % (self.width, H, W))


class HorizontalFlipLayer(_FlipShift):
    """augment/spatial.py:70-93 (``--aug=hflip``): the flip alone -- the same kernel with max_pixels = 0.  Draws the flip
    signs only."""

    def sample(self, B):
        P = torch.zeros(B, ops.HFRT_NPARAM)
        P[:, 0] = torch.bernoulli(torch.ones(B) * 0.5) * 2 - 1
        return P

    def check_size(self, H, W):
        if H != W:
            raise RuntimeError('HorizontalFlipLayer: square images (the hfrt kernel with max_pixels = 0)')


class _DiffAugFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Pd, bits):
        ctx.save_for_backward(Pd)
        ctx.bits = bits
        return ops.diffaug(x, Pd, bits)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        Pd, = ctx.saved_tensors
        return ops.diffaug(g.contiguous(), Pd, ctx.bits, backward=True), None, None


class DiffAugLayer(nn.Module):
    """augment/__init__.py:136-142 + third_party/diffaug.py: DiffAugment with a policy out of color, translation, cutout
    (in this order), forward and backward in one fused launch each on CIFAR-sized images."""

    def __init__(self, policy=""):
        super().__init__()
        self.policy = policy
        self.bits = ops.diffaug_policy_bits(policy) if policy else 0

    def sample(self, B, dim2, dim3):
        """(B, DIFFAUG_NPARAM) CPU block {b, s, c, tx, ty, ox, oy, 0} from the torch CPU generator in the reference's order
        (diffaug.py:24-60): three float32 rand(B,1,1,1) for the colour stage, randint tx, ty, randint ox, oy; stages
        outside the policy draw nothing."""
        P = torch.zeros(B, ops.DIFFAUG_NPARAM)
        if self.bits & 1:
            P[:, 0] = (torch.rand(B, 1, 1, 1) - 0.5).view(B)
            P[:, 1] = (torch.rand(B, 1, 1, 1) * 2).view(B)
            P[:, 2] = (torch.rand(B, 1, 1, 1) + 0.5).view(B)
        if self.bits & 2:
            sx, sy = int(dim2 * 0.125 + 0.5), int(dim3 * 0.125 + 0.5)
            P[:, 3] = torch.randint(-sx, sx + 1, size=[B, 1, 1]).view(B).float()
            P[:, 4] = torch.randint(-sy, sy + 1, size=[B, 1, 1]).view(B).float()
        if self.bits & 4:
            cx, cy = int(dim2 * 0.5 + 0.5), int(dim3 * 0.5 + 0.5)
            P[:, 5] = torch.randint(0, dim2 + (1 - cx % 2), size=[B, 1, 1]).view(B).float()
            P[:, 6] = torch.randint(0, dim3 + (1 - cy % 2), size=[B, 1, 1]).view(B).float()
        return P

    def apply(self, inputs, P):
        """Deterministic device part."""
        if not self.bits:
            return inputs
        Pd = upload(P, inputs.device)
        if inputs.requires_grad and torch.is_grad_enabled():
            return _DiffAugFn.apply(inputs.contiguous().float(), Pd, self.bits)
        return ops.diffaug(inputs.detach().contiguous().float(), Pd, self.bits)

    def forward(self, inputs):
        if not self.bits:                     # DiffAugment(policy=''): the identity
            return inputs
        if not inputs.is_cuda:
            raise RuntimeError('contrad_amd augmentation runs on the MI355X HIP path only (no CPU fallback)')
        B, _, d2, d3 = inputs.shape
        return self.apply(inputs, self.sample(B, d2, d3))


def diffaug(policy='color,cutout'):
    return DiffAugLayer(policy=policy)                   # augment/__init__.py:144-145: the factory's policy is color,cutout


@configurable('augment')
def get_augment(mode='none', diffaug_policy=None, **kwargs):
    """Same entry point as augment.get_augment (augment/__init__.py:13-28): the SimCLR pipelines of the ContraD hot path and
    the augmentations of the baseline modes (none, hflip, hfrt, diffaug).

    ``diffaug`` is switched on by the configuration: it needs the binding ``augment.diffaug_policy`` (configs/gan/diffaug/
    c10_diffaug.gin sets the reference's ``"color,cutout"``); without it the mode raises, as every mode outside the
    configured path does."""
    mapping = {'simclr': simclr, 'simclr_hq': simclr_hq, 'simclr_hq_cutout': simclr_hq_cutout, 'none': NoAugment,
               'hflip': HorizontalFlipLayer, 'hfrt': HorizontalFlipRandomCrop}
    if mode == 'diffaug':
        if diffaug_policy is None:
            raise NotImplementedError("augmentation mode 'diffaug' needs the gin binding augment.diffaug_policy "
                                      "(configs/gan/diffaug/c10_diffaug.gin binds \"color,cutout\")")
        return diffaug(diffaug_policy)
    if mode not in mapping:
        raise NotImplementedError("augmentation mode '%s' is not implemented on this path (SURVEY.md 2 row 6)" % mode)
    return mapping[mode]()
