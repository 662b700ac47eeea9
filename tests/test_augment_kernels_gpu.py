"""GPU parity of the SimCLR augmentation kernels (csrc/augment.hip) against float64 (tests/aug_ref64.py: plain float64
torch, none of this project's kernels), through the C ABI so that every operand lives in guard storage.  Each case names
the launch form it is meant to reach; tests/test_aug_sg2_ref64_cpu.py restates the dispatch rules and fails if a form
has no case or a case's declared form is wrong.  Checked on the whole tensor, as tests/test_dstep_kernels_gpu.py does:
  * max-norm error max|e| / max|ref| below the 1e-3 contract, and both it and the rel-L2 error below a per-family bound
    (FAMILY_TOL, about 5x the worst observed on an MI355X), recorded through ``margin``;
  * outputs, inputs and workspaces sit inside NaN-filled storage with spare floats on both sides (whole multiples of 4
    floats, so operands stay 16-byte aligned); every output sentinel must still be NaN afterwards, and an over-read
    shows up as a NaN in the result;
  * the parts that are exact (copied-through samples, the flip, the identity crop at power-of-two sizes, cutout) are
    compared bitwise.
The backward has one kink, the contrast clamp (HSV is straight-through; crop, gray and blur are linear).  Elements whose
float64 pre-clamp value lies within 1e-5 of 0 or 1 (the set K) may land on either side of the clamp in fp32; for each of
them the reference takes the side that matches the kernel (aug_ref64.resolve_kinks), every other element keeps the
float64 mask, and the whole gradient is then held to the family bounds with no exclusion.  |K| must stay below 0.5 % of
the output.  (A case at 96 x 96 has two such elements; one of them flips on an MI355X and moves its four source pixels
by up to 3.9 against a gradient of max 7.4.)
"""
import math

import numpy as np
import pytest
import torch

import aug_ref64 as A
from contrad_amd import ops
from contrad_amd._lib import lib
from oracle import contrad_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
NP = 16

FAMILY_TOL = {                  # family: (max-norm, rel-L2)      observed worst (max-norm, rel-L2)
    'aug_fwd': (1.8e-4, 1e-5),                  # 3.7e-5, 2.0e-6
    'aug_bwd': (4e-5, 1.9e-5),                  # 8.2e-6, 3.8e-6
    'blur_fwd': (1.3e-6, 4.7e-7),               # 2.7e-7, 9.4e-8
    'blur_bwd': (3.1e-7, 1.6e-7),               # 6.2e-8, 3.3e-8
}


def errors(out, ref):
    out, ref = out.to(torch.float64), ref.to(torch.float64)
    e = out - ref
    return (e.abs().max().item() / max(ref.abs().max().item(), 1e-30),
            e.norm().item() / max(ref.norm().item(), 1e-30))


def check(margin, family, what, out, ref):
    assert torch.isfinite(out).all(), (family, what, 'non-finite output')
    emax, el2 = errors(out, ref)
    assert emax < CONTRACT and el2 < CONTRACT, (family, what, emax, el2)
    tmax, tl2 = FAMILY_TOL[family]
    margin('aug %s max-norm' % family, emax, tmax)
    margin('aug %s rel-L2' % family, el2, tl2)


def _r4(n):
    return (n + 3) // 4 * 4


class Guard(object):
    """``shape`` inside NaN-filled storage with ``pad`` spare floats on both sides (a multiple of 4)."""

    def __init__(self, shape, pad=None, fill=None):
        n = math.prod(shape)
        per = math.prod(shape[1:]) if len(shape) > 1 else 4
        self.pad = _r4(per) + 4 if pad is None else pad
        assert self.pad % 4 == 0
        self.n = n
        self.buf = torch.full((n + 2 * self.pad,), NAN, device=DEV)
        self.view = self.buf[self.pad:self.pad + n].view(*shape)
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.pad]).all()) and bool(torch.isnan(self.buf[self.pad + self.n:]).all())


def P_(t):
    return ops._p(t)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def fwd_form(H, W):
    return 'lds' if 3 * H * W * 4 <= 64 * 1024 else 'multipass'


def bwd_form(H, W):
    return 'lds' if (7 * H * W + H * H + W * W) * 4 <= 64 * 1024 else 'multipass'


def nparts(H, W):
    return -(-H * W // 4096)


# ======================================================================================================================
# parameters and images
# ======================================================================================================================
def make_params(B, H, W, seed, cf_mix=True):
    """A mixed batch: sample 0 the identity crop copied through, 1 its flip, 2 / 3 crops touching the left / right
    border, 4 / 5 the top / bottom border, 6 the sampler's smallest crop (area 0.08), the rest the sampler's own draws
    (scale 0.08 .. 1), 8 of them mirrored (negative theta00), 9 a zoom-out reaching past the border; 10 and 11 the
    identity crop, jittered and not grayed, contrast first (column 15 = 1, f = 1.5) and HSV first (column 15 = 0), with
    a hue shift of -0.2 (across the wrap for hue 0) and f_s / f_v above 1; flips, jitter, gray and the column-15 order
    mixed elsewhere; f_s / f_v up to 1.8 (saturating values)."""
    assert B >= 12
    g = gen(seed)
    P = torch.zeros(B, NP)
    P[:, 0] = 1.0; P[:, 1] = 1.0
    np.random.seed(seed)
    th = O.sample_resized_crop_theta(B, H, W, (0.08, 1.0), (3. / 4., 4. / 3.))
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = th[:, 0, 0], th[:, 1, 1], th[:, 0, 2], th[:, 1, 2]
    P[0, :4] = torch.tensor([1., 1., 0., 0.])
    P[1, :4] = torch.tensor([1., 1., 0., 0.])
    sx, sy = round(0.6 * W) / W, round(0.5 * H) / H
    if B > 2: P[2, 0], P[2, 2] = sx, sx - 1          # left border: the first column samples column 0
    if B > 3: P[3, 0], P[3, 2] = sx, 1 - sx          # right border
    if B > 4: P[4, 1], P[4, 3] = sy, sy - 1          # top
    if B > 5: P[5, 1], P[5, 3] = sy, 1 - sy          # bottom
    if B > 6:                                        # the smallest crop the sampler draws: area 0.08, square
        wq, hq = round(math.sqrt(0.08) * W), round(math.sqrt(0.08) * H)
        P[6, 0], P[6, 1] = wq / W, hq / H
        P[6, 2], P[6, 3] = (W - wq) / W, (hq - H) / H      # (a corner: touches the right and the top borders)
    if B > 8: P[8, 0] = -P[8, 0]                     # a mirrored crop (negative scale)
    if B > 9: P[9, 0], P[9, 1] = 1.25, 1.25          # zoom-out: reflected coordinates (the forward accepts any theta)
    if B > 9: P[9, 3] = -0.5                         # ... shifted past the top border
    flip = torch.ones(B)
    flip[1::2] = -1
    if B > 7: flip[7] = -1
    P[:, 4] = flip
    jit = (torch.rand(B, generator=g) < 0.75).float()
    jit[:2] = 0
    if B > 2: jit[2:7] = 1
    P[:, 5] = jit
    P[:, 6] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    P[:, 7] = torch.empty(B).uniform_(-0.2, 0.2, generator=g)
    P[:, 8] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    P[:, 9] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    gray = (torch.rand(B, generator=g) < 0.3).float()
    gray[:2] = 0
    if B > 4: gray[4] = 1
    P[:, 10] = gray
    P[:, 15] = (torch.arange(B) % 3 == 0).float() if cf_mix else 0.
    # 10 / 11: the planted HSV-edge colours reach the HSV stage unblended (identity crop), in either op order; with
    # f = 1.5 the contrast-first sample clamps black / white / pure R, G, B back to exact 0 / 1 channels
    P[10:12, :4] = torch.tensor([1., 1., 0., 0.])
    P[10:12, 5], P[10:12, 10] = 1., 0.
    P[10, 15], P[11, 15] = 1., 0.
    P[10, 6] = 1.5
    P[10:12, 7], P[10:12, 8], P[10:12, 9] = -0.2, 1.6, 1.7
    return P


SPECIAL = torch.tensor([[0., 0., 0.], [.5, .5, .5], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.], [1., 1., 1.]])


def make_images(B, H, W, seed, special):
    """Uniform images; where ``special`` (B,) is set, rows 1..3 hold 3 x 3 constant patches of black, gray, pure red /
    green / blue and white (Cmax = 0, atan2(0, 0), hue 0 / 1/3 / 2/3) at columns 1 + 4k: any bilinear weights that stay
    inside a patch give its colour back with r = g = b or the zero channels exactly zero."""
    x = torch.rand(B, 3, H, W, generator=gen(seed + 1))
    for b in range(B):
        if special[b]:
            for k in range(SPECIAL.shape[0]):
                x[b, :, 1:4, 1 + 4 * k:4 + 4 * k] = SPECIAL[k].view(3, 1, 1)
    x[1] = x[0]                                      # (sample 1 is sample 0 flipped)
    return x


def case_inputs(case):
    """(P, x, gout) of an AUG_CASES entry.  Without a contrast factor the exact 0 / 1 patches sit on the clamp (the set
    K of the backward), so they are planted in the samples that skip jitter and in sample 10 only."""
    B, H, W, cf, hc, _ = case
    P = make_params(B, H, W, seed=H * 131 + W + cf * 7 + hc)
    special = torch.ones(B, dtype=torch.bool) if hc else (P[:, 5] == 0)
    special[10] = True
    x = make_images(B, H, W, H + W, special)
    gout = torch.randn(B, 3, H, W, generator=gen(H * W))
    return P, x, gout


# (B, H, W, contrast_first, has_contrast, what)
AUG_CASES = [
    (12, 32, 32, -1, 1, 'CIFAR size: column 15 mixed'),
    (12, 32, 32, 0, 1, 'HSV first'),
    (12, 32, 32, 1, 0, 'no contrast factor: the clamp alone'),
    (12, 42, 42, -1, 1, 'the largest LDS backward'),
    (12, 43, 43, -1, 1, 'the smallest multi-pass backward'),
    (12, 43, 43, 1, 1, 'contrast first, multi-pass backward'),
    (12, 73, 73, -1, 1, 'the largest LDS forward'),
    (12, 74, 74, 0, 1, 'the smallest multi-pass forward: nparts = 2, ragged'),
    (12, 74, 74, 1, 0, 'multi-pass, no contrast factor'),
    (12, 96, 96, -1, 1, 'nparts = 3, ragged'),
    (12, 96, 96, 1, 1, 'contrast first'),
    (12, 512, 512, -1, 1, 'AFHQ size: nparts = 64'),
    (12, 40, 100, -1, 1, 'non-square 40 x 100: forward in LDS, backward multi-pass'),
    (12, 100, 40, 0, 1, 'non-square 100 x 40'),
]


def case_forms(case):
    B, H, W = case[:3]
    return fwd_form(H, W), bwd_form(H, W)


def _aug_fwd(x, P, H, W, cf, hc):
    B = x.shape[0]
    gx = Guard(tuple(x.shape), fill=x)
    gp = Guard((B, NP), fill=P)
    gy = Guard(tuple(x.shape))
    nbytes = lib().raw('contrad_simclr_workspace_bytes')(B, H, W)
    gw = Guard(((nbytes + 3) // 4,), pad=16)
    lib().call('contrad_simclr_augment', P_(gx.view), P_(gy.view), P_(gp.view), B, H, W, cf, hc, P_(gw.view), nbytes,
               ops._stream())
    torch.cuda.synchronize()
    assert gy.intact() and gw.intact() and gx.intact() and gp.intact()
    return gy.view


def _aug_bwd(x, P, gout, H, W, cf, hc):
    B = x.shape[0]
    gx = Guard(tuple(x.shape), fill=x)
    gp = Guard((B, NP), fill=P)
    gg = Guard(tuple(x.shape), fill=gout)
    gi = Guard(tuple(x.shape))
    nbytes = lib().raw('contrad_simclr_augment_bwd_workspace_bytes')(B, H, W)
    gw = Guard(((nbytes + 3) // 4,), pad=16)
    lib().call('contrad_simclr_augment_bwd', P_(gx.view), P_(gp.view), P_(gg.view), P_(gi.view), B, H, W, cf, hc,
               P_(gw.view), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert gi.intact() and gw.intact()
    return gi.view


def _pow2(n):
    return n & (n - 1) == 0


@pytest.mark.parametrize('case', AUG_CASES, ids=lambda c: '%dx%d-cf%d-c%d' % c[1:5])
def test_simclr_forward(margin, case):
    B, H, W, cf, hc, _ = case
    P, x, _ = case_inputs(case)
    xd, Pd = x.to(DEV), P.to(DEV)
    y = _aug_fwd(xd, Pd, H, W, cf, hc)
    ref = A.simclr(xd, Pd, cf, hc)
    what = '%dx%d cf=%d contrast=%d %s' % (H, W, cf, hc, fwd_form(H, W))
    check(margin, 'aug_fwd', what, y, ref)
    # exact parts: sample 1 is sample 0 flipped (no colour stage): a column permutation at every size
    assert torch.equal(y[1], y[0].flip(-1)), what
    if _pow2(H) and _pow2(W):                      # the identity crop is exact where the grid arithmetic is
        assert torch.equal(y[0], xd[0]) and torch.equal(y[1], xd[0].flip(-1)), what


@pytest.mark.parametrize('case', AUG_CASES, ids=lambda c: '%dx%d-cf%d-c%d' % c[1:5])
def test_simclr_backward(margin, case):
    B, H, W, cf, hc, _ = case
    P, x, gout = case_inputs(case)
    xd, Pd, gd = x.to(DEV), P.to(DEV), gout.to(DEV)
    gi = _aug_bwd(xd, Pd, gd, H, W, cf, hc)
    ref, nK, flips = A.resolve_kinks(xd, Pd, gd, cf, hc, gi)
    assert nK < 0.005 * x.numel(), nK
    what = '%dx%d cf=%d contrast=%d %s |K|=%d flipped %d' % (H, W, cf, hc, bwd_form(H, W), nK, flips)
    check(margin, 'aug_bwd', what, gi, ref)
    if _pow2(H) and _pow2(W):                      # identity crop, no colour stage: the gradient is copied / flipped
        assert torch.equal(gi[0], gd[0]) and torch.equal(gi[1], gd[1].flip(-1)), what


def test_column_15_is_per_sample(margin):
    """contrast_first = -1 reads the op order per sample: each sample equals a launch with its own fixed order."""
    B, H, W = 12, 32, 32
    P = make_params(B, H, W, seed=77)
    x = make_images(B, H, W, 78, torch.ones(B, dtype=torch.bool)).to(DEV)
    Pd = P.to(DEV)
    mixed = _aug_fwd(x, Pd, H, W, -1, 1)
    first = P[:, 15] != 0
    assert 0 < int(first.sum()) < B
    y1, y0 = _aug_fwd(x, Pd, H, W, 1, 1), _aug_fwd(x, Pd, H, W, 0, 1)
    for b in range(B):
        assert torch.equal(mixed[b], (y1 if first[b] else y0)[b]), b


@pytest.mark.parametrize('HW', [(32, 32), (96, 96)], ids=lambda s: '%dx%d' % s)
def test_clamp_boundary_passes_gradient(margin, HW):
    """Inputs exactly 0 or 1, identity crop, jitter on, no contrast factor: the pre-clamp values sit on the clamp's
    boundary, where torch.clamp passes the gradient.  Compared unmasked."""
    H, W = HW
    B = 4
    P = torch.zeros(B, NP)
    P[:, 0] = 1.; P[:, 1] = 1.; P[:, 4] = 1.; P[:, 5] = 1.; P[:, 6] = 1.; P[:, 8] = 1.; P[:, 9] = 1.
    P[1, 4] = -1.
    x = (torch.rand(B, 3, H, W, generator=gen(5)) < 0.5).float().to(DEV)
    gout = torch.randn(B, 3, H, W, generator=gen(6)).to(DEV)
    Pd = P.to(DEV)
    gi = _aug_bwd(x, Pd, gout, H, W, 1, 0)
    ref = A.simclr_bwd(x, Pd, gout, 1, 0)
    check(margin, 'aug_bwd', 'boundary %dx%d' % HW, gi, ref)
    if _pow2(H) and _pow2(W):
        assert torch.equal(gi[0], gout[0]) and torch.equal(gi[1], gout[1].flip(-1))


# ======================================================================================================================
# blur and its adjoint
# ======================================================================================================================
# (B, H, W, radius, what)
BLUR_CASES = [
    (5, 33, 31, 0, 'radius 0: one tap'),
    (6, 100, 70, 4, 'radius 4, ragged 64 x 64 tiles'),
    (4, 130, 77, 25, 'radius 25 (AFHQ 512: H // 10 // 2), three row tiles'),
    (4, 70, 45, 44, 'radius W - 1: the limit'),
    (3, 512, 512, 25, 'AFHQ size'),
]


@pytest.mark.parametrize('case', BLUR_CASES, ids=lambda c: '%dx%d-r%d' % c[1:4])
def test_blur(margin, case):
    B, H, W, R, _ = case
    P = torch.zeros(B, NP)
    P[:, 11] = torch.tensor([1., 0.] * B)[:B]
    P[-1, 11] = 1.
    k1 = O.gaussian_kernel1d(2 * R + 1, 0.7 + 0.05 * R)
    x = torch.rand(B, 3, H, W, generator=gen(R + H))
    gout = torch.randn(B, 3, H, W, generator=gen(R + W))
    xd, Pd, kd, gd = x.to(DEV), P.to(DEV), k1.to(DEV), gout.to(DEV)
    gx, gp, gk = Guard(x.shape, fill=xd), Guard((B, NP), fill=Pd), Guard((2 * R + 1,), pad=4, fill=kd)
    gt, gy = Guard(x.shape), Guard(x.shape)
    lib().call('contrad_gaussian_blur_masked', P_(gx.view), P_(gt.view), P_(gy.view), P_(gp.view), P_(gk.view), B, H, W,
               R, ops._stream())
    gg = Guard(x.shape, fill=gd)
    gt2, gi = Guard(x.shape), Guard(x.shape)
    lib().call('contrad_gaussian_blur_masked_bwd', P_(gg.view), P_(gt2.view), P_(gi.view), P_(gp.view), P_(gk.view), B,
               H, W, R, ops._stream())
    torch.cuda.synchronize()
    assert gy.intact() and gt.intact() and gi.intact() and gt2.intact()
    what = '%dx%d R=%d' % (H, W, R)
    check(margin, 'blur_fwd', what, gy.view, A.gaussian_blur(xd, Pd, kd))
    check(margin, 'blur_bwd', what, gi.view, A.gaussian_blur_bwd(gd, Pd, kd))
    for b in range(B):
        if P[b, 11] == 0:                          # RandomApply select: copied through, bitwise
            assert torch.equal(gy.view[b], xd[b]) and torch.equal(gi.view[b], gd[b]), (what, b)


# ======================================================================================================================
# cutout
# ======================================================================================================================
# (B, H, W, length)
CUTOUT_CASES = [(6, 32, 32, 1), (6, 64, 48, 15), (4, 512, 512, 15)]


@pytest.mark.parametrize('case', CUTOUT_CASES, ids=lambda c: '%dx%d-l%d' % c[1:4])
def test_cutout(case):
    B, H, W, L = case
    P = torch.zeros(B, NP)
    P[:, 12] = torch.tensor([1., 1., 1., 0., 1., 1.])[:B]
    cen = [(0, 0), (H - 1, W - 1), (0, W - 1), (5, 5), (H - 1, 0), (H // 2, W // 3)]
    for b in range(B):
        P[b, 13], P[b, 14] = cen[b]
    x = torch.rand(B, 3, H, W, generator=gen(H + L)).to(DEV)
    Pd = P.to(DEV)
    gy, gp = Guard(x.shape, fill=x), Guard((B, NP), fill=Pd)
    lib().call('contrad_cutout_masked', P_(gy.view), P_(gp.view), B, H, W, L, ops._stream())
    torch.cuda.synchronize()
    assert gy.intact()
    assert torch.equal(gy.view, A.cutout(x, Pd, L).float())
