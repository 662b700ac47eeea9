"""Parity past the 2 GiB and 4 GiB marks: the conv engine and the kernels that see the same tensors, with operands whose
span in bytes exceeds 2^32 while their element count stays below the library's 2^31 limit.

An operand is made FAR cheaply the way tests/test_conv_paths_gpu.py makes its guard bands: a narrow channel slice of a
buffer with a large leading dimension (spare columns hold 1e3 for inputs and NaN for outputs; a spare image -- at most
256 MiB of it -- sits on each side; after the call every sentinel of the conv operands, inputs included, and every output
sentinel of the other kernels is checked).  A base pointer computed in int, a ``* 4`` applied before the widening cast, or a
block-relative offset that reaches bit 31 and reads as zero lands on other data here and shows as an error against float64.

What the checks rest on: a float64 reference over the WHOLE output, never the code under test and never a few probe
images.
  * Where the float64 operation is expensive (convs, FIR filters, the RGB convs) image n of every input is
    pattern[n % P], P = 7, so ref[n] = ref64[n % P] needs float64 work for P compact images only; the broadcast is
    compared with the whole output in chunks.  P does not divide the number of images in 2^31 or 2^32 bytes of any operand
    (tests/test_far_offsets_cpu.py asserts it): an access that wraps by exactly that distance lands on other data.
    Reductions over the batch (weight gradient, bias gradient) use x and gy periodic with the same P: the reference is
    sum_j count_j * dw64(pattern_j), and a read shifted by anything but a multiple of P pairs the wrong x with gy.
  * Where the float64 operation is cheap (element-wise ops, the row-wise statistics, BatchNorm, the linear head) the data is
    random over the whole tensor and the plain float64 torch expression is evaluated in chunks: stronger than a period, as
    no shift at all goes unseen.
Bounds: the 1e-3 contract, and below it the per-family bound the project already asserts for the same kernel (FAMILY_TOL
of test_conv_paths_gpu.py / test_sg2_ops_kernels_gpu.py, the tables of test_dstep_kernels_gpu.py / test_linhead_gpu.py),
recorded through ``margin``.  Only reductions over 10^3 - 10^6 images may carry a bound of their own (FAR_REDUCTION_TOL:
5 x the error observed against float64 on an MI355X, bound and observation side by side); forward, data gradient,
element-wise ops and blurs get no allowance.

Out of scope here: the SimCLR / hfrt / DiffAugment kernels (a far batch needs thousands of 512^2 images and their guards
already cap C * H * W), knn_select, Adam.

Each test holds at most 24 GiB of device memory and releases it before the next; nothing depends on how much is free."""
import ctypes
import math

import pytest
import torch

import conv_ref64 as R
import dstep_ref64 as D
import linhead_ref64 as LH
import sg2_ref64 as S
from contrad_amd import ops
from contrad_amd._lib import lib

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
P = 7                                   # period of the image patterns
SPARE_MAX = 1 << 26                     # floats of the spare band either side of an operand: one image, 256 MiB at most
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
SLOPE = f32(0.2)
GAIN = f32(math.sqrt(2.0))


def _tables():
    """The bound tables of the modules that test the same kernels at small shapes (loaded for their tables only)."""
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for name in ('test_conv_paths_gpu', 'test_sg2_ops_kernels_gpu', 'test_dstep_kernels_gpu', 'test_linhead_gpu'):
        spec = importlib.util.spec_from_file_location('_far_' + name, os.path.join(here, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out[name] = mod.FAMILY_TOL
    return out


_T = _tables()
CONV_TOL, SG2_TOL, DSTEP_TOL, LINHEAD_TOL = (_T['test_conv_paths_gpu'], _T['test_sg2_ops_kernels_gpu'],
                                             _T['test_dstep_kernels_gpu'], _T['test_linhead_gpu'])

# Reductions over the far batch whose error against float64 exceeds the small-shape bound for numerical reasons alone
# (10^3 - 10^6 images summed in fp32): bound = 5 x the observed error on an MI355X.
# (Listed: the reductions that exceeded their family bound in at least one norm; a norm that met the family bound keeps it,
# as the rule for these bounds says.  KNOWINGLY TIGHT, 0.90 - 0.99 of the family bound: rel-L2 of the 2100x32x32x16-512 dw,
# max-norm of the rgb_wgrad N1400 dw, of the 3650x96x96 dbias and of the 140000 dbias, rel-L2 of the 66000x4x4 dbias.  The sums
# are fixed-order, so the figures repeat; if a compiler or a harmless reordering moves one of them past its family bound, it
# becomes a row of this table at 5 x the new observation -- that is a numerical event, not an addressing one.)
FAR_REDUCTION_TOL = {           # name: (max-norm, rel-L2)                                       observed (max-norm, rel-L2)
    'p2-m2-split-32868x8x8x512-16-k3s1p1 dw':            (2.7e-04, 1.2e-04),      # 5.34e-05, 2.39e-05
    'p2-m2-split-32868x8x8x512-16-k3s1p1 dbias':         (5.7e-05, 5.1e-05),      # 1.13e-05, 1.02e-05
    'p3-m2-split-262160x2x2x128-8-k3s1p1 dw':            (1.1e-04, 4.8e-05),      # 2.10e-05, 9.58e-06
    'p2-m2-split-140000x1x1x1024-512-k1s1p0 dw':         (1.2e-04, 6.1e-05),      # 2.26e-05, 1.21e-05
    'p2-m2-split-140000x1x1x1024-512-k1s1p0 dbias':      (3.0e-06, 7.8e-06),      # 2.70e-06, 1.55e-06
    'p0-m2-split-1048584x1x1x16-1-k1s1p0 dw':            (2.3e-05, 1.5e-05),      # 4.49e-06, 2.94e-06
    'p2-m2-split-66000x4x4x32-160-k3s1p1 dw':            (4.0e-05, 1.9e-05),      # 7.81e-06, 3.66e-06
    'p1-m2-split-3800x17x17x64-64-k3s1p1 dw':            (1.2e-05, 4.4e-06),      # 2.35e-06, 8.72e-07
    'p1-m2-split-2x2048x2048x8-8-k3s1p1 dw':             (9.0e-06, 7.8e-06),      # 1.79e-06, 1.55e-06
    'p1-m2-split-131072x3x3x8-8-k1s1p0 dw':              (1.0e-06, 3.9e-06),      # 8.82e-07, 7.79e-07
    'p4-m2-split-3650x96x96x32-32-k3s1p1 dw':            (8.5e-06, 6.1e-06),      # 1.70e-06, 1.21e-06
    'p4-m2-split-3650x96x96x32-32-k3s1p1 dbias':         (1.0e-06, 5.2e-06),      # 9.49e-07, 1.03e-06
    'p4-m2-split-130x512x512x32-32-k3s1p1 dw':           (6.2e-06, 6.4e-06),      # 1.23e-06, 1.27e-06
    'p4-m2-split-130x512x512x32-32-k3s1p1 dbias':        (1.0e-06, 5.1e-06),      # 7.57e-07, 1.02e-06
    'p2-m2-split-2100x32x32x16-512-k3s1p1 dw':           (2.1e-05, 1.5e-06),      # 4.08e-06, 1.48e-06
    'rgb_wgrad N1400-512x512-K4 dw':                     (2.8e-06, 1.3e-05),      # 2.72e-06, 2.53e-06
    'linhead gradW':                                     (4.1e-05, 2.9e-05),      # 8.07e-06, 5.76e-06
    'linhead gradb':                                     (6.2e-05, 5.2e-05),      # 1.23e-05, 1.03e-05
}


def release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(*shape, seed=0, scale=1.0):
    t = torch.randn(*shape, device=DEV, generator=gen(seed))
    return t if scale == 1.0 else t.mul_(scale)


class Err(object):
    """Accumulates max|e|, sum e^2, max|ref|, sum ref^2 of float32 results against float64 references chunk by chunk (on the
    device: no host read per chunk).  ``ref`` may broadcast against ``out``."""

    def __init__(self):
        z = lambda: torch.zeros((), dtype=torch.float64, device=DEV)
        self.emax, self.sse, self.rmax, self.rss, self.bad = z(), z(), z(), z(), z()

    def add(self, out, ref):
        o = out.to(torch.float64)
        e = o - ref
        self.bad += (~torch.isfinite(o)).sum()
        self.emax = torch.maximum(self.emax, e.abs().max())
        self.sse += (e * e).sum()
        self.rmax = torch.maximum(self.rmax, ref.abs().max())
        self.rss += (ref * ref).sum() * (o.numel() // ref.numel())

    def result(self):
        assert self.bad.item() == 0, 'non-finite values in the output'
        return ((self.emax / self.rmax.clamp_min(1e-300)).item(), (self.sse.sqrt() / self.rss.sqrt().clamp_min(1e-300)).item())


CHUNK = 1 << 25                         # elements per comparison chunk (256 MiB of float64)


def periodic_errors(out, refpat, err=None):
    """Errors of out (N, ...) against ref[n] = refpat[n % npat] (float64, npat = refpat.shape[0]) over the whole tensor."""
    err = err or Err()
    npat = refpat.shape[0]
    per = max(1, out[0].numel())
    step = max(1, CHUNK // per)
    for j in range(npat):
        sub = out[j::npat]
        for a in range(0, sub.shape[0], step):
            err.add(sub[a:a + step], refpat[j])
    return err


def chunked_errors(out, ref_of, step, err=None):
    """Errors of out (N, ...) against float64 ref_of(a, b) = the reference of out[a:b], ``step`` leading indices at a time."""
    err = err or Err()
    for a in range(0, out.shape[0], step):
        b = min(out.shape[0], a + step)
        err.add(out[a:b], ref_of(a, b))
    return err


def counts(N, npat):
    """How many of N images carry each of the npat patterns."""
    return torch.tensor([len(range(j, N, npat)) for j in range(npat)], dtype=torch.float64, device=DEV)


def fill_periodic(view, pat):
    """view[n] = pat[n % npat] for every n (strided copies, no temporary of the view's size)."""
    npat = pat.shape[0]
    for j in range(npat):
        view[j::npat] = pat[j]


def record(margin, tol, prefix, name, emax, el2, reduction=None, case=None):
    """The contract, then the family bound -- or, for a far reduction listed in FAR_REDUCTION_TOL, its own bound."""
    assert emax < CONTRACT and el2 < CONTRACT, (prefix, name, case or reduction, emax, el2)
    tmax, tl2 = tol[name]
    label = '%s %s' % (prefix, name if not isinstance(name, int) else 'path %2d' % name)
    if case is not None:
        label = 'far %s (%s)' % (case, label)
    if reduction is not None:                      # (every far reduction has a row of its own in the margins table)
        tmax, tl2 = FAR_REDUCTION_TOL.get(reduction, (tmax, tl2))
        label = 'far reduction: %s (%s)' % (reduction, label)
    margin('%s  max-norm' % label, emax, tmax)
    margin('%s  rel-L2' % label, el2, tl2)


class Far(object):
    """An NHWC tensor as the channel slice [off, off + C) of N images of leading dimension ld, inside a flat buffer with a
    spare band (one image, SPARE_MAX floats at most) on each side.  ``fill``: NaN for outputs, 1e3 for inputs."""

    def __init__(self, N, H, W, C, ld, fill):
        self.off = 4 if ld - C >= 4 else 0
        self.body = N * H * W * ld
        self.spare = min(H * W * ld, SPARE_MAX) // 4 * 4 + 4
        self.buf = torch.empty(self.body + 2 * self.spare, device=DEV)
        self.buf.fill_(fill)
        self.fill = fill
        self.rows = self.buf[self.spare:self.spare + self.body].view(N * H * W, ld)
        self.t = self.buf.as_strided((N, H, W, C), (H * W * ld, W * ld, ld, 1), self.spare + self.off)
        self.C, self.ld = C, ld

    def bytes(self):
        return self.body * 4

    def intact(self):
        """Every float outside the slice still holds the fill (NaN of an output, 1e3 of an input)."""
        same = torch.isnan if self.fill != self.fill else (lambda t: t == self.fill)
        ok = same(self.buf[:self.spare]).all() & same(self.buf[self.spare + self.body:]).all()
        if self.off:
            ok &= same(self.rows[:, :self.off]).all()
        if self.off + self.C < self.ld:
            ok &= same(self.rows[:, self.off + self.C:]).all()
        return bool(ok)


def far_input(N, H, W, C, ld, pat):
    t = Far(N, H, W, C, ld, 1e3)
    fill_periodic(t.t, pat)
    return t


class Flat(object):
    """A dense operand of ``shape`` with ``pad`` NaN floats either side (pad a multiple of 4: 16-byte alignment kept); the
    operand itself is NaN too when ``nan`` (outputs), else left for the caller to fill."""

    def __init__(self, shape, pad=4096, nan=True, dtype=torch.float32):
        n = math.prod(shape)
        self.n, self.pad = n, pad
        self.buf = torch.empty(n + 2 * pad, device=DEV, dtype=dtype)
        if nan:
            self.buf.fill_(NAN)
        else:
            self.buf[:pad] = NAN
            self.buf[pad + n:] = NAN
        self.view = self.buf[pad:pad + n].view(*shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.pad]).all() & torch.isnan(self.buf[self.pad + self.n:]).all())


def P_(t):
    return ops._p(t)


def call(name, *args):
    lib().call(name, *args, ops._stream())


def cf(v):
    return ctypes.c_float(v)


# ======================================================================================================================
# the conv engine: one far case per (path, mode) of test_conv_paths_gpu.PATH_CASES
# ======================================================================================================================
# (path, mode, split, N, H, W, C, ldx, K, ldy, k, stride, pad, far operands, prepared filter too, what)
# far operands: 'x' the x-side activations (x / dx / act_ref), 'y' the y-side ones (y / gy / addend)
# Contraction lengths C * k * k stay within about twice those of the small matrix: the family bounds were observed there, and
# the error of a forward / data gradient grows with the root of the contraction, not with the batch.  Three rows therefore
# differ from the shapes this matrix started from; what those gave against float64 (max-norm, rel-L2), measured with this code:
#   path 3 data gradient, 2100 x 32^2, 16 <- 512 (contraction 4608):  2.49e-6, 1.20e-6  against the family's 1.5e-6, 6.0e-7
#   path 3 forward, 32868 x 8^2, 512 -> 16 (contraction 4608):        1.40e-6, 7.95e-7  against 1.5e-6, 6.0e-7
#     (twice the rel-L2 of the 1152-long contractions, as the root predicts: numerical, every value right to six digits;
#     both rows stay in the matrix for their paths 7 / 2 / 3, path 3 forward and data gradient have other far cases);
#   the kNN bank GEMM with all 8192 channels: forward 1.96e-6, 1.13e-6 with one seed and 3.64e-6 max-norm with another,
#     against 3.0e-6, 1.5e-6; data gradient 8.7e-7, 4.0e-7: it reads a 1024-channel slice of the 8192-wide rows instead.
# The last rows have C = K = 8 where 64 would also plan path 1: the float64 reference of one 2048^2 x 64 image unfolds to
# 19 GB.
FAR_CASES = [
    (0, 0, False, 2100, 32, 32, 3, 512, 5, 512, 3, 1, 1, 'xy', False, 'Cin = 3: scalar gathers'),
    (0, 1, False, 2100, 32, 32, 3, 512, 5, 512, 3, 1, 1, 'xy', False, ''),
    (0, 2, True, 2100, 32, 32, 3, 512, 5, 512, 3, 1, 1, 'xy', False, ''),
    (1, 0, False, 131072, 3, 3, 8, 1024, 8, 1024, 1, 1, 0, 'xy', False, ''),
    (1, 1, False, 131072, 3, 3, 8, 1024, 8, 1024, 1, 1, 0, 'xy', False, ''),
    (1, 2, True, 131072, 3, 3, 8, 1024, 8, 1024, 1, 1, 0, 'xy', False, ''),
    (2, 0, False, 140000, 1, 1, 1024, 8192, 512, 512, 1, 1, 0, 'x', False, 'a kNN-bank GEMM: rows 32 KiB apart, only the bank is far'),
    (2, 1, False, 140000, 1, 1, 1024, 8192, 512, 512, 1, 1, 0, 'x', False, ''),
    (2, 2, True, 140000, 1, 1, 1024, 8192, 512, 512, 1, 1, 0, 'x', False, ''),
    (3, 0, False, 3800, 17, 17, 64, 1024, 64, 1024, 3, 1, 1, 'xy', False, 'odd 17 x 17 map'),
    (3, 1, False, 3800, 17, 17, 64, 1024, 64, 1024, 3, 1, 1, 'xy', False, ''),
    (1, 2, True, 3800, 17, 17, 64, 1024, 64, 1024, 3, 1, 1, 'xy', False, ''),
    (3, 0, False, 262160, 2, 2, 128, 1024, 8, 1024, 3, 1, 1, 'xy', False, 'pixel-major tiles'),
    (1, 1, False, 262160, 2, 2, 128, 1024, 8, 1024, 3, 1, 1, 'xy', False, ''),
    (3, 2, True, 262160, 2, 2, 128, 1024, 8, 1024, 3, 1, 1, 'xy', False, ''),
    (11, 0, False, 130, 512, 512, 32, 32, 32, 32, 3, 1, 1, 'xy', False, 'StyleGAN2-512 first block, dense'),
    (11, 1, False, 130, 512, 512, 32, 32, 32, 32, 3, 1, 1, 'xy', False, ''),
    (4, 2, True, 130, 512, 512, 32, 32, 32, 32, 3, 1, 1, 'xy', False, 'wgrad_c32 needs the dense ld'),
    (6, 0, False, 3650, 96, 96, 32, 32, 32, 32, 3, 1, 1, 'xy', False, 'conv_c32: a map that is no power of two'),
    (6, 1, False, 3650, 96, 96, 32, 32, 32, 32, 3, 1, 1, 'xy', False, ''),
    (4, 2, True, 3650, 96, 96, 32, 32, 32, 32, 3, 1, 1, 'xy', False, ''),
    (5, 0, False, 1048584, 1, 1, 16, 1024, 1, 1024, 1, 1, 0, 'xy', False, 'the logit: one output channel'),
    (0, 1, False, 1048584, 1, 1, 16, 1024, 1, 1024, 1, 1, 0, 'xy', False, ''),
    (0, 2, True, 1048584, 1, 1, 16, 1024, 1, 1024, 1, 1, 0, 'xy', False, ''),
    (7, 0, False, 2100, 32, 32, 16, 512, 512, 512, 3, 1, 1, 'xy', False, 'F(2x2,3x3)'),
    (2, 2, True, 2100, 32, 32, 16, 512, 512, 512, 3, 1, 1, 'xy', False, ''),
    (7, 1, False, 32868, 8, 8, 512, 512, 16, 512, 3, 1, 1, 'xy', True, 'F(2x2,3x3) data gradient, prepared filter too'),
    (2, 2, True, 32868, 8, 8, 512, 512, 16, 512, 3, 1, 1, 'xy', False, ''),
    (9, 0, False, 66, 256, 256, 64, 256, 64, 256, 3, 1, 1, 'xy', True, 'F(4x4,3x3), prepared filter too'),
    (9, 1, False, 66, 256, 256, 64, 256, 64, 256, 3, 1, 1, 'xy', False, ''),
    (7, 2, True, 66, 256, 256, 64, 256, 64, 256, 3, 1, 1, 'xy', False, 'F(3x3,2x2)'),
    (8, 0, False, 2100, 32, 32, 64, 512, 128, 2048, 4, 2, 1, 'xy', False, 'F(2x2,2x2) phases'),
    (8, 1, False, 2100, 32, 32, 64, 512, 128, 2048, 4, 2, 1, 'xy', False, ''),
    (8, 2, True, 2100, 32, 32, 64, 512, 128, 2048, 4, 2, 1, 'xy', False, ''),
    (10, 0, False, 1100, 33, 33, 16, 1024, 256, 4096, 3, 2, 0, 'xy', False, 'strided 3x3 phases'),
    (2, 1, False, 1100, 33, 33, 16, 1024, 256, 4096, 3, 2, 0, 'xy', False, ''),
    (2, 2, True, 1100, 33, 33, 16, 1024, 256, 4096, 3, 2, 0, 'xy', False, ''),
    (11, 0, False, 66000, 4, 4, 32, 1024, 160, 1024, 3, 1, 1, 'xy', False, 'F(4x4,3x3), 32-wide cout blocks'),
    (11, 1, False, 66000, 4, 4, 32, 1024, 160, 1024, 3, 1, 1, 'xy', False, ''),
    (2, 2, True, 66000, 4, 4, 32, 1024, 160, 1024, 3, 1, 1, 'xy', False, ''),
    # split-K forward and data gradient: few output rows, so only a huge leading dimension makes an operand far
    (2, 0, True, 9, 17, 17, 64, 64, 64, 464424, 3, 1, 1, 'y', False, 'split-K forward into rows 1.8 MB apart'),
    (2, 1, True, 9, 17, 17, 64, 64, 64, 464424, 3, 1, 1, 'y', False, 'split-K data gradient of such a gy'),
    # one image alone is 2 GiB: every block-relative family refuses it, the guards' fallback runs
    # (two such images span exactly 2^32 bytes: no operand is declared far, the image-relative offsets pass 2^31)
    (1, 0, False, 2, 2048, 2048, 8, 128, 8, 128, 3, 1, 1, '', False, 'one image of 2 GiB: the fallback of every guard'),
    (1, 1, False, 2, 2048, 2048, 8, 128, 8, 128, 3, 1, 1, '', False, ''),
    (1, 2, True, 2, 2048, 2048, 8, 128, 8, 128, 3, 1, 1, '', False, ''),
]


def far_desc(case):
    _, _, _, N, H, W, C, ldx, K, ldy, k, s, p = case[:13]
    return ops.make_desc(N, H, W, C, K, k, k, s, p, ldx, ldy, far_ldw(case))


def far_ldw(case):
    """Four spare columns past the channel count rounded to 4 (wgrad_c32, path 4, needs the dense filter)."""
    return (case[8] + 3) // 4 * 4 + (0 if case[0] == 4 else 4)


def far_id(case):
    Pth, m, sp, N, H, W, C, ldx, K, ldy, k, s, p = case[:13]
    return 'p%d-m%d%s-%dx%dx%dx%d-%d-k%ds%dp%d' % (Pth, m, '-split' if sp else '', N, H, W, C, K, k, s, p)


def _far_weights(case, seed):
    _, _, _, N, H, W, C, ldx, K, ldy, k, s, p = case[:13]
    w = randn(K, C, k, k, seed=seed, scale=1.0 / math.sqrt(C * k * k))
    wp = torch.zeros(k * k * C, far_ldw(case), device=DEV)
    wp[:, :K] = w.permute(2, 3, 1, 0).reshape(k * k * C, K)
    return w, wp


@pytest.mark.parametrize('case', FAR_CASES, ids=far_id)
def test_far_conv_matches_float64(case, margin):
    Pth, mode, split, N, H, W, C, ldx, K, ldy, k, s, p, far, prep, _ = case
    d = far_desc(case)
    assert lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode) == Pth
    Ho, Wo = d.Ho, d.Wo
    seed = 5000 + FAR_CASES.index(case)
    npat = min(N, P)
    w, wp = _far_weights(case, seed)
    name = far_id(case)
    if mode == 0:
        xp, ap = randn(npat, H, W, C, seed=seed + 1), randn(npat, Ho, Wo, K, seed=seed + 2)
        bias = randn(K, seed=seed + 3, scale=0.3)
        ref = R.fwd(xp, w, bias, s, p, SLOPE, GAIN, ap)
        x, add = far_input(N, H, W, C, ldx, xp), far_input(N, Ho, Wo, K, ldy, ap)
        y = Far(N, Ho, Wo, K, ldy, NAN)
        assert ('x' not in far or x.bytes() > 2 ** 32) and ('y' not in far or y.bytes() > 2 ** 32)
        pf = ops.filter_prep([(0, d, wp)], torch.device(DEV)) if prep else None
        assert not prep or pf.get(0, wp) is not None
        for filters in ((None, pf) if prep else (None,)):
            y.buf.fill_(NAN)
            ops.conv2d_fwd(x.t, wp, bias, K, k, k, s, p, slope=SLOPE, gain=GAIN, out=y.t, addend=add.t, filters=filters)
            torch.cuda.synchronize()
            assert y.intact(), 'forward wrote outside y'
            assert x.intact() and add.intact(), 'forward wrote into the guard bands of its inputs'
            record(margin, CONV_TOL, 'conv', Pth, *periodic_errors(y.t, ref).result(), case=name + (' prepared' if filters else ''))
        del x, add, y, pf
    elif mode == 1:
        gp, ap = randn(npat, Ho, Wo, K, seed=seed + 1), randn(npat, H, W, C, seed=seed + 2)
        ref = R.dgrad(gp, w, (H, W), s, p, ap, SLOPE, GAIN)
        gy, act = far_input(N, Ho, Wo, K, ldy, gp), far_input(N, H, W, C, ldx, ap)
        dx = Far(N, H, W, C, ldx, NAN)
        assert ('x' not in far or dx.bytes() > 2 ** 32) and ('y' not in far or gy.bytes() > 2 ** 32)
        pf = ops.filter_prep([(1, d, wp)], torch.device(DEV)) if prep else None
        assert not prep or pf.get(1, wp) is not None
        for filters in ((None, pf) if prep else (None,)):
            dx.buf.fill_(NAN)
            ops.conv2d_dgrad(gy.t, wp, (N, H, W, C), k, k, s, p, act_ref=act.t, slope=SLOPE, gain=GAIN, out=dx.t,
                             filters=filters)
            torch.cuda.synchronize()
            assert dx.intact(), 'data gradient wrote outside dx'
            assert gy.intact() and act.intact(), 'data gradient wrote into the guard bands of its inputs'
            record(margin, CONV_TOL, 'conv', Pth, *periodic_errors(dx.t, ref).result(), case=name + (' prepared' if filters else ''))
        del gy, act, dx, pf
    else:
        xp, gp = randn(npat, H, W, C, seed=seed + 1), randn(npat, Ho, Wo, K, seed=seed + 2)
        cnt = counts(N, npat)
        refw, refb = R.wgrad(xp, gp.to(torch.float64) * cnt.view(-1, 1, 1, 1), k, k, s, p)
        refw = refw.permute(2, 3, 1, 0).reshape(k * k * C, K)
        x, gy = far_input(N, H, W, C, ldx, xp), far_input(N, Ho, Wo, K, ldy, gp)
        assert ('x' not in far or x.bytes() > 2 ** 32) and ('y' not in far or gy.bytes() > 2 ** 32)
        ldw = far_ldw(case)
        bias_ok = C % 4 == 0 and K % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0
        dwb = torch.full((k * k * C + 2, ldw), NAN, device=DEV)
        dbb = torch.full((K + 8,), NAN, device=DEV)
        dwp, dbias = dwb[1:-1], (dbb[4:4 + K] if bias_ok else None)
        ops.conv2d_wgrad(x.t, gy.t, k, k, s, p, out=dwp, dbias=dbias)
        torch.cuda.synchronize()
        inner = torch.zeros_like(dwb, dtype=torch.bool)
        inner[1:-1, :K] = True
        assert torch.isnan(dwb[~inner]).all(), 'weight gradient wrote outside dwp[:, :K]'
        assert x.intact() and gy.intact(), 'weight gradient wrote into the guard bands of its inputs'
        e = Err()
        e.add(dwp[:, :K], refw)
        record(margin, CONV_TOL, 'conv', Pth, *e.result(), reduction=name + ' dw')
        if bias_ok:
            assert torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all(), 'dbias written out of range'
            e = Err()
            e.add(dbias, refb)
            record(margin, CONV_TOL, 'conv', Pth, *e.result(), reduction=name + ' dbias')
        del x, gy
    release()


# ======================================================================================================================
# upfirdn2d: the 4x4-FIR forms on far tensors, through the fused entry point with every epilogue operand
# ======================================================================================================================
FIR_PADS = {(1, 1): (1, 2, 1, 2), (1, 2): (1, 1, 1, 1), (2, 1): (2, 1, 2, 1)}      # (up, down) -> px0, px1, py0, py1
# (form, major, in_h, in_w, minor, up, down, what)
UF_FAR_CASES = [
    ('u1d1_buf', 130, 512, 512, 32, 1, 1, 'blur: input, output, addend, act_ref and out2 of 4.06 GiB each'),
    ('u1d2_buf', 130, 512, 512, 32, 1, 2, 'decimating blur: a far input'),
    ('u2d1_buf', 130, 256, 256, 32, 2, 1, 'upsampling FIR: far outputs'),
    ('u1d1_ptr', 2, 4096, 4096, 32, 1, 1, 'one image of 2^31 bytes: the pointer form'),
    ('u1d2_ptr', 2, 4096, 4096, 32, 1, 2, 'one input image of 2^31 bytes'),
    ('u2d1_ptr', 2, 2048, 2048, 32, 2, 1, 'one output image of 2^31 bytes'),
]


def uf_cfg(case):
    form, major, in_h, in_w, minor, up, down, _ = case
    return (major, in_h, in_w, minor, 4, 4, up, up, down, down) + FIR_PADS[(up, down)]


def _fir(seed):
    return (torch.rand(4, 4, device=DEV, generator=gen(seed)) + 0.1) / 16


def periodic_operand(shape, seed):
    """(storage, pattern) of a dense input whose image n is pattern[n % P]; with no more than P images the operand is its
    own pattern (random over the whole tensor)."""
    t = Flat(shape, nan=False)
    if shape[0] <= P:
        t.view.normal_(generator=gen(seed))
        return t, t.view
    pat = randn(min(shape[0], P), *shape[1:], seed=seed)
    fill_periodic(t.view, pat)
    return t, pat


def _fir_errors(outs, ref_of, npat, minor):
    """Each out (major, oh, ow, minor) of ``outs`` against ref_of(j, c0, c1) = the tuple of float64 references of images
    j, j + npat, ... in channels [c0, c1): the references are made four channels at a time and compared in bands of
    rows, so no float64 image is ever whole."""
    errs = [Err() for _ in outs]
    oh, ow = outs[0].shape[1:3]
    band = max(1, min(oh, CHUNK // (ow * 4)))
    for j in range(npat):
        for c0 in range(0, minor, 4):
            refs = ref_of(j, c0, c0 + 4)
            for out, ref, err in zip(outs, refs, errs):
                sub = out[j::npat]
                step = max(1, CHUNK // (band * ow * 4))
                for r in range(0, oh, band):
                    for a in range(0, sub.shape[0], step):
                        err.add(sub[a:a + step, r:r + band, :, c0:c0 + 4], ref[:, r:r + band])
    return errs


@pytest.mark.parametrize('case', UF_FAR_CASES, ids=lambda c: c[0])
def test_far_upfirdn2d_fused(case, margin):
    form, major, in_h, in_w, minor, up, down, _ = case
    cfg = uf_cfg(case)
    oh, ow = S.out_size(*cfg[1:3], *cfg[4:])
    npat = min(major, P)
    seed = 6000 + UF_FAR_CASES.index(case)
    k = _fir(seed)
    x, xp = periodic_operand((major, in_h, in_w, minor), seed + 1)
    add, ap = periodic_operand((major, oh, ow, minor), seed + 2)
    aref, rp = periodic_operand((major, oh, ow, minor), seed + 3)
    out, out2 = Flat((major, oh, ow, minor)), Flat((major, oh, ow, minor))
    call('contrad_upfirdn2d_fused', P_(x.view), P_(k), P_(out.view), *cfg, P_(add.view), P_(aref.view), cf(SLOPE), cf(GAIN),
         P_(out2.view))
    torch.cuda.synchronize()
    assert out.intact() and out2.intact() and x.intact() and add.intact() and aref.intact()
    if major > P:
        x = add = aref = None                          # (the patterns are what the references read)

    def refs(j, c0, c1):
        v = S.upfirdn2d(xp[j:j + 1, :, :, c0:c1], k, *cfg[6:])
        return S.fused_epilogue(v, ap[j:j + 1, :, :, c0:c1], rp[j:j + 1, :, :, c0:c1], SLOPE, GAIN)

    for e in _fir_errors((out.view, out2.view), refs, npat, minor):
        record(margin, SG2_TOL, 'sg2', 'upfirdn', *e.result())
    del out, out2, x, add, aref, xp, ap, rp
    release()


# (form, N, in_h, in_w, K, what)
MODCONV_FAR_CASES = [
    ('u1d1_buf', 130, 512, 512, 32, 'the upsampling StyledConv tail at 512^2'),
    ('u1d1_ptr', 2, 4096, 4096, 32, 'one image of 2^31 bytes'),
]


@pytest.mark.parametrize('case', MODCONV_FAR_CASES, ids=lambda c: c[0])
def test_far_upfirdn2d_modconv(case, margin):
    form, N, in_h, in_w, K, _ = case
    pads = FIR_PADS[(1, 1)]
    oh, ow = S.out_size(in_h, in_w, 4, 4, 1, 1, 1, 1, *pads)
    npat = min(N, P)
    seed = 6100 + MODCONV_FAR_CASES.index(case)
    k = _fir(seed)
    x, xp = periodic_operand((N, in_h, in_w, K), seed + 1)
    dp = torch.rand(npat, K, device=DEV, generator=gen(seed + 2)) + 0.5
    qp = torch.rand(npat, K, device=DEV, generator=gen(seed + 3)) + 0.5
    zp = randn(npat, oh, ow, seed=seed + 4)
    bias, nw = randn(K, seed=seed + 5), torch.tensor([0.3], device=DEV)
    idx = torch.arange(N, device=DEV) % npat
    demod, post, noise = dp[idx].contiguous(), qp[idx].contiguous(), zp[idx].contiguous()
    y = Flat((N, oh, ow, K))
    call('contrad_upfirdn2d_modconv', P_(x.view), P_(k), P_(y.view), N, in_h, in_w, K, *pads, P_(demod), P_(noise), P_(nw),
         P_(bias), P_(post))
    torch.cuda.synchronize()
    assert y.intact() and x.intact()

    def ref(j, c0, c1):
        v = S.upfirdn2d(xp[j:j + 1, :, :, c0:c1], k, 1, 1, 1, 1, *pads)
        return (S.modconv_epilogue(v, bias[c0:c1], dp[j:j + 1, c0:c1], zp[j:j + 1], nw, qp[j:j + 1, c0:c1]),)

    record(margin, SG2_TOL, 'sg2', 'modconv', *_fir_errors((y.view,), ref, npat, K)[0].result())
    del x, y, xp, noise
    release()


# ======================================================================================================================
# element-wise kernels, flat or NHWC: random data over the whole tensor, the float64 expression in chunks
# ======================================================================================================================
FLAT_N = 2 ** 30 + 2 ** 22 + 5          # the scalar tail sits past 4 GiB too
ROW = 599999                            # "image" of a flat op: an odd row length that divides no power of two
BIAS_C = 24                             # channels of the flat bias (chunks start at multiples of it)
ESTEP = CHUNK // BIAS_C * BIAS_C


def _flat_random(n, seed):
    t = Flat((n,), nan=False)
    t.view.normal_(generator=gen(seed))
    return t


@pytest.mark.parametrize('act,grad', [(3, 0), (3, 1), (3, 2)], ids=['act3-grad0', 'act3-grad1', 'act3-grad2'])
def test_far_fused_bias_act(act, grad, margin):
    n = FLAT_N
    x, ref = _flat_random(n, 7001), (_flat_random(n, 7002) if grad == 1 else None)
    b = randn(BIAS_C, seed=7003)
    y = Flat((n,))
    alpha, scale = f32(0.2), f32(1.4142135)
    call('contrad_fused_bias_act', P_(x.view), P_(b), P_(ref.view if ref else None), P_(y.view), n, 1, BIAS_C, act, grad,
         cf(alpha), cf(scale))
    torch.cuda.synchronize()
    assert y.intact() and x.intact()
    if grad == 2:         # (the result does not depend on x: the point is that every element past 4 GiB is written, with a zero)
        assert int((y.view != 0).sum()) == 0
    else:
        rv = ref.view if ref else None
        e = chunked_errors(y.view, lambda a, c: S.fused_bias_act(x.view[a:c], b, None if rv is None else rv[a:c], 1, BIAS_C,
                                                                 act, grad, alpha, scale), ESTEP)
        record(margin, SG2_TOL, 'sg2', 'bias_act', *e.result())
    del x, ref, y
    release()


def test_far_lincomb_axpby_scale_dev(margin):
    n = FLAT_N
    x, z = _flat_random(n, 7011), _flat_random(n, 7012)
    y = Flat((n,))
    a, b = f32(0.7071068), f32(-1.3)
    call('contrad_lincomb', P_(x.view), P_(z.view), P_(y.view), n, cf(a), cf(b))
    torch.cuda.synchronize()
    assert y.intact()
    record(margin, SG2_TOL, 'sg2', 'lincomb',
           *chunked_errors(y.view, lambda p, q: S.lincomb(x.view[p:q], z.view[p:q], a, b), CHUNK).result())
    # scale_dev into the same output
    y.buf.fill_(NAN)
    s = torch.tensor([-0.37], device=DEV)
    c = f32(2.5)
    call('contrad_scale_dev', P_(x.view), P_(s), cf(c), P_(y.view), n)
    torch.cuda.synchronize()
    assert y.intact()
    record(margin, SG2_TOL, 'sg2', 'scale_dev',
           *chunked_errors(y.view, lambda p, q: S.scale_dev(x.view[p:q], s, c), CHUNK).result())
    # axpby_ in place on z: z = a2 * z + b2 * x, against y = the float64 expression of the old z (kept in y first)
    y.view.copy_(z.view)
    a2, b2 = f32(0.999), f32(0.001)
    ops.axpby_(z.view, x.view, a2, b2)
    torch.cuda.synchronize()
    assert z.intact() and x.intact()
    record(margin, DSTEP_TOL, 'dstep', 'axpby',
           *chunked_errors(z.view, lambda p, q: a2 * y.view[p:q].double() + b2 * x.view[p:q].double(), CHUNK).result())
    del x, y, z
    release()


def test_far_sumsq(margin):
    n = FLAT_N
    x = _flat_random(n, 7021)
    nbytes = lib().raw('contrad_sumsq_workspace_bytes')(ctypes.c_longlong(n))
    ws, out = Flat((nbytes // 4,), pad=4), Flat((1,), pad=4)
    scale = 0.125
    call('contrad_sumsq', P_(x.view), ctypes.c_longlong(n), cf(scale), P_(out.view), P_(ws.view), ctypes.c_longlong(nbytes))
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and x.intact()
    ref = torch.zeros((), dtype=torch.float64, device=DEV)
    for a in range(0, n, CHUNK):
        ref += S.sumsq(x.view[a:a + CHUNK], scale)
    e = Err()
    e.add(out.view, ref.view(1))
    record(margin, SG2_TOL, 'sg2', 'sumsq', *e.result(), reduction='sumsq')
    del x
    release()


# (N, HW, C): images of an odd pixel count, 4.0 GiB
NHWC_FAR = (67, 599999, 28)


def test_far_nhwc_scale_and_modconv_epilogue(margin):
    N, HW, C = NHWC_FAR
    assert N * HW * C * 4 > 2 ** 32 + HW * C * 4 and N * HW * C < 2 ** 31
    x = Flat((N, HW, C), nan=False)
    x.view.normal_(generator=gen(7031))
    s = randn(N, C, seed=7032)
    y = Flat((N, HW, C))
    call('contrad_nhwc_scale', P_(x.view), P_(s), P_(y.view), N, ctypes.c_longlong(HW), C)
    torch.cuda.synchronize()
    assert y.intact() and x.intact()
    record(margin, SG2_TOL, 'sg2', 'nhwc_scale',
           *chunked_errors(y.view, lambda a, b: S.nhwc_scale(x.view[a:b], s[a:b], b - a, HW, C), 1).result())
    # modconv_epilogue_ with every term, out of place into the same output
    y.buf.fill_(NAN)
    demod = torch.rand(N, C, device=DEV, generator=gen(7033)) + 0.5
    post = torch.rand(N, C, device=DEV, generator=gen(7034)) + 0.5
    noise, nw, bias = randn(N, HW, seed=7035), torch.tensor([0.3], device=DEV), randn(C, seed=7036)
    call('contrad_modconv_epilogue', P_(x.view), P_(demod), P_(noise), P_(nw), P_(bias), P_(post), P_(y.view), N,
         ctypes.c_longlong(HW), C)
    torch.cuda.synchronize()
    assert y.intact() and x.intact()

    def ref(a, b):
        return S.modconv_epilogue(x.view[a:b].view(b - a, HW, 1, C), bias, demod[a:b], noise[a:b].view(b - a, HW, 1), nw,
                                  post[a:b]).view(b - a, HW, C)

    record(margin, SG2_TOL, 'sg2', 'modconv', *chunked_errors(y.view, ref, 1).result())
    del x, y
    release()


@pytest.mark.parametrize('per_channel', [1, 0], ids=['b-per-channel', 'b-broadcast'])
def test_far_nhwc_dot(per_channel, margin):
    N, HW, C = NHWC_FAR
    a = Flat((N, HW, C), nan=False)
    a.view.normal_(generator=gen(7041))
    b = Flat((N, HW, C) if per_channel else (N, HW), nan=False)
    b.view.normal_(generator=gen(7042))
    nbytes = lib().raw('contrad_nhwc_dot_workspace_bytes')(N, ctypes.c_longlong(HW), C)
    ws, out = Flat((nbytes // 4,), pad=4), Flat((N, C), pad=4)
    call('contrad_nhwc_dot', P_(a.view), P_(b.view), P_(out.view), N, ctypes.c_longlong(HW), C, per_channel, P_(ws.view),
         ctypes.c_longlong(nbytes))
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and a.intact() and b.intact()
    e = chunked_errors(out.view, lambda p, q: S.nhwc_dot(a.view[p:q], b.view[p:q], q - p, HW, C, per_channel), 1)
    record(margin, SG2_TOL, 'sg2', 'nhwc_dot', *e.result(), reduction='nhwc_dot b%d' % per_channel)
    del a, b
    release()


# ======================================================================================================================
# RGB-end convolutions (csrc/conv_small.hip)
# ======================================================================================================================
def _packed(w, extra=4):
    K, C, k, _ = w.shape
    wp = torch.full((k * k * C, ops.round_up(K, 4) + extra), NAN, device=DEV)
    wp[:, :K] = w.permute(2, 3, 1, 0).reshape(k * k * C, K)
    return wp


# (N, H, W, K, ldy, k, what)
RGB_FAR_CASES = [
    (2100, 32, 32, 64, 512, 3, 'a far y / gy: the SNDCGAN first conv into a wide buffer'),
    (1400, 512, 512, 4, 4, 3, 'a far image tensor (4.4 GiB) and a dense far y (5.9 GiB)'),
]


@pytest.mark.parametrize('case', RGB_FAR_CASES, ids=lambda c: 'N%d-%dx%d-K%d-ldy%d' % c[:5])
def test_far_rgb_conv_fwd_wgrad(case, margin):
    N, H, W, K, ldy, k, _ = case
    seed = 7100 + RGB_FAR_CASES.index(case)
    ip = torch.rand(P, 3, H, W, device=DEV, generator=gen(seed))
    w = randn(K, 3, k, k, seed=seed + 1, scale=0.2)
    bias = randn(K, seed=seed + 2, scale=0.1)
    wp = _packed(w)
    img = Flat((N, 3, H, W), nan=False)
    fill_periodic(img.view, ip)
    y = Far(N, H, W, K, ldy, NAN)
    assert y.bytes() > 2 ** 32
    ops.rgb_conv_fwd(img.view, wp, bias, K, k, 2.0, -1.0, SLOPE, GAIN, out=y.t)
    torch.cuda.synchronize()
    assert y.intact() and img.intact()
    ref = D.rgb_fwd(ip, w, bias, 2.0, -1.0, SLOPE, GAIN)
    record(margin, DSTEP_TOL, 'dstep', 'rgb_fwd', *periodic_errors(y.t, ref).result())
    # weight gradient: gy periodic in the same storage, the reference weighted by the pattern counts
    gp = randn(P, H, W, K, seed=seed + 3)
    y.buf.fill_(NAN)                                   # (NaN in the spare channels and bands: a stray read shows)
    fill_periodic(y.t, gp)
    ldw = K + 8
    dwb = torch.full((k * k * 3 + 2, ldw), NAN, device=DEV)
    dbb = torch.full((K + 8,), NAN, device=DEV)
    ops.rgb_conv_wgrad(img.view, y.t, k, 2.0, -1.0, dwb[1:-1, :K], dbb[4:4 + K])
    torch.cuda.synchronize()
    inner = torch.zeros_like(dwb, dtype=torch.bool)
    inner[1:-1, :K] = True
    assert torch.isnan(dwb[~inner]).all() and torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all()
    cnt = counts(N, P)
    dw_ref, db_ref = D.rgb_wgrad(ip, gp.to(torch.float64) * cnt.view(-1, 1, 1, 1), k, 2.0, -1.0)
    what = 'rgb_wgrad N%d-%dx%d-K%d' % (N, H, W, K)
    e = Err()
    e.add(ops.unpack_weight(dwb[1:-1], K, 3, k, k), dw_ref)
    record(margin, DSTEP_TOL, 'dstep', 'rgb_wgrad', *e.result(), reduction=what + ' dw')
    e = Err()
    e.add(dbb[4:4 + K], db_ref)
    record(margin, DSTEP_TOL, 'dstep', 'rgb_wgrad', *e.result(), reduction=what + ' dbias')
    del img, y
    release()


def test_far_rgb_conv_dgrad(margin):
    """A far gy (2100 x 32^2 x 64 in a 512-wide buffer) into NCHW images, tanh end."""
    N, H, W, K, ldy, C, k = 2100, 32, 32, 64, 512, 3, 3
    gp = randn(P, H, W, K, seed=7201, scale=0.1)
    w = randn(K, C, k, k, seed=7202, scale=0.1)
    bias = randn(C, seed=7203, scale=0.1)
    gy = far_input(N, H, W, K, ldy, gp)
    assert gy.bytes() > 2 ** 32
    out = Flat((N, C, H, W))
    ops.rgb_conv_dgrad(gy.t, _packed(w), bias, C, k, act=1, out_scale=0.5, out_shift=0.5, out=out.view)
    torch.cuda.synchronize()
    assert out.intact()
    ref = D.rgb_dgrad(gp, w, bias, 1, 0.5, 0.5)
    record(margin, DSTEP_TOL, 'dstep', 'rgb_dgrad', *periodic_errors(out.view, ref).result())
    del gy, out
    release()


RGB_DGRAD_FAR_OUT = (1030, 512, 512, 16, 4, 1)      # N, H, W, K, C, k: out 4.02 GiB, gy 16.1 GiB = 4.3e9 elements


def test_far_rgb_conv_dgrad_far_output(margin):
    """The generic rgb_conv_dgrad_kernel (C = 4, ToRGB-style 1x1 with per-sample modulation) storing NCHW images past 4 GiB.
    Its gy has 16 channels per pixel: 16.1 GiB and more than 2^31 ELEMENTS -- the RGB convs have no element limit
    (include/contrad_hip.h), and this is the one case of the module that shows it."""
    N, H, W, K, C, k = RGB_DGRAD_FAR_OUT
    gp = randn(P, H, W, K, seed=7211, scale=0.1)
    mp = torch.rand(P, K, device=DEV, generator=gen(7212)) + 0.5
    w = randn(K, C, k, k, seed=7213, scale=0.3)
    bias = randn(C, seed=7214, scale=0.1)
    gy = far_input(N, H, W, K, K, gp)
    out = Flat((N, C, H, W))
    assert out.n * 4 > 2 ** 32 + C * H * W * 4 and out.n < 2 ** 31 and gy.body > 2 ** 31
    mod = mp[torch.arange(N, device=DEV) % P].contiguous()
    ops.rgb_conv_dgrad(gy.t, _packed(w), bias, C, k, act=1, out_scale=0.5, out_shift=0.5, out=out.view, mod=mod)
    torch.cuda.synchronize()
    assert out.intact() and gy.intact()
    ref = D.rgb_dgrad(gp, w, bias, 1, 0.5, 0.5, mod=mp)
    record(margin, DSTEP_TOL, 'dstep', 'rgb_dgrad', *periodic_errors(out.view, ref).result())
    del gy, out
    release()


# ======================================================================================================================
# row-wise statistics and BatchNorm on rows of a wide buffer: M = 2^20 + 3 rows, K = 64, ld = 1024 (4.0 GiB)
# ======================================================================================================================
ROWS_FAR = (2 ** 20 + 3, 64, 1024)


def _far_rows(M, K, ld, fill, data=None):
    """(storage, (M, K) view at column 4 of rows of stride ld, a spare row band either side)."""
    t = Far(M, 1, 1, K, ld, fill)
    v = t.buf.as_strided((M, K), (ld, 1), t.spare + t.off)
    if data is not None:
        v.copy_(data)
    return t, v


def test_far_colstats_bn(margin):
    M, K, ld = ROWS_FAR
    assert M * ld * 4 > 2 ** 32 + ld * 4 and M * ld < 2 ** 31
    g = gen(7301)
    std = torch.rand(K, device=DEV, generator=g) * 2 + 0.1
    x0 = torch.randn(M, K, device=DEV, generator=g) * std + 0.25
    gamma = torch.rand(K, device=DEV, generator=g) + 0.5
    beta = torch.randn(K, device=DEV, generator=g) * 0.3
    xs, x = _far_rows(M, K, ld, 1e3, x0)
    eps = 1e-5
    ref = D.colstats(x0)
    for with_sq in (False, True):
        out = Flat((2 if with_sq else 1, K), pad=4)
        ops.colstats(x, with_sq=with_sq, out=out.view)
        torch.cuda.synchronize()
        assert out.intact()
        for i, nm in enumerate(('sum', 'sumsq')[:2 if with_sq else 1]):
            e = Err()
            e.add(out.view[i], ref[i])
            record(margin, DSTEP_TOL, 'dstep', 'colstats', *e.result(), reduction='colstats sq%d %s' % (with_sq, nm))
    # bn_batch_stats: the same sums and the running update in two launches
    rm0, rv0 = randn(K, seed=7302), torch.rand(K, device=DEV, generator=gen(7303)) + 0.5
    cb = randn(K, seed=7304, scale=0.1)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
    stats = ops.bn_batch_stats(x, cb, 0.1, rm, rv, nbt)
    rm_ref, rv_ref = D.bn_running(rm0, rv0, x0, cb, 0.1)
    torch.cuda.synchronize()
    assert nbt.item() == 42
    for nm, got, want in (('stats', stats, ref), ('running mean', rm, rm_ref), ('running var', rv, rv_ref)):
        e = Err()
        e.add(got, want)
        record(margin, DSTEP_TOL, 'dstep', 'colstats' if nm == 'stats' else 'bn_running', *e.result(),
               reduction='bn_batch_stats ' + nm)
    # forward into a far output, backward with far dy and dx
    ys, y = _far_rows(M, K, ld, NAN)
    ops.bn_relu_apply(x, y, stats, float(M), gamma, beta, eps, 1)
    torch.cuda.synchronize()
    assert ys.intact()
    y_ref = D.bn_relu(x0, gamma, beta, eps, 1)
    record(margin, DSTEP_TOL, 'dstep', 'bn_fwd', *chunked_errors(y, lambda a, b: y_ref[a:b], CHUNK // K).result())
    mask = y > 0
    del y_ref
    dy0 = randn(M, K, seed=7305)
    ys.buf.fill_(1e3)
    y.copy_(dy0)                                        # (the output's storage now holds dy)
    dy = y
    nbytes = lib().raw('contrad_colstats_workspace_bytes')(ctypes.c_longlong(M), K, 1)
    ws, out2k = torch.empty((nbytes + 3) // 4, device=DEV), Flat((2, K), pad=4)
    lib().call('contrad_bn_relu_bwd_stats', P_(dy), P_(x), ctypes.c_longlong(M), K, ld, P_(stats), float(M), P_(gamma),
               P_(beta), eps, P_(out2k.view), P_(ws), ctypes.c_longlong(nbytes), ops._stream())
    dxs, dx = _far_rows(M, K, ld, NAN)
    lib().call('contrad_bn_relu_bwd_apply', P_(dy), P_(x), P_(dx), ctypes.c_longlong(M), K, ld, P_(stats), float(M),
               P_(gamma), P_(beta), eps, P_(out2k.view), ops._stream())
    torch.cuda.synchronize()
    assert dxs.intact() and out2k.intact()
    dx_ref, dg_ref, db_ref = D.bn_relu_bwd(dy0, x0, gamma, beta, eps, mask=mask)
    record(margin, DSTEP_TOL, 'dstep', 'bn_bwd', *chunked_errors(dx, lambda a, b: dx_ref[a:b], CHUNK // K).result(),
           reduction='bn_bwd dx')
    for nm, got, want in (('dgamma', out2k.view[1], dg_ref), ('dbeta', out2k.view[0], db_ref)):
        e = Err()
        e.add(got, want)
        record(margin, DSTEP_TOL, 'dstep', 'bn_bwd', *e.result(), reduction='bn_bwd ' + nm)
    del xs, ys, dxs, x, y, dy, dx, dx_ref, x0, dy0, mask
    release()


# ======================================================================================================================
# readers of dataset-sized storage
# ======================================================================================================================
def test_far_gather_u8_is_bitwise_totensor():
    """A device-resident uint8 set of 5 500 x 512^2 x 3 (4.3 GiB): images 0, n - 1 and those on both sides of byte 2^31 and
    of byte 2^32, flipped and not, bitwise ToTensor."""
    n, H, W = 5500, 512, 512
    img = H * W * 3
    src = torch.empty((n, H, W, 3), dtype=torch.uint8, device=DEV)
    step = 500
    for a in range(0, n, step):
        src[a:a + step] = torch.randint(0, 256, (min(step, n - a), H, W, 3), dtype=torch.uint8, device=DEV,
                                        generator=gen(7400 + a))
    idx = [0, n - 1, 2 ** 31 // img - 1, 2 ** 31 // img, 2 ** 31 // img + 1, 2 ** 32 // img - 1, 2 ** 32 // img,
           2 ** 32 // img + 1]
    assert idx[3] * img < 2 ** 31 < (idx[3] + 1) * img and idx[6] * img < 2 ** 32 < (idx[6] + 1) * img < n * img
    flips = [i % 2 == 1 for i in range(len(idx))]
    params = torch.tensor([[float(i), float(f)] for i, f in zip(idx, flips)], device=DEV)
    B = len(idx)
    big = torch.full((B * 3 * H * W + 2048,), NAN, device=DEV)
    out = big[1024:1024 + B * 3 * H * W].view(B, 3, H, W)
    got = ops.gather_u8_nchw(src, params, H, W, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(big[:1024]).all() and torch.isnan(big[-1024:]).all()
    want = src[torch.tensor(idx, device=DEV)].cpu().permute(0, 3, 1, 2).float().div(255)      # (ToTensor, on the host)
    f = torch.tensor(flips)
    want[f] = want[f].flip(-1)
    assert torch.equal(got.cpu().view(torch.int32), want.contiguous().view(torch.int32))
    del src, big, out, got
    release()


def test_far_linhead(margin):
    """linhead_fwd and linhead_wgrad_sgd on a feature bank of 131 081 x 8192 (4.0 GiB): random features, the float64 head
    in row chunks."""
    N, K, C = 131081, 8192, 10
    assert N * K * 4 > 2 ** 32 + K * 4 and N * K < 2 ** 31
    # (the inputs of tests/test_linhead_gpu.py, whose bounds this holds: post-ReLU features, nn.Linear's default init)
    F = Flat((N, K), nan=False)
    F.view.normal_(generator=gen(7501)).relu_().mul_(2.0 / math.sqrt(K))
    W = (torch.rand(C, K, device=DEV, generator=gen(7502)) * 2 - 1) / math.sqrt(K)
    b = (torch.rand(C, device=DEV, generator=gen(7503)) * 2 - 1) / math.sqrt(K)
    y = torch.randint(0, C, (N,), device=DEV, generator=gen(7504))
    logits, dlogits = Flat((N, C), pad=64), Flat((N, C), pad=64)
    ops.linhead_fwd(F.view, W, b, y=y, logits=logits.view, dlogits=dlogits.view)
    gW, gb = Flat((C, K), pad=64), Flat((C,), pad=4)
    ops.linhead_wgrad_sgd(F.view, dlogits.view, grad_weight=gW.view, grad_bias=gb.view)
    torch.cuda.synchronize()
    assert logits.intact() and dlogits.intact() and gW.intact() and gb.intact() and F.intact()
    step = 8192
    el, ed = Err(), Err()
    gW_ref = torch.zeros(C, K, dtype=torch.float64, device=DEV)
    gb_ref = torch.zeros(C, dtype=torch.float64, device=DEV)
    for a in range(0, N, step):
        r = LH.head_ref64(F.view[a:a + step], W, b, y[a:a + step], scale=1.0 / N)
        el.add(logits.view[a:a + step], r['logits'])
        ed.add(dlogits.view[a:a + step], r['dlogits'])
        gW_ref += r['gradW']
        gb_ref += r['gradb']
    record(margin, LINHEAD_TOL, 'linhead', 'logits', *el.result())
    record(margin, LINHEAD_TOL, 'linhead', 'dlogits', *ed.result())
    for nm, got, want in (('gradW', gW.view, gW_ref), ('gradb', gb.view, gb_ref)):
        e = Err()
        e.add(got, want)
        record(margin, LINHEAD_TOL, 'linhead', nm, *e.result(), reduction='linhead ' + nm)
    del F, logits, dlogits
    release()
