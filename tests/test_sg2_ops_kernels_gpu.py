"""GPU parity of the StyleGAN2 op kernels (csrc/stylegan2_ops.hip) against float64 (tests/sg2_ref64.py: plain float64
torch, none of this project's kernels), through the C ABI so that every operand lives in guard storage.  Each upfirdn2d
case names the launch form it is meant to reach (the first word of ``what`` for the modconv cases); tests/
test_aug_sg2_ref64_cpu.py restates upfirdn2d_launch's dispatch and fails if a form has no case or a case's declared form
is wrong.  Checked as tests/test_dstep_kernels_gpu.py does: max-norm and rel-L2 error over the whole tensor below the
1e-3 contract and a per-family bound (FAMILY_TOL, about 5x the worst observed on an MI355X, recorded through
``margin``); outputs and inputs inside NaN-filled storage with spare
floats on both sides (multiples of 4, so float4 operands stay 16-byte aligned), every output sentinel still NaN after
the call; exact results (grad 2, padding channels, two calls of a fixed-order reduction) compared bitwise.  The very
large cases (a non-temporal-store output of >= 256 MB, more than 65535 images) compare their first and last images."""
import math

import pytest
import torch

import sg2_ref64 as S
from contrad_amd import ops
from contrad_amd._lib import lib

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3

FAMILY_TOL = {                  # family: (max-norm, rel-L2)      observed worst (max-norm, rel-L2)
    'upfirdn': (1.2e-6, 4.6e-7),                # 2.3e-7, 9.1e-8
    'modconv': (6.3e-7, 2.9e-7),                # 1.3e-7, 5.8e-8
    'bias_act': (4e-7, 1.9e-7),                 # 8.0e-8, 3.9e-8
    'lincomb': (3.1e-7, 1.7e-7),                # 6.2e-8, 3.4e-8
    'scale_dev': (2.5e-7, 1.5e-7),              # 5.0e-8, 3.0e-8
    'pixelnorm': (4.9e-7, 3.3e-7),              # 9.9e-8, 6.6e-8
    'nhwc_scale': (1.9e-7, 1.3e-7),             # 3.8e-8, 2.5e-8
    'nhwc_dot': (1.7e-6, 1.7e-6),               # 3.5e-7, 3.4e-7
    'sumsq': (2.5e-7, 2.5e-7),                  # 1.4e-8, 1.4e-8 (one fp32 rounding of the result is 6e-8)
    'mbstd': (8e-6, 2.6e-6),                    # 1.6e-6, 5.3e-7
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
    margin('sg2 %s max-norm' % family, emax, tmax)
    margin('sg2 %s rel-L2' % family, el2, tl2)


class Guard(object):
    """``shape`` inside NaN-filled storage with ``pad`` spare floats on both sides (a multiple of 4)."""

    def __init__(self, shape, pad=None, fill=None):
        shape = tuple(shape)
        n = math.prod(shape)
        per = math.prod(shape[1:]) if len(shape) > 1 else 4
        self.pad = min((per + 3) // 4 * 4, 4096) + 4 if pad is None else pad
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
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(*shape, seed=0):
    return torch.randn(*shape, device=DEV, generator=gen(seed))


def call(name, *args):
    lib().call(name, *args, ops._stream())


def status(name, *args):
    return lib().raw(name)(*args, ops._stream())


# ======================================================================================================================
# upfirdn2d: the launch forms of upfirdn2d_launch
# ======================================================================================================================
BIG = 65540          # images: past the 65535 limit of grid.y
# (form, major, in_h, in_w, minor, (kh, kw), up_x, up_y, down_x, down_y, px0, px1, py0, py1, what)
UF_CASES = [
    ('u1d1_buf', 3, 17, 13, 32, (4, 4), 1, 1, 1, 1, 2, 1, 1, 2, 'blur, odd map, asymmetric pads'),
    ('u1d1_buf', 2, 19, 21, 4, (4, 4), 1, 1, 1, 1, -1, 2, 2, -1, 'negative pads, minor 4'),
    ('u1d1_buf', 16, 256, 256, 64, (4, 4), 1, 1, 1, 1, 1, 2, 2, 1, 'output 268 MB: non-temporal stores'),
    ('u1d1_ptr', BIG, 6, 5, 4, (4, 4), 1, 1, 1, 1, 1, 2, 2, 1, 'more than 65535 images'),
    ('u1d2_buf', 3, 17, 15, 32, (4, 4), 1, 1, 2, 2, 1, 1, 2, 1, 'decimating blur, odd map'),
    ('u1d2_buf', 2, 12, 10, 4, (4, 4), 1, 1, 2, 2, 2, -1, -1, 2, 'negative pads'),
    ('u1d2_ptr', BIG, 8, 7, 4, (4, 4), 1, 1, 2, 2, 1, 1, 1, 2, 'more than 65535 images'),
    ('u2d1_buf', 3, 9, 7, 32, (4, 4), 2, 2, 1, 1, 2, 1, 1, 2, 'upsampling FIR, pad parity (1, 0)'),
    ('u2d1_buf', 2, 7, 8, 4, (4, 4), 2, 2, 1, 1, 1, 2, 2, 1, 'pad parity (0, 1)'),
    ('u2d1_buf', 2, 5, 6, 8, (4, 4), 2, 2, 1, 1, 3, 0, 1, 2, 'pad parity (1, 1)'),
    ('u2d1_ptr', BIG, 4, 4, 4, (4, 4), 2, 2, 1, 1, 2, 1, 2, 1, 'more than 65535 images'),
    ('u2d1_planes', 6, 9, 11, 1, (4, 4), 2, 2, 1, 1, 2, 1, 1, 2, 'minor 1 planes'),
    ('u2d1_planes', 5, 8, 7, 1, (4, 4), 2, 2, 1, 1, 1, 2, 2, 1, 'minor 1, other parity'),
    ('strip4', 3, 11, 9, 8, (3, 5), 1, 1, 1, 1, 2, 1, 1, 0, '3 x 5 kernel, out_h 10: a partial last strip'),
    ('strip4', 2, 13, 6, 32, (4, 2), 1, 1, 1, 1, 0, 1, 2, -1, '4 x 2 kernel, negative pad'),
    ('generic4', 2, 9, 10, 8, (4, 4), 2, 1, 1, 1, 2, 1, 1, 2, 'up_x != up_y'),
    ('generic4', 2, 9, 7, 4, (2, 2), 2, 2, 1, 1, 0, 1, 1, 0, '2 x 2 kernel, upsampling'),
    ('generic4', 3, 5, 9, 4, (3, 3), 1, 1, 1, 1, 1, 1, 0, 0, '3 x 3 kernel, out_h 3 < 4'),
    ('generic1', 2, 11, 9, 3, (4, 4), 1, 1, 1, 1, 1, 2, 2, 1, 'minor 3 blur'),
    ('generic1', 2, 9, 8, 3, (4, 4), 2, 2, 1, 1, 2, 1, 1, 2, 'minor 3 upsampling'),
    ('generic1', 3, 10, 11, 1, (3, 4), 1, 1, 2, 2, 1, 0, 0, 1, 'minor 1 decimation, 3 x 4 kernel'),
]


def _kernel(kh, kw, seed):
    """A non-symmetric FIR kernel (the FLIP matters)."""
    return (torch.rand(kh, kw, device=DEV, generator=gen(seed)) + 0.1) / (kh * kw)


def _cfg(case):
    form, major, in_h, in_w, minor, (kh, kw), ux, uy, dx, dy, px0, px1, py0, py1, _ = case
    return major, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1


def _ends(t, n=2):
    return torch.cat([t[:n], t[-n:]]) if t.shape[0] > 2 * n else t


@pytest.mark.parametrize('case', UF_CASES, ids=lambda c: '%s-%s' % (c[0], c[-1].split(':')[0].replace(' ', '_')))
def test_upfirdn2d(margin, case):
    major, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = _cfg(case)
    out_h, out_w = S.out_size(in_h, in_w, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1)
    big = major * out_h * out_w * minor >= 2 ** 24 or major > 65535
    gk = Guard((kh, kw), pad=4, fill=_kernel(kh, kw, major + in_h))
    gx = Guard((major, in_h, in_w, minor), fill=randn(major, in_h, in_w, minor, seed=in_w))
    oshape = (major, out_h, out_w, minor)
    cfg = (major, in_h, in_w, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1)
    what = '%s %s' % (case[0], cfg)
    E = _ends if big else (lambda t: t)            # (the very large launches: first and last images only)
    ref = S.upfirdn2d(E(gx.view), gk.view, ux, uy, dx, dy, px0, px1, py0, py1)
    go = Guard(oshape)
    call('contrad_upfirdn2d', P_(gx.view), P_(gk.view), P_(go.view), *cfg)
    torch.cuda.synchronize()
    assert go.intact() and gx.intact()
    check(margin, 'upfirdn', what, E(go.view), ref)
    del go
    # the fused epilogue with and without each operand: (addend, out, out2 + act_ref)
    slope, gain = 0.2, 1.4142135
    add = Guard(oshape, fill=randn(*oshape, seed=3))
    aref = Guard(oshape, fill=randn(*oshape, seed=4))
    for has_add, has_out, has_out2 in ((1, 1, 1),) if big else ((1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 0, 1)):
        go = Guard(oshape) if has_out else None
        go2 = Guard(oshape) if has_out2 else None
        call('contrad_upfirdn2d_fused', P_(gx.view), P_(gk.view), P_(go.view if go else None), *cfg,
             P_(add.view if has_add else None), P_(aref.view if has_out2 else None), ctypes_float(slope),
             ctypes_float(gain), P_(go2.view if go2 else None))
        torch.cuda.synchronize()
        r1, r2 = S.fused_epilogue(ref, E(add.view) if has_add else None, E(aref.view) if has_out2 else None, f32(slope),
                                  f32(gain))
        tag = ' epilogue addend=%d out=%d out2=%d' % (has_add, has_out, has_out2)
        if go:
            assert go.intact()
            check(margin, 'upfirdn', what + tag + ': out', E(go.view), r1)
        if go2:
            assert go2.intact()
            check(margin, 'upfirdn', what + tag + ': out2', E(go2.view), r2)
        del go, go2


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def ctypes_float(v):
    import ctypes
    return ctypes.c_float(v)


# (N, in_h, in_w, K, px0, px1, py0, py1, demod, noise, post, what)
MODCONV_CASES = [
    (3, 17, 15, 32, 2, 1, 1, 2, True, True, True, 'u1d1_buf, every term'),
    (2, 9, 11, 8, 1, 1, 1, 1, False, False, False, 'u1d1_buf, bias alone'),
    (2, 13, 9, 12, 2, 1, 1, 2, True, False, True, 'u1d1_buf, no noise'),
    (BIG, 5, 4, 4, 1, 2, 2, 1, True, True, True, 'u1d1_ptr: more than 65535 images'),
]


@pytest.mark.parametrize('case', MODCONV_CASES, ids=lambda c: c[-1].split(',')[0].split(':')[0] + '-%d' % c[3])
def test_upfirdn2d_modconv(margin, case):
    N, in_h, in_w, K, px0, px1, py0, py1, dm, nz, po, what = case
    out_h, out_w = S.out_size(in_h, in_w, 4, 4, 1, 1, 1, 1, px0, px1, py0, py1)
    gk = Guard((4, 4), pad=4, fill=_kernel(4, 4, K))
    gx = Guard((N, in_h, in_w, K), fill=randn(N, in_h, in_w, K, seed=K))
    demod = Guard((N, K), fill=torch.rand(N, K, device=DEV, generator=gen(1)) + 0.5) if dm else None
    noise = Guard((N, out_h, out_w), fill=randn(N, out_h, out_w, seed=2)) if nz else None
    nw = Guard((1,), pad=4, fill=torch.tensor([0.3], device=DEV)) if nz else None
    bias = Guard((K,), pad=4, fill=randn(K, seed=5))
    post = Guard((N, K), fill=torch.rand(N, K, device=DEV, generator=gen(6)) + 0.5) if po else None
    gy = Guard((N, out_h, out_w, K))
    v = lambda g: None if g is None else g.view
    call('contrad_upfirdn2d_modconv', P_(gx.view), P_(gk.view), P_(gy.view), N, in_h, in_w, K, px0, px1, py0, py1,
         P_(v(demod)), P_(v(noise)), P_(v(nw)), P_(bias.view), P_(v(post)))
    torch.cuda.synchronize()
    assert gy.intact()
    E = _ends if N > 65535 else (lambda t: t)
    e = lambda g: None if g is None else E(g.view)
    up = S.upfirdn2d(E(gx.view), gk.view, 1, 1, 1, 1, px0, px1, py0, py1)
    ref = S.modconv_epilogue(up, bias.view, e(demod), e(noise), v(nw), e(post))
    check(margin, 'modconv', what, E(gy.view), ref)


# (N, HW, K, demod, noise (0 none, 1 with noise_w, 2 without noise_w), post, in place, what)
EPI_CASES = [
    (3, 37, 4, True, 1, True, False, 'K = 4, every term'),
    (2, 50, 4, False, 0, False, False, 'K = 4, bias alone'),
    (2, 19, 512, True, 0, True, False, 'K = 512, no noise'),
    (2, 19, 512, False, 1, False, False, 'K = 512, noise alone'),
    (2, 23, 8, True, 2, False, False, 'noise without noise_w: no noise term'),
    (3, 21, 12, True, 1, True, True, 'in place'),
    (5, 4096, 1024, True, 1, True, False, 'past the 16384-block grid cap'),
]


@pytest.mark.parametrize('case', EPI_CASES, ids=lambda c: 'N%d-HW%d-K%d-%s' % (c[:3] + (c[-1].replace(' ', '_'),)))
def test_modconv_epilogue(margin, case):
    """contrad_modconv_epilogue (the tail of every non-upsampling StyledConv): y = sqrt2 * lrelu_0.2(x * demod +
    noise_w * noise + bias) [* post], each optional operand present and absent."""
    N, HW, K, dm, nz, po, inplace, what = case
    if 'grid cap' in what:
        assert N * HW * K // 4 > 16384 * 256
    gx = Guard((N, HW, K), fill=randn(N, HW, K, seed=K + HW))
    x0 = gx.view.clone()
    demod = Guard((N, K), fill=torch.rand(N, K, device=DEV, generator=gen(1)) + 0.5) if dm else None
    noise = Guard((N, HW), fill=randn(N, HW, seed=2)) if nz else None
    nw = Guard((1,), pad=4, fill=torch.tensor([0.3], device=DEV)) if nz == 1 else None
    bias = Guard((K,), pad=4, fill=randn(K, seed=5))
    post = Guard((N, K), fill=torch.rand(N, K, device=DEV, generator=gen(6)) + 0.5) if po else None
    gy = gx if inplace else Guard((N, HW, K))
    v = lambda g: None if g is None else g.view
    call('contrad_modconv_epilogue', P_(gx.view), P_(v(demod)), P_(v(noise)), P_(v(nw)), P_(bias.view), P_(v(post)),
         P_(gy.view), N, HW, K)
    torch.cuda.synchronize()
    assert gy.intact()
    nzv = None if noise is None else noise.view.view(N, HW, 1)
    ref = S.modconv_epilogue(x0.view(N, HW, 1, K), bias.view, v(demod), nzv, v(nw), v(post)).view(N, HW, K)
    check(margin, 'modconv', what, gy.view, ref)


def test_modconv_epilogue_rejects_ragged_channels():
    x = torch.zeros(2, 3, 6, device=DEV)
    b = torch.zeros(8, device=DEV)
    rc = status('contrad_modconv_epilogue', P_(x), P_(None), P_(None), P_(None), P_(b), P_(None), P_(x), 2, 3, 6)
    assert rc == -22


# ======================================================================================================================
# fused_bias_act, lincomb, scale_dev
# ======================================================================================================================
# (n, step_b, size_b, what): bias b[(i / step_b) % size_b]
BIAS_CASES = [(4103, 1, 24, 'NHWC bias'), (6 * 37 * 5, 37, 5, 'NCHW bias'), (4194304 + 9, 1, 512, 'grid-stride')]


@pytest.mark.parametrize('case', BIAS_CASES, ids=lambda c: 'n%d' % c[0])
@pytest.mark.parametrize('act', [1, 3])
@pytest.mark.parametrize('grad', [0, 1, 2])
def test_fused_bias_act(margin, case, act, grad):
    n, step_b, size_b, what = case
    gx = Guard((n,), fill=randn(n, seed=n))
    gb = Guard((size_b,), pad=4, fill=randn(size_b, seed=size_b))
    gr = Guard((n,), fill=randn(n, seed=n + 1))
    gy = Guard((n,))
    alpha, scale = 0.2, 1.4142135
    call('contrad_fused_bias_act', P_(gx.view), P_(gb.view), P_(gr.view), P_(gy.view), n, step_b, size_b, act, grad,
         ctypes_float(alpha), ctypes_float(scale))
    torch.cuda.synchronize()
    assert gy.intact()
    if grad == 2:
        assert torch.equal(gy.view, torch.zeros(n, device=DEV))
        return
    ref = S.fused_bias_act(gx.view, gb.view, gr.view, step_b, size_b, act, grad, f32(alpha), f32(scale))
    check(margin, 'bias_act', '%s act=%d grad=%d' % (what, act, grad), gy.view, ref)


@pytest.mark.parametrize('n', [1, 4097, 4 * 256 * 16384 + 7])
def test_lincomb(margin, n):
    gx, gz = Guard((n,), fill=randn(n, seed=1)), Guard((n,), fill=randn(n, seed=2))
    gy = Guard((n,))
    a, b = 0.7071068, -1.3
    call('contrad_lincomb', P_(gx.view), P_(gz.view), P_(gy.view), n, ctypes_float(a), ctypes_float(b))
    torch.cuda.synchronize()
    assert gy.intact()
    check(margin, 'lincomb', 'n=%d' % n, gy.view, S.lincomb(gx.view, gz.view, f32(a), f32(b)))


@pytest.mark.parametrize('n', [3, 4099, 4096 * 2048 + 5])
def test_scale_dev(margin, n):
    gx = Guard((n,), fill=randn(n, seed=3))
    gs = Guard((1,), pad=4, fill=torch.tensor([-0.37], device=DEV))
    gy = Guard((n,))
    c = 2.5
    call('contrad_scale_dev', P_(gx.view), P_(gs.view), ctypes_float(c), P_(gy.view), n)
    torch.cuda.synchronize()
    assert gy.intact()
    check(margin, 'scale_dev', 'n=%d' % n, gy.view, S.scale_dev(gx.view, gs.view, f32(c)))


# ======================================================================================================================
# pixelnorm, nhwc_scale, nhwc_dot
# ======================================================================================================================
@pytest.mark.parametrize('MK', [(7, 1), (13, 512), (5, 513), (6, 512)], ids=lambda s: 'M%d-K%d' % s)
def test_pixelnorm(margin, MK):
    M, K = MK
    x = randn(M, K, seed=M * K)
    if MK == (6, 512):
        x[0] = 0.
        x[3] = 0.                                  # rows of zeros: rsqrt(1e-8) * 0
    gx, gy = Guard((M, K), fill=x), Guard((M, K))
    call('contrad_pixelnorm', P_(gx.view), P_(gy.view), M, K)
    torch.cuda.synchronize()
    assert gy.intact()
    check(margin, 'pixelnorm', 'M=%d K=%d' % MK, gy.view, S.pixelnorm(gx.view, M, K))
    if MK == (6, 512):
        assert torch.equal(gy.view[0], torch.zeros(K, device=DEV)) and torch.equal(gy.view[3], gy.view[0])


@pytest.mark.parametrize('NHC', [(3, 37, 12), (2, 4097, 4), (4, 65536, 68)], ids=lambda s: 'N%d-HW%d-C%d' % s)
def test_nhwc_scale(margin, NHC):
    N, HW, C = NHC
    gx = Guard((N, HW, C), fill=randn(N, HW, C, seed=C))
    gs = Guard((N, C), fill=randn(N, C, seed=C + 1))
    gy = Guard((N, HW, C))
    call('contrad_nhwc_scale', P_(gx.view), P_(gs.view), P_(gy.view), N, HW, C)
    torch.cuda.synchronize()
    assert gy.intact()
    check(margin, 'nhwc_scale', 'N=%d HW=%d C=%d' % NHC, gy.view, S.nhwc_scale(gx.view, gs.view, N, HW, C))


def test_nhwc_scale_rejects_ragged_channels():
    x = torch.zeros(2, 3, 6, device=DEV)
    s = torch.zeros(2, 6, device=DEV)
    assert status('contrad_nhwc_scale', P_(x), P_(s), P_(x), 2, 3, 6) == -22


def nhwc_dot_segments(N, HW):
    return max(1, min(-(-HW // 64), -(-2048 // N)))


# (N, HW, C, b_per_channel, what)
DOT_CASES = [
    (3, 200, 4, 0, 'C = 4, below the cap'),
    (3, 200, 4, 1, 'C = 4, b per channel'),
    (64, 4096, 4, 1, 'C = 4 at the cap'),
    (16, 16384, 8, 0, 'at the cap, b broadcast'),
    (2, 100, 1024, 1, 'C = 1024 below the cap'),
    (1024, 129, 1024, 0, 'C = 1024 at the cap'),
    (3, 77, 12, 1, 'C = 12: lanes_c 4, one idle'),
]


@pytest.mark.parametrize('case', DOT_CASES, ids=lambda c: 'N%d-HW%d-C%d-b%d' % c[:4])
def test_nhwc_dot(margin, case):
    N, HW, C, bpc, what = case
    S_ = nhwc_dot_segments(N, HW)
    capped = S_ < -(-HW // 64)
    assert capped == ('at the cap' in what)
    ga = Guard((N, HW, C), fill=randn(N, HW, C, seed=HW))
    gb = Guard((N, HW, C) if bpc else (N, HW), fill=randn(*((N, HW, C) if bpc else (N, HW)), seed=HW + 1))
    nbytes = lib().raw('contrad_nhwc_dot_workspace_bytes')(N, HW, C)
    assert nbytes == N * S_ * C * 4
    gw = Guard((nbytes // 4,), pad=4)
    go, go2 = Guard((N, C)), Guard((N, C))
    call('contrad_nhwc_dot', P_(ga.view), P_(gb.view), P_(go.view), N, HW, C, bpc, P_(gw.view), nbytes)
    call('contrad_nhwc_dot', P_(ga.view), P_(gb.view), P_(go2.view), N, HW, C, bpc, P_(gw.view), nbytes)
    torch.cuda.synchronize()
    assert go.intact() and go2.intact() and gw.intact()
    check(margin, 'nhwc_dot', '%s S=%d' % (what, S_), go.view, S.nhwc_dot(ga.view, gb.view, N, HW, C, bpc))
    assert torch.equal(go.view, go2.view)            # a fixed summation order


def test_nhwc_dot_rejects_unsupported_channels():
    a = torch.zeros(2, 3, 1028, device=DEV)
    w = torch.zeros(4096, device=DEV)
    for C in (6, 1028):
        assert status('contrad_nhwc_dot', P_(a), P_(a), P_(w), 2, 3, C, 1, P_(w), 4 * 4096) == -22, C


# ======================================================================================================================
# sumsq, minibatch-stddev
# ======================================================================================================================
@pytest.mark.parametrize('n', [1, 4095, 4096 * 1024 + 3])
def test_sumsq(margin, n):
    gx = Guard((n,), fill=randn(n, seed=n))
    nbytes = lib().raw('contrad_sumsq_workspace_bytes')(n)
    assert nbytes == min(-(-n // 4096), 1024) * 4
    gw = Guard((nbytes // 4,), pad=4)
    go, go2 = Guard((1,), pad=4), Guard((1,), pad=4)
    scale = 0.125
    call('contrad_sumsq', P_(gx.view), n, ctypes_float(scale), P_(go.view), P_(gw.view), nbytes)
    call('contrad_sumsq', P_(gx.view), n, ctypes_float(scale), P_(go2.view), P_(gw.view), nbytes)
    torch.cuda.synchronize()
    assert go.intact() and go2.intact() and gw.intact()
    check(margin, 'sumsq', 'n=%d' % n, go.view, S.sumsq(gx.view, scale).view(1))
    assert torch.equal(go.view, go2.view)


# (B, P, C, Cp)
MBSTD_CASES = [(1, 16, 32, 48), (4, 16, 32, 48), (8, 16, 512, 528), (12, 16, 32, 48), (16, 16, 512, 528),
               (8, 64, 32, 48), (12, 64, 512, 528)]


@pytest.mark.parametrize('case', MBSTD_CASES, ids=lambda c: 'B%d-P%d-C%d' % c[:3])
def test_minibatch_stddev(margin, case):
    B, P, C, Cp = case
    gx = Guard((B, P, C), fill=randn(B, P, C, seed=B * P + C))
    ggy = Guard((B, P, Cp), fill=randn(B, P, Cp, seed=B + C))
    gh = Guard((B, P, C), fill=randn(B, P, C, seed=B + P))
    what = 'B=%d P=%d C=%d Cp=%d' % case
    # mode 0
    go = Guard((B, P, Cp))
    call('contrad_minibatch_stddev', 0, P_(gx.view), P_(None), P_(None), P_(go.view), P_(None), B, P, C, Cp)
    torch.cuda.synchronize()
    assert go.intact()
    check(margin, 'mbstd', what + ' mode 0', go.view, S.mbstd(0, gx.view, B, P, C, Cp))
    assert torch.equal(go.view[:, :, :C], gx.view)
    assert torch.equal(go.view[:, :, C + 1:], torch.zeros(B, P, Cp - C - 1, device=DEV))
    # mode 1
    g1 = Guard((B, P, C))
    call('contrad_minibatch_stddev', 1, P_(gx.view), P_(ggy.view), P_(None), P_(g1.view), P_(None), B, P, C, Cp)
    torch.cuda.synchronize()
    assert g1.intact()
    check(margin, 'mbstd', what + ' mode 1', g1.view, S.mbstd(1, gx.view, B, P, C, Cp, gy=ggy.view))
    # mode 2
    g2, g2b = Guard((B, P, C)), Guard((B, P, Cp))
    call('contrad_minibatch_stddev', 2, P_(gx.view), P_(ggy.view), P_(gh.view), P_(g2.view), P_(g2b.view), B, P, C, Cp)
    torch.cuda.synchronize()
    assert g2.intact() and g2b.intact()
    r2, r2b = S.mbstd(2, gx.view, B, P, C, Cp, gy=ggy.view, h=gh.view)
    if B > 1:                                      # (one sample: var = 0, the gradient is exactly 0)
        check(margin, 'mbstd', what + ' mode 2 d/dx', g2.view, r2)
    else:
        assert g2.view.abs().max().item() == 0.0
    check(margin, 'mbstd', what + ' mode 2 d/dgy', g2b.view, r2b)
    assert torch.equal(g2b.view[:, :, :C], gh.view)
    assert torch.equal(g2b.view[:, :, C + 1:], torch.zeros(B, P, Cp - C - 1, device=DEV))


# ======================================================================================================================
# modconv_tables_kernel, modconv_demod_kernel: the generator's weight tables and demodulation factors, one launch each
# ======================================================================================================================
U24 = 2.0 ** -24
# (Cout, Cin, k, transposed, demodulate): ragged 32 x 32 tiles in both orientations, 1x1 and 3x3, a 3-channel ToRGB
TABLE_CASES = [(64, 32, 3, False, True), (32, 64, 3, True, True), (3, 48, 1, True, False), (40, 36, 3, False, True),
               (70, 33, 3, True, True), (128, 256, 1, False, False)]


def test_modconv_tables_match_float64():
    """contrad_modconv_tables (six layers, one launch).  A packed weight is one fp32 product w * scale: it must equal the
    float64 product rounded once.  A demodulation table entry is a sum of T <= 9 squares of those products: all terms are
    positive, so any order and fused or unfused multiply-adds stay within (T + 3) * 2^-24 of the float64 sum, relative, element
    by element (one rounding of the product entering squared, one per square, T - 1 additions).  Packed weights are column
    slices of wider NaN buffers with a spare row either side: every sentinel must survive."""
    g = torch.Generator().manual_seed(8)
    layers, refs, guards = [], [], []
    for co, ci, k, tr, dm in TABLE_CASES:
        w = torch.randn(co, ci, k, k, generator=g)
        scale = float(torch.tensor(1.0 / math.sqrt(ci * k * k), dtype=torch.float32))
        rows, cols = (k * k * co, ci) if tr else (k * k * ci, co)
        wbuf = torch.full((rows + 2, cols + 8), NAN, device=DEV)
        gq = Guard((ci, co)) if dm else None
        gw = Guard(tuple(w.shape), fill=w.to(DEV))
        layers.append((gw.view, wbuf[1:-1, 4:4 + cols], gq.view if dm else None, tr, scale))
        ws = (w.double() * scale).float().double()                # the fp32 product, exactly
        ref_wp = (ws.permute(2, 3, 0, 1).reshape(k * k * co, ci) if tr else ws.permute(2, 3, 1, 0).reshape(k * k * ci, co))
        refs.append((ref_wp, ws.pow(2).sum((2, 3)).t() if dm else None, k * k))
        guards.append((wbuf, gq, gw, w))
    ops.modconv_tables(layers)
    torch.cuda.synchronize()
    for (wd, wp, wsq, tr, scale), (ref_wp, ref_wsq, T), (wbuf, gq, gw, w) in zip(layers, refs, guards):
        assert torch.equal(wp.cpu().double(), ref_wp)
        inner = torch.zeros_like(wbuf, dtype=torch.bool)
        inner[1:-1, 4:4 + wp.shape[1]] = True
        assert bool(torch.isnan(wbuf[~inner]).all()), 'a packed weight wrote outside its columns'
        assert gw.intact() and torch.equal(wd.cpu(), w)
        if wsq is not None:
            assert gq.intact()
            err = (wsq.cpu().double() - ref_wsq).abs() / ref_wsq
            assert err.max().item() <= (T + 3) * U24, (tr, T, err.max().item())


@pytest.mark.parametrize('B', [5, 16, 70])
def test_modconv_demod_matches_float64(B):
    """contrad_modconv_demod: out = rsqrt(style^2 @ wsq + eps) of six layers from one launch (ragged 64-channel output chunks,
    ragged 16-sample blocks, Cin of exactly one 512-channel LDS chunk, two, and a ragged second one).  Every term of the sum
    is non-negative, so in any order with fused or unfused multiply-adds it is within (Cin + 2) * 2^-24 of the float64 sum,
    relative (one rounding per square, at most one per product, Cin - 1 additions, eps); the reciprocal square root halves that
    and adds its own rounding and the hardware approximation's error, allowed 4 * 2^-24 here."""
    g = torch.Generator().manual_seed(9)
    jobs, refs, guards = [], [], []
    for cin, k in [(512, 512), (32, 64), (100, 36), (1024, 300), (600, 70), (64, 3)]:
        st = torch.randn(B, cin, generator=g)
        wsq = torch.rand(cin, k, generator=g) / cin
        gs, gw, go = Guard((B, cin), fill=st.to(DEV)), Guard((cin, k), fill=wsq.to(DEV)), Guard((B, k))
        jobs.append((gs.view, gw.view, go.view))
        refs.append((torch.rsqrt((st.double() ** 2) @ wsq.double() + 1e-8), cin))
        guards.append((gs, gw, go))
    ops.modconv_demod(jobs, 1e-8)
    torch.cuda.synchronize()
    for (st, wsq, out), (ref, cin), gds in zip(jobs, refs, guards):
        assert all(gd.intact() for gd in gds)
        err = (out.cpu().double() - ref).abs() / ref
        assert torch.isfinite(out).all() and err.max().item() <= ((cin + 2) / 2 + 4) * U24, (cin, err.max().item())
