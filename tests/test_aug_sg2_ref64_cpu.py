"""CPU checks of the float64 references tests/aug_ref64.py and tests/sg2_ref64.py (no GPU): against the fp32 oracle, the
reference's goldens (tests/golden/augment.npz, the ufd_* / flr_* arrays of stylegan2_d.npz) and, where the kernels
restate them in closed form, against CPU float64 autograd to 1e-12.  Then the coverage of the two GPU parity modules
(tests/test_augment_kernels_gpu.py, tests/test_sg2_ops_kernels_gpu.py): the launchers' dispatch rules are restated here,
and the test fails if a launch form has no GPU case or a case's declared form differs from the rule."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_ref64 as A
import sg2_ref64 as S
from oracle import contrad_oracle as O
from oracle import stylegan2_oracle as SO

_HERE = os.path.dirname(os.path.abspath(__file__))
f64 = torch.float64


def T(a):
    return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def golden_params(g, tag):
    B = g[tag + '_x'].shape[0]
    P = torch.zeros(B, 16)
    th = T(g[tag + '_p_theta'])
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = th[:, 0, 0], th[:, 1, 1], th[:, 0, 2], th[:, 1, 2]
    P[:, 4] = T(g[tag + '_p_flip_sign'])
    P[:, 5] = T(g[tag + '_p_jitter_mask'])
    P[:, 6] = T(g[tag + '_p_f_contrast'])
    P[:, 7], P[:, 8], P[:, 9] = T(g[tag + '_p_f_h']), T(g[tag + '_p_f_s']), T(g[tag + '_p_f_v'])
    P[:, 10] = T(g[tag + '_p_gray_mask'])
    for col, key in ((11, '_p_blur_mask'), (12, '_p_cut_mask'), (13, '_p_cut_h'), (14, '_p_cut_w')):
        if tag + key in g.files:
            P[:, col] = T(g[tag + key]).float()
    return P, int(bool(g[tag + '_p_contrast_first']))


def random_params(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    np.random.seed(seed)
    P = torch.zeros(B, 16)
    th = O.sample_resized_crop_theta(B, H, W, (0.08, 1.0), (3. / 4., 4. / 3.))
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = th[:, 0, 0], th[:, 1, 1], th[:, 0, 2], th[:, 1, 2]
    P[:, 4] = torch.tensor([1., -1.] * B)[:B]
    P[:, 5] = torch.tensor([1., 1., 0.] * B)[:B]
    P[:, 6] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    P[:, 7] = torch.empty(B).uniform_(-0.2, 0.2, generator=g)
    P[:, 8] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    P[:, 9] = torch.empty(B).uniform_(0.2, 1.8, generator=g)
    P[:, 10] = torch.tensor([0., 1., 0., 0.] * B)[:B]
    return P


def oracle_params(P, cf):
    B = P.shape[0]
    th = torch.zeros(B, 2, 3)
    th[:, 0, 0], th[:, 1, 1], th[:, 0, 2], th[:, 1, 2] = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    return {'theta': th, 'flip_sign': P[:, 4], 'jitter_mask': P[:, 5], 'contrast_first': bool(cf),
            'f_contrast': P[:, 6], 'f_h': P[:, 7], 'f_s': P[:, 8], 'f_v': P[:, 9], 'gray_mask': P[:, 10]}


# ======================================================================================================================
# aug_ref64
# ======================================================================================================================
def test_aug_stages_against_goldens(golden):
    g = golden('augment')
    for tag in ('c10a', 'c10b'):
        x = T(g[tag + '_x'])
        P, cf = golden_params(g, tag)
        P1 = P.clone(); P1[:, 4] = 1.
        assert maxerr(A.crop_flip(x, P1), g[tag + '_stage_crop']) < 1e-5
        assert maxerr(A.crop_flip(x, P), g[tag + '_stage_flip']) < 1e-5
        assert maxerr(A.simclr(x, P, cf, 1), g[tag + '_out']) < 1e-5, tag
    B = g['hsv_x'].shape[0]
    P = torch.zeros(B, 16)
    P[:, 7], P[:, 8], P[:, 9] = T(g['hsv_fh']), T(g['hsv_fs']), T(g['hsv_fv'])
    assert maxerr(A.hsv_jitter(T(g['hsv_x']).double(), P), g['hsv_adjusted']) < 1e-5
    assert maxerr(A.rgb2hsv(T(g['hsv_x']).double()), g['hsv_hsv']) < 1e-5
    P = torch.zeros(g['con_x'].shape[0], 16)
    P[:, 6] = T(g['con_f'])
    assert maxerr(torch.clamp(A.contrast_pre(T(g['con_x']).double(), P, 1), 0, 1), g['con_out']) < 1e-6


@pytest.mark.parametrize('tag', ['hq', 'cut'])
def test_aug_blur_cutout_pipeline_against_goldens(golden, tag):
    g = golden('augment')
    x = T(g[tag + '_x'])
    P, cf = golden_params(g, tag)
    H = x.shape[2]
    R = int((H // 10) / 2)
    k1 = O.gaussian_kernel1d(2 * R + 1, float(g[tag + '_p_sigma']))
    y = A.gaussian_blur(A.simclr(x, P, cf, 1), P, k1)
    if tag == 'cut':
        y = A.cutout(y, P, int(g['cut_p_cut_length']))
    assert maxerr(y, g[tag + '_out']) < 3e-5          # (the golden's fp32 contrast at f up to 1.8, then a 7 x 7 blur)


@pytest.mark.parametrize('cf', [0, 1])
def test_aug_against_fp32_oracle_nonsquare(cf):
    B, H, W = 6, 20, 28
    P = random_params(B, H, W, 3 + cf)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(4))
    p = oracle_params(P, cf)
    assert maxerr(A.simclr(x, P, cf, 1), O.simclr_apply(x, p)) < 1e-5
    # column 15 (contrast_first = -1) picks the order per sample
    P[:, 15] = torch.tensor([1., 0., 0., 1., 1., 0.])
    y = A.simclr(x, P, -1, 1)
    y1, y0 = A.simclr(x, P, 1, 1), A.simclr(x, P, 0, 1)
    for b in range(B):
        assert torch.equal(y[b], (y1 if P[b, 15] else y0)[b])
    # the backward against the oracle's fp32 autograd (straight-through HSV)
    gout = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(5))
    xr = x.clone().requires_grad_()
    O.simclr_apply(xr, p).backward(gout)
    ref = A.simclr_bwd(x, P, gout, cf, 1)
    assert ((ref - xr.grad.double()).norm() / ref.norm()).item() < 1e-5


@pytest.mark.parametrize('cf', [-1, 0, 1])
@pytest.mark.parametrize('hc', [0, 1])
def test_aug_backward_closed_form(cf, hc):
    """The kernels' closed form (csrc/augment.hip, simclr_small_bwd_kernel): gray backward, the clamp mask gm, contrast
    backward f * gm + (1 - f) * mean(gm), HSV straight-through, then the gather transpose Wy^T G Wx -- against float64
    autograd to 1e-12, on a non-square image with a mirrored and a zoom-out crop."""
    B, H, W = 6, 12, 17
    P = random_params(B, H, W, 11)
    P[2, 0] = -P[2, 0]
    P[3, 0], P[3, 1], P[3, 3] = 1.25, 1.3, -0.4
    P[:, 15] = torch.tensor([1., 0., 1., 0., 0., 1.])
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(12))
    gout = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(13))
    want = A.simclr_bwd(x, P, gout, cf, hc)
    assert (A.simclr_bwd_closed(x, P, gout, cf, hc) - want).abs().max().item() < 1e-12


@pytest.mark.parametrize('hc', [0, 1])
def test_resolve_kinks_finds_the_flipped_elements(hc):
    """Inputs exactly 0 or 1 under the identity crop sit on the clamp (the set K).  A gradient computed with the mask of
    two of them flipped is matched exactly by resolve_kinks, which flips those two and no others."""
    B, H, W = 3, 8, 8
    P = torch.zeros(B, 16)
    P[:, 0] = 1.; P[:, 1] = 1.; P[:, 4] = 1.; P[:, 5] = 1.; P[:, 6] = 1.3; P[:, 8] = 1.; P[:, 9] = 1.
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1)) * 0.5 + 0.25
    x[0, 1, 2, 3] = 0.
    x[2, 0, 5, 5] = 1.
    x[1, 2, 4, 1] = 0.
    gout = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(2))
    if hc:                                            # (with contrast the planted values move off the clamp: put the
        P[:, 6] = 1.0                                 # factor at 1, so pre = x and the three elements stay in K)
    _, pre = A.simclr_parts(x.double(), P, 1, hc)
    passing = (pre >= 0) & (pre <= 1)
    flipped = passing.clone()
    flipped[0, 1, 2, 3] = False
    flipped[2, 0, 5, 5] = False
    got = A.simclr_bwd_closed(x, P, gout, 1, hc, flipped)
    ref, nK, flips = A.resolve_kinks(x, P, gout, 1, hc, got)
    assert nK == 3 and flips == 2
    assert (ref - got).abs().max().item() < 1e-12
    ref0, _, flips0 = A.resolve_kinks(x, P, gout, 1, hc, A.simclr_bwd(x, P, gout, 1, hc))
    assert flips0 == 0 and (ref0 - A.simclr_bwd(x, P, gout, 1, hc)).abs().max().item() < 1e-12


def test_blur_adjoint_identity():
    B, H, W, R = 3, 13, 11, 5
    P = torch.zeros(B, 16)
    P[:, 11] = torch.tensor([1., 0., 1.])
    k1 = O.gaussian_kernel1d(2 * R + 1, 1.3)
    x = torch.randn(B, 3, H, W, dtype=f64)
    g = torch.randn(B, 3, H, W, dtype=f64)
    lhs = (A.gaussian_blur(x, P, k1) * g).sum()
    rhs = (x * A.gaussian_blur_bwd(g, P, k1)).sum()
    assert abs((lhs - rhs).item()) < 1e-12 * abs(lhs.item()) + 1e-12
    # separable (2R+1)-tap correlation with reflect padding, one axis at a time
    gk = k1.double()
    xp = F.pad(x, [R, R, 0, 0], mode='reflect')
    hx = sum(gk[t] * xp[..., t:t + W] for t in range(2 * R + 1))
    hp = F.pad(hx, [0, 0, R, R], mode='reflect')
    sep = sum(gk[t] * hp[:, :, t:t + H, :] for t in range(2 * R + 1))
    y = A.gaussian_blur(x, P, k1)
    assert (y[0] - sep[0]).abs().max().item() < 1e-12 and torch.equal(y[1], x[1])


def test_cutout_against_oracle():
    B, H, W, L = 4, 16, 12, 5
    x = torch.rand(B, 3, H, W)
    P = torch.zeros(B, 16)
    P[:, 12] = 1.
    P[:, 13] = torch.tensor([0., 15., 7., 3.])
    P[:, 14] = torch.tensor([0., 11., 0., 6.])
    want = O.cutout(x, P[:, 13].long(), P[:, 14].long(), L)
    assert torch.equal(A.cutout(x, P, L), want)


# ======================================================================================================================
# sg2_ref64
# ======================================================================================================================
def test_upfirdn2d_against_goldens(golden):
    g = golden('stylegan2_d')
    x = T(g['ufd_x']).permute(0, 2, 3, 1)
    for tag in ('blur22', 'blur11', 'up2', 'down2', 'neg', 'k2'):
        up, down, p0, p1 = [int(v) for v in g['ufd_%s_cfg' % tag]]
        y = S.upfirdn2d(x, T(g['ufd_%s_k' % tag]), up, up, down, down, p0, p1, p0, p1)
        assert maxerr(y.permute(0, 3, 1, 2), g['ufd_%s_out' % tag]) < 1e-6, tag
    xs = x.reshape(-1)
    b = T(g['flr_b'])
    C = b.numel()
    y = S.fused_bias_act(xs, b, None, 1, C, 3, 0, 0.2, 2 ** 0.5).view(x.shape)
    assert maxerr(y.permute(0, 3, 1, 2), g['flr_out']) < 1e-6


def _upfirdn_loop(x, k, ux, uy, dx, dy, px0, px1, py0, py1):
    M, H, W, C = x.shape
    kh, kw = k.shape
    oh, ow = S.out_size(H, W, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1)
    out = torch.zeros(M, oh, ow, C, dtype=f64)
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(kh):
                for kx in range(kw):
                    py, px = oy * dy + ky - py0, ox * dx + kx - px0
                    if py < 0 or px < 0 or py % uy or px % ux or py // uy >= H or px // ux >= W:
                        continue
                    out[:, oy, ox] += k[kh - 1 - ky, kw - 1 - kx] * x[:, py // uy, px // ux]
    return out


@pytest.mark.parametrize('cfg', [(1, 1, 1, 1, 2, 1, 1, 2), (2, 1, 1, 1, -1, 2, 2, -1), (1, 2, 2, 1, 1, 0, 0, 1),
                                 (2, 2, 1, 1, 2, 1, 1, 2), (1, 1, 2, 2, 1, 1, 2, 1), (1, 1, 1, 1, 0, 1, 2, -1)])
def test_upfirdn2d_per_axis_against_loop(cfg):
    x = torch.randn(2, 7, 6, 3, dtype=f64)
    k = torch.rand(3, 4, dtype=f64)
    assert (S.upfirdn2d(x, k, *cfg) - _upfirdn_loop(x, k, *cfg)).abs().max().item() < 1e-12


def test_epilogues_and_elementwise():
    v = torch.randn(2, 5, 3, 8, dtype=f64)
    add, ref = torch.randn_like(v), torch.randn_like(v)
    out, out2 = S.fused_epilogue(v, add, ref, 0.2, 1.5)
    assert torch.equal(out, v + add)
    sel = torch.where(ref > 0, torch.tensor(1.5, dtype=f64), torch.tensor(0.2 * 1.5, dtype=f64))
    assert (out2 - (v + add) * sel).abs().max().item() < 1e-12
    demod, noise, post = torch.rand(2, 8, dtype=f64), torch.randn(2, 5, 3, dtype=f64), torch.rand(2, 8, dtype=f64)
    nw, bias = torch.tensor([0.3], dtype=f64), torch.randn(8, dtype=f64)
    y = S.modconv_epilogue(v, bias, demod, noise, nw, post)
    t = v * demod.view(2, 1, 1, 8) + 0.3 * noise.unsqueeze(-1)
    w = SO.fused_leaky_relu(t.permute(0, 3, 1, 2), bias).permute(0, 2, 3, 1) * post.view(2, 1, 1, 8)
    assert (y - w).abs().max().item() < 1e-12
    # fused_bias_act: grad 1 is the derivative of grad 0 at ref
    x = torch.randn(60, dtype=f64)
    b = torch.randn(4, dtype=f64)
    r = torch.randn(60, dtype=f64)
    rr = r.clone().requires_grad_()
    d = torch.autograd.grad(S.fused_bias_act(rr, None, None, 1, 1, 3, 0, 0.2, 1.0).sum(), rr)[0]
    g1 = S.fused_bias_act(x, b, r, 3, 4, 3, 1, 0.2, 1.0)
    bb = b[(torch.arange(60) // 3) % 4]
    assert (g1 - (x + bb) * d).abs().max().item() < 1e-12
    assert torch.equal(S.fused_bias_act(x, b, r, 3, 4, 1, 2, 0.2, 1.0), torch.zeros(60, dtype=f64))


def test_pixelnorm_sumsq_dot_against_oracle_forms():
    x = torch.randn(5, 9, dtype=f64)
    assert (S.pixelnorm(x, 5, 9) - x / torch.sqrt((x * x).mean(1, keepdim=True) + 1e-8)).abs().max() < 1e-12
    a, b = torch.randn(2, 7, 4, dtype=f64), torch.randn(2, 7, 4, dtype=f64)
    assert (S.nhwc_dot(a, b, 2, 7, 4, 1) - torch.einsum('nhc,nhc->nc', a, b)).abs().max() < 1e-12
    assert (S.nhwc_dot(a, b[..., 0], 2, 7, 4, 0) - torch.einsum('nhc,nh->nc', a, b[..., 0])).abs().max() < 1e-12
    assert abs(S.sumsq(a, 0.5).item() - 0.5 * a.pow(2).sum().item()) < 1e-12


@pytest.mark.parametrize('B', [1, 4, 8, 12])
def test_mbstd_against_oracle_and_closed_form(B):
    P, C, Cp = 6, 5, 8
    x = torch.randn(B, P, C, dtype=f64)
    y = S.mbstd(0, x, B, P, C, Cp)
    xo = x.view(B, 2, 3, C).permute(0, 3, 1, 2).float()                   # NCHW for the oracle
    want = SO.minibatch_stddev(xo).permute(0, 2, 3, 1).reshape(B, P, C + 1)
    assert maxerr(y[:, :, :C + 1], want) < 1e-6
    assert torch.equal(y[:, :, C + 1:], torch.zeros(B, P, Cp - C - 1, dtype=f64))
    # modes 1 / 2 (double-backward autograd) against the closed form in csrc/stylegan2_ops.hip
    gy, h = torch.randn(B, P, Cp, dtype=f64), torch.randn(B, P, C, dtype=f64)
    G = min(B, 4)
    M = B // G
    xg = x.view(G, M, P, C)
    mu = xg.mean(0, keepdim=True)
    sig = torch.sqrt(((xg - mu) ** 2).mean(0, keepdim=True) + 1e-8)
    gs = gy[:, :, C].reshape(G, M, P).sum((0, 2)).view(1, M, 1, 1)
    PC = P * C
    gx = gy[:, :, :C].reshape(G, M, P, C) + gs * (xg - mu) / (G * PC * sig)
    assert (S.mbstd(1, x, B, P, C, Cp, gy=gy) - gx.reshape(B, P, C)).abs().max().item() < 1e-12
    hg = h.view(G, M, P, C)
    hx = (hg * (xg - mu)).sum(0, keepdim=True)
    gx2 = gs / (G * PC) * ((hg - hg.mean(0, keepdim=True)) / sig - (xg - mu) * hx / (G * sig ** 3))
    t = (hx / sig).sum((2, 3), keepdim=True) / (G * PC)
    ggy = torch.zeros(G, M, P, Cp, dtype=f64)
    ggy[..., :C] = hg
    ggy[..., C] = t.view(1, M, 1).expand(G, M, P)
    r2, r2b = S.mbstd(2, x, B, P, C, Cp, gy=gy, h=h)
    assert (r2 - gx2.reshape(B, P, C)).abs().max().item() < 1e-12
    assert (r2b - ggy.reshape(B, P, Cp)).abs().max().item() < 1e-12


# ======================================================================================================================
# coverage of the GPU parity modules
# ======================================================================================================================
def _load(name):
    """A GPU parity module, loaded for its case tables only (importing it touches no GPU)."""
    spec = importlib.util.spec_from_file_location('_cases_' + name, os.path.join(_HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    if _HERE not in sys.path:
        sys.path.insert(0, _HERE)
    spec.loader.exec_module(mod)
    return mod


def upfirdn_form(major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """upfirdn2d_launch's dispatch (csrc/stylegan2_ops.hip), restated."""
    out_h, out_w = S.out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1)
    vec = minor % 4 == 0
    fir4 = vec and kh == 4 and kw == 4 and up_x == up_y and down_x == down_y
    buf_ok = major <= 65535 and in_h * in_w * minor * 4 < 2 ** 31 and out_h * out_w * minor * 4 < 2 ** 31
    if fir4 and up_x == 1 and down_x == 1:
        return 'u1d1_buf' if buf_ok else 'u1d1_ptr'
    if fir4 and ((up_x == 1 and down_x == 2) or (up_x == 2 and down_x == 1)):
        return ('u1d2' if down_x == 2 else 'u2d1') + ('_buf' if buf_ok else '_ptr')
    if minor == 1 and kh == 4 and kw == 4 and up_x == 2 and up_y == 2 and down_x == 1 and down_y == 1:
        return 'u2d1_planes'
    if vec and up_x == 1 and up_y == 1 and down_x == 1 and down_y == 1 and out_h >= 4:
        return 'strip4'
    return 'generic4' if vec else 'generic1'


UF_FORMS = {'u1d1_buf': 'upfirdn4_u1d1_buf_kernel', 'u1d1_ptr': 'upfirdn4_u1d1_kernel',
            'u1d2_buf': 'upfirdn4_u1d2_buf_kernel', 'u1d2_ptr': 'upfirdn4_u1d2_kernel',
            'u2d1_buf': 'upfirdn4_u2d1_buf_kernel', 'u2d1_ptr': 'upfirdn4_u2d1_kernel',
            'u2d1_planes': 'upfirdn4_u2d1_planes_kernel', 'strip4': 'upfirdn2d_strip_kernel<4>',
            'generic4': 'upfirdn2d_kernel<4>', 'generic1': 'upfirdn2d_kernel<1>'}


def simclr_forms(H, W):
    """contrad_simclr_augment / _bwd: the one-block LDS kernels while the image (forward: 3HW floats; backward:
    7HW + H^2 + W^2 floats) fits 64 KiB, the multi-pass kernels beyond; nparts = cdiv(HW, 4096)."""
    fwd = 'lds' if 3 * H * W * 4 <= 65536 else 'multipass'
    bwd = 'lds' if (7 * H * W + H * H + W * W) * 4 <= 65536 else 'multipass'
    return fwd, bwd, -(-H * W // 4096)


def test_simclr_path_thresholds():
    assert simclr_forms(73, 73)[0] == 'lds' and simclr_forms(74, 74)[0] == 'multipass'
    assert simclr_forms(42, 42)[1] == 'lds' and simclr_forms(43, 43)[1] == 'multipass'
    assert simclr_forms(40, 100)[:2] == ('lds', 'multipass')


def test_upfirdn_cases_cover_every_form():
    M = _load('test_sg2_ops_kernels_gpu')
    seen = set()
    for case in M.UF_CASES:
        got = upfirdn_form(*M._cfg(case))
        assert got == case[0], (case, got)
        seen.add(got)
    assert seen == set(UF_FORMS), set(UF_FORMS) - seen
    for case in M.MODCONV_CASES:
        N, in_h, in_w, K, px0, px1, py0, py1 = case[:8]
        form = case[-1].split(',')[0].split(':')[0]
        assert upfirdn_form(N, in_h, in_w, K, 4, 4, 1, 1, 1, 1, px0, px1, py0, py1) == form
    assert {c[-1].split(',')[0].split(':')[0] for c in M.MODCONV_CASES} == {'u1d1_buf', 'u1d1_ptr'}
    # the very large launches: non-temporal stores (output >= 256 MB) and the pointer forms (> 65535 images)
    nt = [c for c in M.UF_CASES if c[1] * np.prod(S.out_size(*M._cfg(c)[1:3], *M._cfg(c)[4:])) * c[4] * 4 >= 256 << 20]
    assert nt and all(upfirdn_form(*M._cfg(c)).endswith('_buf') for c in nt)
    # odd maps, negative pads, minor 1 / 3 / 4 / 32, non-square kernels
    assert {1, 3, 4, 32} <= {c[4] for c in M.UF_CASES}
    assert any(min(c[10:14]) < 0 for c in M.UF_CASES) and any(c[5][0] != c[5][1] for c in M.UF_CASES)
    # the standalone modconv epilogue: K = 4 and a large K, each optional operand present and absent, the grid cap
    E = M.EPI_CASES
    assert {4} <= {c[2] for c in E} and max(c[2] for c in E) >= 512
    for col in (3, 5, 6):
        assert {bool(c[col]) for c in E} == {True, False}, col
    assert {c[4] for c in E} == {0, 1, 2}
    assert any(c[0] * c[1] * c[2] // 4 > 16384 * 256 for c in E)
    # the reductions' caps
    caps = [M.nhwc_dot_segments(c[0], c[1]) < -(-c[1] // 64) for c in M.DOT_CASES]
    assert any(caps) and not all(caps)
    assert {4, 1024} <= {c[2] for c in M.DOT_CASES}
    assert {c[2] for c in M.DOT_CASES if M.nhwc_dot_segments(c[0], c[1]) < -(-c[1] // 64)} >= {4, 1024}
    assert {1, 4, 8, 12, 16} <= {c[0] for c in M.MBSTD_CASES}
    assert {(32, 48), (512, 528)} <= {c[2:] for c in M.MBSTD_CASES}


def test_augment_cases_cover_every_form():
    M = _load('test_augment_kernels_gpu')
    forms = set()
    for case in M.AUG_CASES:
        B, H, W, cf, hc = case[:5]
        fwd, bwd, nparts = simclr_forms(H, W)
        assert M.case_forms(case) == (fwd, bwd)
        forms |= {('fwd', fwd), ('bwd', bwd)}
    assert forms == {('fwd', 'lds'), ('fwd', 'multipass'), ('bwd', 'lds'), ('bwd', 'multipass')}
    sizes = {c[1:3] for c in M.AUG_CASES}
    assert {(32, 32), (42, 42), (43, 43), (73, 73), (74, 74), (96, 96), (512, 512)} <= sizes
    assert any(H != W and simclr_forms(H, W)[:2] == ('lds', 'multipass') for H, W in sizes)
    assert any(H > W for H, W in sizes) and any(H < W for H, W in sizes)
    assert any(simclr_forms(H, W)[1] == 'multipass' and (H * W) % 4096 for H, W in sizes)      # a ragged nparts
    assert {-1, 0, 1} <= {c[3] for c in M.AUG_CASES} and {0, 1} <= {c[4] for c in M.AUG_CASES}
    # the HSV-edge colours reach the HSV stage of a jittered sample unblended, in every op order the case runs:
    # Cmax = 0, r = g = b > 0 (atan2(0, 0)), and the pure hues 0, 1/3, 2/3
    for case in M.AUG_CASES:
        B, H, W, cf, hc = case[:5]
        P, x, _ = M.case_inputs(case)
        c = A.crop_flip(x, P)
        pre = torch.clamp(A.contrast_pre(c, P, hc), 0, 1)
        first = A.contrast_first(P, cf)
        for order in ({True, False} if cf < 0 else {bool(cf)}):
            sel = (P[:, 5] != 0) & (first == order)
            hin = (pre if order else c)[sel]
            r, g, b = hin[:, 0], hin[:, 1], hin[:, 2]
            classes = {'black': hin.amax(1) == 0, 'gray': (r == g) & (g == b) & (r > 0),
                       'red': (r > 0) & (g == 0) & (b == 0), 'green': (g > 0) & (r == 0) & (b == 0),
                       'blue': (b > 0) & (r == 0) & (g == 0)}
            missing = [k for k, m in classes.items() if not bool(m.any())]
            assert not missing, (case[:5], 'contrast first' if order else 'HSV first', missing)
    radii = {c[3] for c in M.BLUR_CASES}
    assert {0, 4, 25} <= radii and any(c[3] == min(c[1], c[2]) - 1 for c in M.BLUR_CASES)
    assert all(c[1] % 64 and c[2] % 64 for c in M.BLUR_CASES if c[1] != 512)
    assert {1, 15} <= {c[3] for c in M.CUTOUT_CASES}
