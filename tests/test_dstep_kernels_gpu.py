"""GPU parity of the non-conv kernels of the training steps against float64 (tests/dstep_ref64.py: plain float64 torch,
none of this project's kernels): csrc/ntxent.hip, specnorm.hip, conv_small.hip and elementwise.hip, over the launch
forms their dispatchers can pick (each case names the instantiation it is meant to reach).  Checked on the whole tensor:
  * max-norm error max|e| / max|ref| below the 1e-3 contract, and both it and the rel-L2 error ||e||_2 / ||ref||_2
    below a per-family bound (FAMILY_TOL, set at about 5x the worst observed on an MI355X), recorded through ``margin``;
  * outputs land in NaN-filled buffers with spare rows / columns / elements around them (in-place operands live inside
    larger NaN-filled storage), and every sentinel must still be NaN afterwards;
  * inputs are views of NaN-filled buffers too where the API takes a leading dimension, so a read past the operand
    shows up as a NaN in the result.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import dstep_ref64 as R
from contrad_amd import ops
from contrad_amd._lib import ADAM_CHUNK, lib
from contrad_amd.optim import FusedAdam
from oracle import contrad_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))           # (the fp32 value a kernel receives)

# per-family bounds against float64, about 5x the worst observed on an MI355X over this module
FAMILY_TOL = {                  # family: (max-norm, rel-L2)      observed worst (max-norm, rel-L2)
    'contrast_loss': (6e-7, 6e-7),              # 1.2e-7, 1.2e-7
    'contrast_lse': (8e-7, 7e-7),               # 1.6e-7, 1.3e-7
    'contrast_dz': (3.5e-5, 8e-6),              # 6.7e-6, 1.6e-6
    'l2norm_fwd': (6e-7, 2.5e-7),               # 1.1e-7, 5.1e-8
    'l2norm_bwd': (7e-7, 5e-7),                 # 1.3e-7, 9.4e-8
    'sn_weight': (9e-7, 1.1e-6),                # 1.8e-7, 2.1e-7
    'sn_uv': (1e-6, 8.5e-7),                    # 2.1e-7, 1.7e-7
    'sn_grad': (1.3e-6, 1.1e-6),                # 2.5e-7, 2.2e-7
    'rgb_fwd': (1.2e-6, 5e-7),                  # 2.4e-7, 9.9e-8
    'rgb_wgrad': (2.8e-6, 2.2e-6),              # 5.5e-7, 4.4e-7
    'rgb_dgrad': (6e-6, 3e-6),                  # 1.2e-6, 5.8e-7
    'colstats': (1e-6, 4e-7),                   # 2.0e-7, 7.6e-8
    'bn_fwd': (1.3e-6, 7e-7),                   # 2.6e-7, 1.4e-7
    'bn_bwd': (8.5e-7, 7e-7),                   # 1.7e-7, 1.4e-7
    'bn_running': (5e-7, 2.5e-7),               # 9.7e-8, 4.8e-8
    'bn_offset': (CONTRACT, CONTRACT),          # 5.3e-4, 2.8e-4 at 64 x std (see test_bn_offset_cost)
    'gan_loss': (1e-6, 8.5e-7),                 # 2.0e-7, 1.7e-7
    'gan_grad': (8e-7, 3e-7),                   # 1.5e-7, 5.7e-8
    'adam': (7e-7, 3.2e-7),                     # 1.4e-7, 6.3e-8
    'axpby': (5e-7, 1.8e-7),                    # 1.0e-7, 3.6e-8
}


def check(margin, family, what, out, ref):
    emax, el2 = R.errors(out, ref)
    assert emax < CONTRACT, (family, what, emax)
    tmax, tl2 = FAMILY_TOL[family]
    margin('dstep %s max-norm' % family, emax, tmax)
    margin('dstep %s rel-L2' % family, el2, tl2)


class Guard(object):
    """A NaN-filled (rows + 2 pr, ld) buffer whose operand is rows [pr, pr + rows) x columns [c0, c0 + cols)."""

    def __init__(self, rows, cols, ld=None, c0=0, pr=1):
        ld = cols + c0 if ld is None else ld
        assert c0 + cols <= ld
        self.buf = torch.full((rows + 2 * pr, ld), NAN, device=DEV)
        self.view = self.buf[pr:pr + rows, c0:c0 + cols]
        self.ld = ld
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        self.mask[pr:pr + rows, c0:c0 + cols] = False

    def intact(self):
        return bool(torch.isnan(self.buf[self.mask]).all())


def flat(shape, pad=4, fill=None):
    """A dense operand of ``shape`` with ``pad`` NaN floats either side: (Guard, view)."""
    n = math.prod(shape)
    g = Guard(1, n, ld=n + 2 * pad, c0=pad, pr=0)
    v = g.view.view(*shape)
    if fill is not None:
        v.copy_(fill)
    return g, v


def strided(x2d, ld, c0=0):
    """x2d copied into a NaN-filled buffer as rows of stride ld starting c0 floats in (c0 may exceed ld - K: the rows
    then straddle the buffer's own rows, as a misaligned view does)."""
    M, K = x2d.shape
    buf = torch.full(((M + 1) * ld + c0,), NAN, device=DEV)
    v = buf.as_strided((M, K), (ld, 1), c0)
    v.copy_(x2d)
    return v


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def call(name, *args):
    lib().call(name, *args)


P = ops._p


# ======================================================================================================================
# ntxent.hip
# ======================================================================================================================
def contrast_splits(R_):
    tiles = -(-R_ // 64)
    return max(1, min(256 // tiles, tiles))


# (N, D, mode, what)
CONTRAST_CASES = [
    (37, 1, 0, 'DP=64, D=1: scalar staging'),
    (37, 3, 1, 'DP=64, D=3: scalar staging, R=111'),
    (50, 64, 0, 'DP=64, R=100'),
    (33, 65, 1, 'DP=128, D=65: scalar staging, R=99'),
    (100, 96, 0, 'DP=128'),
    (64, 128, 1, 'DP=128, R=192'),
    (45, 129, 0, 'DP=256, D=129: scalar staging, R=90'),
    (70, 200, 1, 'DP=256, R=210'),
    (128, 256, 0, 'DP=256'),
    (2, 128, 1, 'SupCon N=2: one positive per anchor'),
    (1, 16, 0, 'NT-Xent N=1'),
    (512, 128, 1, 'the c10_b512 SupCon shape'),
    (4128, 128, 0, 'R=8256 > 8192: S=1, dZ written by contrast_bwd_kernel'),
    (2752, 64, 1, 'R=8256 SupCon: S=1'),
]


def contrast_z(N, D, mode):
    """The normalised rows of a contrastive problem: 2N (NT-Xent) or 3N (SupCon) of them.  (Shared with
    tests/test_workspace_contract_gpu.py.)"""
    return F.normalize(torch.randn((2 if mode == 0 else 3) * N, D, device=DEV, generator=gen(N * 7 + D + mode)))


@pytest.mark.parametrize('case', CONTRAST_CASES, ids=lambda c: 'N%d-D%d-m%d' % c[:3])
def test_contrast(margin, case):
    N, D, mode, _ = case
    R_ = (2 if mode == 0 else 3) * N
    S = contrast_splits(R_)
    if N >= 4128:
        assert S == 1
    temp = 0.1
    inv_temp = f32(1.0 / temp)
    z = contrast_z(N, D, mode)
    loss_ref, lse_ref, dz_ref = R.contrast(z, N, mode, 1.0 / inv_temp)
    nbytes = lib().raw('contrad_contrast_workspace_bytes')(R_, D)
    ws = torch.empty((nbytes + 3) // 4, device=DEV)
    g_lse, lse = flat((R_,))
    g_rl, rowloss = flat((R_,))
    g_loss, loss = flat((1,))
    call('contrad_contrast_fwd', P(z), R_, D, N, mode, inv_temp, P(lse), P(rowloss), P(loss), P(ws), nbytes,
         ops._stream())
    gdz = Guard(R_, D)
    call('contrad_contrast_bwd', P(z), P(lse), R_, D, N, mode, inv_temp, P(None), P(gdz.view), P(ws), nbytes,
         ops._stream())
    gs_val = 0.375
    gs = torch.full((1,), gs_val, device=DEV)
    gdz2 = Guard(R_, D)
    call('contrad_contrast_bwd', P(z), P(lse), R_, D, N, mode, inv_temp, P(gs), P(gdz2.view), P(ws), nbytes,
         ops._stream())
    torch.cuda.synchronize()
    assert g_lse.intact() and g_rl.intact() and g_loss.intact() and gdz.intact() and gdz2.intact()
    what = 'N=%d D=%d mode=%d S=%d' % (N, D, mode, S)
    check(margin, 'contrast_loss', what, loss, loss_ref.reshape(1))
    check(margin, 'contrast_lse', what, lse, lse_ref)
    check(margin, 'contrast_dz', what, gdz.view, dz_ref)
    check(margin, 'contrast_dz', what + ' grad_scale', gdz2.view, dz_ref * gs_val)
    if mode == 1:                                                      # (only the fakes are anchors)
        assert torch.equal(rowloss[:2 * N], torch.zeros(2 * N, device=DEV))


def test_contrast_supcon_single_sample_rejected():
    """SupCon with N = 1 has no positive for its one anchor: the reference divides 0 by 0 (NaN loss).  The launcher
    rejects it instead of returning a finite number that matches nothing."""
    z = F.normalize(torch.randn(3, 8, device=DEV))
    with pytest.raises(RuntimeError, match='status -22'):
        ops.contrast_fwd(z, 1, 1, 0.1)
    lse = torch.zeros(3, device=DEV)
    with pytest.raises(RuntimeError, match='status -22'):
        ops.contrast_bwd(z, lse, 1, 1, 0.1)


# (R, D, ldu, c0, what)
L2_CASES = [
    (1536, 128, 640, 256, 'projection column slice of a wider head output'),
    (75, 3, 8, 5, 'D=3, odd offset'),
    (9, 300, 300, 0, 'D > 256, dense'),
]


@pytest.mark.parametrize('case', L2_CASES, ids=lambda c: 'R%d-D%d-ld%d' % c[:3])
def test_l2norm(margin, case):
    R_, D, ldu, c0, _ = case
    u = strided(torch.randn(R_, D, device=DEV, generator=gen(R_)) * 3, ldu, c0)
    z_ref, inv_ref = R.l2norm(u)
    gz, z = flat((R_, D))
    ginv, inv = flat((R_,))
    call('contrad_l2norm_fwd', P(u), ldu, P(z), P(inv), R_, D, 1e-12, ops._stream())
    dz = torch.randn(R_, D, device=DEV, generator=gen(R_ + 1))
    du_ref = R.l2norm_bwd(dz, u)
    gdu = Guard(R_, D, ld=D + 12, c0=4)
    ops.l2norm_bwd(dz, z, inv, out=gdu.view)
    base = torch.randn(R_, D, device=DEV, generator=gen(R_ + 2))
    gacc = Guard(R_, D, ld=D + 12, c0=8)
    gacc.view.copy_(base)
    ops.l2norm_bwd(dz, z, inv, out=gacc.view, accumulate=True)
    torch.cuda.synchronize()
    assert gz.intact() and ginv.intact() and gdu.intact() and gacc.intact()
    what = 'R=%d D=%d ldu=%d' % (R_, D, ldu)
    check(margin, 'l2norm_fwd', what, z, z_ref)
    check(margin, 'l2norm_fwd', what + ' inv', inv, inv_ref)
    check(margin, 'l2norm_bwd', what, gdu.view, du_ref)
    check(margin, 'l2norm_bwd', what + ' accumulate', gacc.view, du_ref + base.double())


# ======================================================================================================================
# specnorm.hip
# ======================================================================================================================
class Layer(object):
    """One layer of a weight-prep batch: W (K, C*T) inside NaN-padded storage, u / v likewise (SN layers), the packed
    destination with ldw >= K and NaN-filled spare columns / rows."""

    def __init__(self, K, C, T, fixed, ldw, seed, mis=False):
        g = gen(seed)
        self.K, self.C, self.T, self.fixed, self.ldw = K, C, T, fixed, ldw
        self.gw_store, self.w = flat((K, C * T), pad=1 if mis else 4,
                                     fill=torch.randn(K, C * T, device=DEV, generator=g) * 0.05)
        if fixed > 0:
            self.gu = self.gv = self.u = self.v = None
            self.spec = ops.SnSpec(self.w, fixed_scale=fixed, view_kct=(K, C, T))
        else:
            # u, v as earlier power iterations leave them (u = W v / |W v|): sigma = u^T W v is then |W v|, not a
            # cancelling sum of random-signed terms whose fp32 rounding would be amplified into W / sigma
            v = F.normalize(torch.randn(C * T, device=DEV, generator=g), dim=0)
            self.gu, self.u = flat((K,), fill=F.normalize(self.w.double() @ v.double(), dim=0).float())
            self.gv, self.v = flat((C * T,), fill=v)
            self.spec = ops.SnSpec(self.w, self.u, self.v, view_kct=(K, C, T))
        self.gwp = Guard(T * C, K, ld=ldw)
        self.gus, self.us = flat((K,))
        self.gvs, self.vs = flat((C * T,))


def sn_batch_run(margin, layers, training, what, split=None):
    """Weight prep then weight gradient over ``layers`` (as one list, or split at ``split`` the way
    models/gan/sndcgan.py:105-106 prepares the trunk in eval mode and the heads in the caller's mode)."""
    n = len(layers)
    specs = [L.spec for L in layers]
    wps, ldws = [L.gwp.view for L in layers], [L.ldw for L in layers]
    us, vs = [L.us for L in layers], [L.vs for L in layers]
    modes = [training] * n if split is None else [False] * split + [training] * (n - split)
    refs = []
    for L, tr in zip(layers, modes):
        refs.append(R.sn_prep(L.w, L.u, L.v, tr, fixed_scale=L.fixed))
    offs, nscr = ops.sn_scratch_floats(specs)
    scratch = torch.empty(nscr, device=DEV)
    gsig, sigma = flat((n,))
    if split is None:
        ops.sn_weight_prep(specs, wps, ldws, training, scratch, offs, sigma, us, vs)
    else:
        ops.sn_weight_prep(specs[:split], wps[:split], ldws[:split], False, scratch, offs[:split], sigma, us[:split],
                           vs[:split])
        ops.sn_weight_prep(specs[split:], wps[split:], ldws[split:], training, scratch, offs[split:], sigma[split:],
                           us[split:], vs[split:])
    torch.cuda.synchronize()
    assert gsig.intact()
    for i, (L, (weff, u2, v2, sig)) in enumerate(zip(layers, refs)):
        w_l = '%s layer %d (K=%d C=%d T=%d ldw=%d%s)' % (what, i, L.K, L.C, L.T, L.ldw,
                                                        ' fixed' if L.fixed > 0 else '')
        assert L.gwp.intact() and L.gw_store.intact(), w_l
        check(margin, 'sn_weight', w_l, R.unpack(L.gwp.view, L.K, L.C, L.T), weff)
        check(margin, 'sn_weight', w_l + ' sigma', sigma[i:i + 1], sig.reshape(1))
        if L.fixed > 0:
            assert L.gus.intact() and L.gvs.intact(), w_l          # no snapshot of a fixed-scale layer
            continue
        assert L.gu.intact() and L.gv.intact() and L.gus.intact() and L.gvs.intact(), w_l
        check(margin, 'sn_uv', w_l + ' u', L.u, u2)
        check(margin, 'sn_uv', w_l + ' v', L.v, v2)
        assert torch.equal(L.us, L.u) and torch.equal(L.vs, L.v), w_l
    # backward: G (packed, NaN in the spare columns) -> dL/dW_orig (K, C*T) in NaN-padded storage
    gwps, gws, gguards = [], [], []
    for i, L in enumerate(layers):
        G = Guard(L.T * L.C, L.K, ld=L.ldw)
        G.view.copy_(torch.randn(L.T * L.C, L.K, device=DEV, generator=gen(100 + i)))
        gg, gw = flat((L.K, L.C * L.T))
        gwps.append(G.view)
        gws.append(gw)
        gguards.append(gg)
    ops.sn_weight_grad(specs, wps, ldws, gwps, gws, scratch, offs, sigma, us, vs)
    torch.cuda.synchronize()
    for i, (L, (weff, u2, v2, sig)) in enumerate(zip(layers, refs)):
        w_l = '%s layer %d grad' % (what, i)
        assert gguards[i].intact(), w_l
        ref = R.sn_grad(R.unpack(gwps[i], L.K, L.C, L.T), L.w, u2, v2, fixed_scale=L.fixed)
        check(margin, 'sn_grad', w_l, gws[i], ref)


def _mixed_layers(seed):
    # (K, C, T, fixed_scale, ldw, misaligned w)
    shapes = [(64, 3, 9, 0, 64, False),            # the first conv of D
              (128, 64, 16, 0.25, 132, False),     # fixed scale, ldw > K
              (30, 7, 9, 0, 33, False),            # K % 4 != 0, IN = 63, odd ldw: scalar paths
              (33, 5, 1, 0, 36, False),            # T = 1, IN = 5
              (16, 20, 16, 0.5, 16, False),        # fixed, T = 16
              (100, 300, 1, 0, 104, True),         # IN = 300 (not a multiple of 256), misaligned W: scalar paths
              (512, 36, 16, 0, 520, False),        # IN = 576, K = 512 over 128 phase-2 blocks
              (7, 1000, 1, 0, 7, False)]           # K < 32, IN over four phase-1 slots
    return [Layer(K, C, T, fs, ldw, seed + i, mis) for i, (K, C, T, fs, ldw, mis) in enumerate(shapes)]


@pytest.mark.parametrize('training', [True, False])
def test_sn_mixed_batch(margin, training):
    sn_batch_run(margin, _mixed_layers(10), training, 'mixed training=%d' % training)


@pytest.mark.parametrize('training', [True, False])
def test_sn_more_than_max_layers(margin, training):
    """30 layers: ops._sn_batches splits the call at CONTRAD_SN_MAX_LAYERS and offsets sigma."""
    assert ops.SN_MAX_LAYERS == 24
    layers = []
    for i in range(30):
        K, C, T = [(16, 8, 9), (40, 3, 1), (29, 12, 16), (64, 64, 9), (5, 300, 1)][i % 5]
        fs = 0.125 if i % 7 == 3 else 0.0
        layers.append(Layer(K, C, T, fs, K + 4 * (i % 3), 200 + i))
    sn_batch_run(margin, layers, training, '30 layers training=%d' % training)


@pytest.mark.parametrize('training', [True, False])
def test_sn_sndcgan_split(margin, training):
    """The D_SNDCGAN batch (7 convs, then the linear / projection heads, the 8192-wide ones viewed as (K, 512, 16))
    prepared as models/gan/sndcgan.py:105-106 does when the trunk is frozen: trunk in eval mode, heads in ``training``."""
    shapes = [(co, ci, k * k) for (ci, co, k, _, _) in O.SNDCGAN_D_CONVS]
    shapes += [(512, 512, 16), (1, 512, 1), (512, 512, 16), (128, 512, 1), (512, 512, 16), (128, 512, 1)]
    layers = [Layer(K, C, T, 0.0, ops.round_up(K, 4), 300 + i) for i, (K, C, T) in enumerate(shapes)]
    sn_batch_run(margin, layers, training, 'sndcgan split training=%d' % training, split=7)


# ======================================================================================================================
# conv_small.hip
# ======================================================================================================================
SLOPE = f32(0.2)
GAIN = f32(math.sqrt(2.0))


def packed_weight(w, extra):
    """pack_weight with ldw = round_up(K, 4) + extra and NaN in the spare columns."""
    K, C, k, _ = w.shape
    ldw = ops.round_up(K, 4) + extra
    wp = torch.full((k * k * C, ldw), NAN, device=DEV)
    wp[:, :K] = w.permute(2, 3, 1, 0).reshape(k * k * C, K)
    return wp


# (N, H, W, K, k, bias, ldy_extra, what)
RGB_FWD_CASES = [
    (5, 32, 32, 64, 3, True, 0, '<3,3>: the SNDCGAN first conv'),
    (3, 40, 32, 128, 1, True, 8, '<1,3>: H=40 not a multiple of pick_th(32)=32, ldy > K'),
    (4, 7, 9, 16, 3, False, 4, '<3,3>: no bias, H < TH, odd W'),
    (2, 12, 20, 4, 3, True, 4, '<3,3>: K=4, one lane per pixel'),
    (2, 9, 64, 1024, 1, False, 0, '<1,3>: K=1024, 256 lanes per pixel, TH=16'),
    (800, 8, 8, 32, 3, True, 0, 'wgrad <3,3>: 800 tiles > 768-block cap, blocks loop'),
    (2100, 8, 8, 16, 1, False, 4, 'wgrad <1,3>: 2100 tiles > 2048-block cap, blocks loop'),
]


def rgb_inputs(case):
    """(img, w, bias guard, bias, gy) of an RGB_FWD_CASES entry: gy NHWC with ldy > K where the case says so and NaN in the
    spare channels.  (Shared with tests/test_workspace_contract_gpu.py.)"""
    N, H, W, K, k, has_bias, ye, _ = case
    g = gen(N + K + k)
    img = torch.rand(N, 3, H, W, device=DEV, generator=g)
    w = torch.randn(K, 3, k, k, device=DEV, generator=g) * 0.2
    gb, bias = flat((K,), fill=torch.randn(K, device=DEV, generator=g) * 0.1) if has_bias else (None, None)
    gyv = torch.full((N, H, W, K + ye), NAN, device=DEV)
    gyv[..., :K] = torch.randn(N, H, W, K, device=DEV, generator=g)
    return img, w, gb, bias, gyv[..., :K]


@pytest.mark.parametrize('case', RGB_FWD_CASES, ids=lambda c: 'N%d-%dx%d-K%d-k%d' % c[:5])
def test_rgb_conv_fwd_wgrad(margin, case):
    N, H, W, K, k, has_bias, ye, _ = case
    img, w, gb, bias, gyv = rgb_inputs(case)
    wp = packed_weight(w, 4)
    ldy = K + ye
    gy_out = Guard(N * H * W, K, ld=ldy, pr=H * W)                   # (a spare image either side)
    y = gy_out.buf[H * W:H * W * (N + 1)].view(N, H, W, ldy)[..., :K]
    ops.rgb_conv_fwd(img, wp, bias, K, k, 2.0, -1.0, SLOPE, GAIN, out=y)
    ref = R.rgb_fwd(img, w, bias, 2.0, -1.0, SLOPE, GAIN)
    # wgrad: gy NHWC with ldy > K and NaN in the spare channels; dwp rows x ldw with NaN spare rows / columns
    ldw = K + 8
    gdw = Guard(k * k * 3, K, ld=ldw)
    gdb, db = flat((K,))
    ops.rgb_conv_wgrad(img, gyv, k, 2.0, -1.0, gdw.view, db)
    dw_ref, db_ref = R.rgb_wgrad(img, gyv, k, 2.0, -1.0)
    torch.cuda.synchronize()
    assert gy_out.intact() and gdw.intact() and gdb.intact()
    what = 'N=%d %dx%d K=%d k=%d' % (N, H, W, K, k)
    check(margin, 'rgb_fwd', what, y, ref)
    check(margin, 'rgb_wgrad', what + ' dw', ops.unpack_weight(gdw.view, K, 3, k, k), dw_ref)
    check(margin, 'rgb_wgrad', what + ' dbias', db, db_ref)


# (N, H, W, K, C, k, mod, residual, act, bias, ldy_extra, kernel)
RGB_DGRAD_CASES = [
    (6, 32, 32, 64, 3, 3, False, False, 1, True, 0, 'tile: generator last layer + tanh'),
    (3, 17, 24, 32, 1, 3, False, False, 0, False, 8, 'tile: C=1, TH=10 ragged, ldy > K'),
    (2, 9, 64, 128, 2, 3, False, False, 0, True, 0, 'tile: W=64, TH=4'),
    (2, 5, 128, 32, 3, 3, False, False, 1, True, 4, '<3,1>: W=128 tile over 64 KB, falls back'),
    (1, 3, 256, 64, 2, 3, False, False, 0, False, 0, '<3,1>: W=256 falls back'),
    (4, 8, 8, 128, 3, 3, True, False, 0, True, 0, '<3,1>: mod'),
    (3, 16, 16, 64, 3, 3, False, True, 1, True, 4, '<3,1>: residual + tanh'),
    (2, 9, 11, 16, 4, 3, False, False, 0, True, 0, '<3,1>: C=4, K=16'),
    (2, 6, 6, 16, 3, 3, False, False, 0, False, 0, '<3,1>: K=16 not a multiple of 32'),
    (4, 16, 16, 256, 3, 1, True, True, 0, True, 0, '<1,1>: ToRGB, mod + residual'),
    (3, 8, 8, 512, 3, 1, True, False, 0, False, 8, '<1,2>: K=512'),
    (2, 7, 5, 32, 1, 1, False, False, 1, True, 0, '<1,1>: C=1, tanh'),
]


@pytest.mark.parametrize('case', RGB_DGRAD_CASES, ids=lambda c: 'N%d-%dx%d-K%d-C%d-k%d' % c[:6])
def test_rgb_conv_dgrad(margin, case):
    N, H, W, K, C, k, has_mod, has_res, act, has_bias, ye, _ = case
    g = gen(N * H + K + C + k)
    ldy = K + ye
    gy = torch.full((N, H, W, ldy), NAN, device=DEV)
    gy[..., :K] = torch.randn(N, H, W, K, device=DEV, generator=g) * 0.1
    gy = gy[..., :K]
    w = torch.randn(K, C, k, k, device=DEV, generator=g) * 0.1
    wp = packed_weight(w, 4)
    gb, bias = flat((C,), fill=torch.randn(C, device=DEV, generator=g) * 0.1) if has_bias else (None, None)
    mod = torch.rand(N, K, device=DEV, generator=g) + 0.5 if has_mod else None
    res = torch.randn(N, C, H, W, device=DEV, generator=g) * 0.5 if has_res else None
    scale, shift = (0.5, 0.5) if act else (2.0, 0.0)
    gout = Guard(N * C * H, W, pr=C * H)
    out = gout.view.reshape(N, C, H, W)
    ops.rgb_conv_dgrad(gy, wp, bias, C, k, act=act, out_scale=scale, out_shift=shift, out=out, mod=mod, residual=res)
    ref = R.rgb_dgrad(gy, w, bias, act, scale, shift, mod, res)
    torch.cuda.synchronize()
    assert gout.intact() and (gb is None or gb.intact())
    check(margin, 'rgb_dgrad', 'N=%d %dx%d K=%d C=%d k=%d' % (N, H, W, K, C, k), out, ref)


# ======================================================================================================================
# elementwise.hip: colstats
# ======================================================================================================================
# (M, K, ld, misalign, accumulate, what)
COLSTATS_CASES = [
    (1003, 67, 67, 0, False, 'scalar: K % 4 != 0'),
    (500, 64, 68, 1, False, 'scalar: x 4-byte misaligned'),
    (1, 67, 67, 0, False, 'scalar: M=1'),
    (777, 64, 64, 0, False, 'vec CQB=16'),
    (2000, 128, 160, 0, True, 'vec CQB=32, ld > K, accumulate'),
    (1000, 256, 256, 0, False, 'vec CQB=64'),
    (4096, 512, 512, 0, True, 'vec CQB=128, accumulate'),
    (300, 1024, 1024, 0, False, 'vec CQB=256'),
    (300, 1028, 1032, 0, False, 'vec CQB=256, two column blocks, the second ragged'),
    (64, 8192, 8192, 0, False, 'vec CQB=256, 8 column blocks'),
    (1, 64, 64, 0, False, 'vec: M=1'),
    (100003, 64, 64, 0, False, 'vec: 512 row blocks of 196 rows'),
]


def colstats_inputs(case, with_sq):
    """(x, base) of a COLSTATS_CASES entry: the strided, possibly misaligned operand and what an accumulating case adds to
    (None otherwise).  (Shared with tests/test_workspace_contract_gpu.py.)"""
    M, K, ld, mis, acc, _ = case
    x = strided(torch.randn(M, K, device=DEV, generator=gen(M + K)) + 0.25, ld, mis)
    assert (x.data_ptr() % 16 != 0) == bool(mis)
    base = torch.randn(2 if with_sq else 1, K, device=DEV, generator=gen(1)) * 10 if acc else None
    return x, base


@pytest.mark.parametrize('case', COLSTATS_CASES, ids=lambda c: 'M%d-K%d-ld%d-m%d-a%d' % c[:5])
@pytest.mark.parametrize('with_sq', [True, False])
def test_colstats(margin, case, with_sq):
    M, K, ld, mis, acc, _ = case
    x, base = colstats_inputs(case, with_sq)
    nstat = 2 if with_sq else 1
    gout, out = flat((nstat, K), fill=base)
    ops.colstats(x, with_sq=with_sq, out=out, accumulate=acc)
    ref = R.colstats(x)[:nstat]
    if acc:
        ref = ref + base.double()
    torch.cuda.synchronize()
    assert gout.intact()
    what = 'M=%d K=%d ld=%d sq=%d' % (M, K, ld, with_sq)
    check(margin, 'colstats', what + ' sum', out[0], ref[0])
    if with_sq:
        check(margin, 'colstats', what + ' sumsq', out[1], ref[1])


# ======================================================================================================================
# elementwise.hip: BatchNorm + ReLU
# ======================================================================================================================
# (M, K, ld, perm_hw, offset (in units of each channel's std), what)
BN_CASES = [
    (2048, 64, 64, 1, 0.0, 'G_SNDCGAN 16x16 BN, N=8'),
    (1000, 96, 104, 1, 1.0, 'ld > K'),
    (64, 8192, 8192, 16, 0.0, "G_SNDCGAN norm_init: linear -> BN1d, perm_hw=16"),
    (37, 128, 128, 1, 0.0, 'odd batch'),
    (4096, 128, 128, 1, 16.0, 'common offset 16 x std'),
    (4096, 128, 128, 1, 64.0, 'common offset 64 x std'),
]


def bn_inputs(M, K, offset, seed):
    g = gen(seed)
    std = torch.rand(K, device=DEV, generator=g) * 2 + 0.1
    x = torch.randn(M, K, device=DEV, generator=g) * std + offset * std * torch.where(
        torch.rand(K, device=DEV, generator=g) < 0.5, -1.0, 1.0)
    gamma = torch.rand(K, device=DEV, generator=g) + 0.5
    beta = torch.randn(K, device=DEV, generator=g) * 0.3
    return x, gamma, beta


@pytest.mark.parametrize('case', BN_CASES, ids=lambda c: 'M%d-K%d-ld%d-p%d-off%g' % c[:5])
def test_bn_relu(margin, case):
    M, K, ld, perm, offset, _ = case
    x0, gamma, beta = bn_inputs(M, K, offset, M + K)
    x = strided(x0, ld)
    eps = 1e-5
    what = 'M=%d K=%d ld=%d perm=%d offset=%g' % (M, K, ld, perm, offset)
    stats = ops.colstats(x, with_sq=True)
    # running statistics, with the producing conv's bias folded into the mean, and num_batches_tracked
    g = gen(7)
    rm0, rv0 = torch.randn(K, device=DEV, generator=g), torch.rand(K, device=DEV, generator=g) + 0.5
    cb = torch.randn(K, device=DEV, generator=g) * 0.1
    grm, rm = flat((K,), fill=rm0)
    grv, rv = flat((K,), fill=rv0)
    nbt_buf = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    nbt_buf[1] = 41
    ops.bn_running_update(stats, float(M), cb, 0.1, rm, rv, nbt_buf[1:2])
    rm_ref, rv_ref = R.bn_running(rm0, rv0, x, cb, 0.1)
    # forward
    gy = Guard(M, K, ld=ld + 4, c0=4)
    ops.bn_relu_apply(x, gy.view, stats, float(M), gamma, beta, eps, perm)
    y_ref = R.bn_relu(x, gamma, beta, eps, perm)
    # backward (the C API takes a leading dimension shared by dy, x and dx)
    dy = strided(torch.randn(M, K, device=DEV, generator=g), ld)
    nbytes = lib().raw('contrad_colstats_workspace_bytes')(ctypes.c_longlong(M), K, 1)
    ws = torch.empty((nbytes + 3) // 4, device=DEV)
    g2k, out2k = flat((2, K))
    call('contrad_bn_relu_bwd_stats', P(dy), P(x), ctypes.c_longlong(M), K, ld, P(stats), float(M), P(gamma), P(beta),
         eps, P(out2k), P(ws), ctypes.c_longlong(nbytes), ops._stream())
    gdx = Guard(M, K, ld=ld)
    call('contrad_bn_relu_bwd_apply', P(dy), P(x), P(gdx.view), ctypes.c_longlong(M), K, ld, P(stats), float(M),
         P(gamma), P(beta), eps, P(out2k), ops._stream())
    y = gy.view if perm == 1 else gy.view.reshape(M, perm, K // perm).transpose(1, 2).reshape(M, K)
    dx_ref, dg_ref, db_ref = R.bn_relu_bwd(dy, x, gamma, beta, eps, mask=y > 0)     # (on the kernel's active set)
    torch.cuda.synchronize()
    assert grm.intact() and grv.intact() and gy.intact() and g2k.intact() and gdx.intact()
    assert nbt_buf.tolist() == [-7, 42, -7]
    # a large common offset costs what var = E[x^2] - mean^2 in fp32 loses: those cases are held to the contract alone
    fam = (lambda f: f) if offset <= 1 else (lambda f: 'bn_offset')
    check(margin, fam('bn_running'), what + ' mean', rm, rm_ref)
    check(margin, fam('bn_running'), what + ' var', rv, rv_ref)
    check(margin, fam('bn_fwd'), what, gy.view, y_ref)
    check(margin, fam('bn_bwd'), what + ' dx', gdx.view, dx_ref)
    check(margin, fam('bn_bwd'), what + ' dgamma', out2k[1], dg_ref)
    check(margin, fam('bn_bwd'), what + ' dbeta', out2k[0], db_ref)


def test_bn_offset_cost(margin):
    """What the fp32 var = E[x^2] - mean^2 of the statistics costs as the common offset grows (recorded, not asserted
    beyond the offsets of BN_CASES: the table shows the max-norm error of the BN output at each offset)."""
    M, K = 4096, 128
    for offset in (0.0, 4.0, 16.0, 64.0, 256.0):
        x, gamma, beta = bn_inputs(M, K, offset, 5)
        stats = ops.colstats(x, with_sq=True)
        y = torch.empty_like(x)
        ops.bn_relu_apply(x, y, stats, float(M), gamma, beta, 1e-5)
        emax, _ = R.errors(y, R.bn_relu(x, gamma, beta, 1e-5))
        margin('dstep bn_fwd offset %5.0f x std (max-norm, observed only)' % offset, emax, float('inf'))


# ---- eval mode: running statistics as they are (contrad_bn_relu_apply_eval) ----
# (M, K, ld, perm_hw, what)
BN_EVAL_SHAPES = [
    (5, 8192, 8192, 16, 'norm_init at 32x32'),
    (3, 2048, 2048, 4, 'norm_init at 16x16'),
    (768, 128, 128, 1, 'the 16x16 BN of three images; also in place, as CDDLSSampler._g_forward calls it'),
    (33, 64, 66, 1, 'ld != K'),
    (7, 6, 7, 1, 'odd stride'),
    (2000, 64, 64, 1, 'more than one block'),
]
# The bound of each case is R.bn_eval_bound: max(FAMILY_TOL['bn_fwd'], 2 x the error of plain fp32 torch on the same device
# tensors); regime A is held to FAMILY_TOL['bn_fwd'] alone.  Observed worst on an MI355X over BN_EVAL_SHAPES, with and
# without conv bias (profiles/bn_eval.txt):
BN_EVAL_OBSERVED = {            # regime: kernel (max-norm, rel-L2)      fp32 torch (max-norm, rel-L2); the parent commit's form
    'A': (1.1e-7, 5.9e-8),      # 1.4e-7, 5.9e-8; 1.1e-7, 5.9e-8
    'B': (4.4e-7, 4.3e-7),      # 4.6e-7, 4.4e-7; 7.3e-6, 2.3e-6
    'C': (2.9e-6, 2.8e-6),      # 2.6e-6, 2.8e-6; 9.0e-4, 2.7e-4
    'D': (2.7e-5, 3.4e-5),      # 2.7e-5, 3.4e-5; 9.1e-2, 2.0e-2
    'E': (3.1e-5, 4.1e-5),      # 2.9e-5, 4.1e-5; 6.7e-4, 2.4e-4
    'F': (1.0e-5, 1.8e-5),      # 1.0e-5, 1.8e-5; 5.8e-4, 2.3e-4
    'G': (1.3e-7, 4.9e-8),      # 2.0e-6, 2.1e-6; 1.6e-7, 6.4e-8
}


@pytest.mark.parametrize('regime', list(R.BN_EVAL_REGIMES))
@pytest.mark.parametrize('shape', BN_EVAL_SHAPES, ids=lambda c: 'M%d-K%d-ld%d-p%d' % c[:4])
def test_bn_relu_eval(margin, shape, regime):
    """Eval-mode BatchNorm + ReLU at the statistics of a trained generator (regimes of tests/dstep_ref64.py: mean^2 / var from
    0.1 to 3e8, var = 0, running_mean and conv bias that cancel) against float64."""
    import types
    M, K, ld, perm, _ = shape
    eps = 1e-5
    for with_bias in (True, False):
        if not with_bias and regime in R.BN_EVAL_NEEDS_BIAS:
            continue
        inp = R.bn_eval_inputs(regime, M, K, M + K + ord(regime), with_bias, DEV)
        inp['x'] = x = strided(inp['x'], ld)
        y_ref = R.bn_relu_eval(x, inp['cb'], inp['rm'], inp['rv'], inp['gamma'], inp['beta'], eps, perm)
        e_torch = R.errors(R.bn_relu_eval_fp32(inp, eps, perm), y_ref)
        gm, mean = flat((K,), fill=ops.bn_eval_mean(types.SimpleNamespace(running_mean=inp['rm']), inp['cb']))
        gv, var = flat((K,), fill=inp['rv'])
        gg, gamma = flat((K,), fill=inp['gamma'])
        gb, beta = flat((K,), fill=inp['beta'])
        gy = Guard(M, K, ld=ld + 4, c0=4)
        ops.bn_relu_apply_eval(x, gy.view, mean, var, gamma, beta, eps, perm)
        outs = [('', gy)]
        if perm == 1 and M == 768:
            gx = Guard(M, K, ld=ld + 4, c0=4)
            gx.view.copy_(x)
            ops.bn_relu_apply_eval(gx.view, gx.view, mean, var, gamma, beta, eps, 1)
            outs.append((' in place', gx))
        torch.cuda.synchronize()
        assert gm.intact() and gv.intact() and gg.intact() and gb.intact()
        tmax, tl2 = R.bn_eval_bound(FAMILY_TOL['bn_fwd'], e_torch, regime)
        margin('dstep bn_eval regime %s fp32 torch max-norm (observed only)' % regime, e_torch[0], float('inf'))
        margin('dstep bn_eval regime %s fp32 torch rel-L2 (observed only)' % regime, e_torch[1], float('inf'))
        for tag, g in outs:
            what = 'regime %s M=%d K=%d ld=%d perm=%d bias=%d%s' % (regime, M, K, ld, perm, with_bias, tag)
            assert g.intact(), what
            emax, el2 = R.errors(g.view, y_ref)
            print('bn_eval %s: kernel %.2e / %.2e, fp32 torch %.2e / %.2e' % ((what, emax, el2) + e_torch))
            assert emax < CONTRACT, (what, emax)
            margin('dstep bn_eval regime %s max-norm' % regime, emax, tmax)
            margin('dstep bn_eval regime %s rel-L2' % regime, el2, tl2)
        if len(outs) == 2:
            assert torch.equal(outs[0][1].view, outs[1][1].view)


def test_bn_relu_apply_eval_rejects_bad_arguments():
    x = torch.zeros(4, 8, device=DEV)
    k = torch.ones(8, device=DEV)
    good = [P(x), P(x), ctypes.c_longlong(4), 8, 8, 8, P(k), P(k), P(k), P(k), 1e-5, 1, ops._stream()]
    call('contrad_bn_relu_apply_eval', *good)
    for i, bad in ((0, None), (1, None), (6, None), (7, None), (8, None), (9, None), (2, ctypes.c_longlong(0)), (3, 0),
                   (4, 7), (5, 7), (10, -1.0), (11, 0), (11, 3)):
        args = list(good)
        args[i] = bad
        with pytest.raises(RuntimeError, match='status -22'):
            call('contrad_bn_relu_apply_eval', *args)


# ======================================================================================================================
# elementwise.hip: GAN losses
# ======================================================================================================================
# (N, ld, col, scale, what)
GAN_CASES = [
    (37, 1, 0, 3.0, 'dense logits'),
    (300, 5, 2, 3.0, 'column 2 of a 5-wide head output, N > 256'),
    (300, 4, 1, 30.0, 'saturating |d| ~ 30'),
    (1000, 1, 0, 100.0, 'saturating |d| ~ 100, N > 256'),
]


@pytest.mark.parametrize('kind', ['nonsat', 'wgan', 'hinge', 'lsgan'])
@pytest.mark.parametrize('case', GAN_CASES, ids=lambda c: 'N%d-ld%d-s%g' % (c[0], c[1], c[3]))
def test_gan_losses(margin, case, kind):
    N, ld, col, scale, _ = case
    head = torch.randn(3 * N, ld, device=DEV, generator=gen(N + ld)) * scale
    d = head[:, col:col + 1]
    kid = ops.GAN_LOSS_KINDS[kind]
    gout, out = flat((3,))
    ggrad, grad = flat((3 * N,))
    call('contrad_gan_d_loss', P(d), ld, N, kid, P(out), P(grad), ops._stream())
    loss, gr, gg = R.gan_d(d[:N, 0], d[2 * N:, 0], kind)
    ref_out = torch.stack([loss, d[:N, 0].double().mean(), d[2 * N:, 0].double().mean()])
    ref_grad = torch.cat([gr, torch.zeros(N, dtype=torch.float64, device=DEV), gg])
    gout1, out1 = flat((1,))
    ggrad1, grad1 = flat((N,))
    call('contrad_gan_g_loss', P(d), ld, N, kid, P(out1), P(grad1), ops._stream())
    lg, ggr = R.gan_g(d[:N, 0], kind)
    torch.cuda.synchronize()
    assert gout.intact() and ggrad.intact() and gout1.intact() and ggrad1.intact()
    what = '%s N=%d ld=%d |d|~%g' % (kind, N, ld, scale)
    check(margin, 'gan_loss', what + ' D', out, ref_out)
    check(margin, 'gan_grad', what + ' D', grad, ref_grad)
    check(margin, 'gan_loss', what + ' G', out1, lg.reshape(1))
    check(margin, 'gan_grad', what + ' G', grad1, ggr)


# ======================================================================================================================
# elementwise.hip: Adam, axpby
# ======================================================================================================================
CH = ADAM_CHUNK


def adam_tensors(sizes, seed):
    """Parameters, gradients, m, v of ``sizes`` inside NaN-padded storage: [(guards, p, g, m, v)]."""
    g = gen(seed)
    out = []
    for n in sizes:
        gp, p = flat((n,), fill=torch.randn(n, device=DEV, generator=g))
        gg, gr = flat((n,), fill=torch.randn(n, device=DEV, generator=g))
        gm, m = flat((n,), fill=torch.randn(n, device=DEV, generator=g) * 0.1)
        gv, v = flat((n,), fill=torch.rand(n, device=DEV, generator=g) * 0.01)
        out.append(((gp, gg, gm, gv), p, gr, m, v))
    return out


def test_adam_many_tensors_trajectory(margin):
    """70 tensors (two CONTRAD_ADAM_MAX_TENSORS batches), numel 1, CHUNK - 1, CHUNK, CHUNK + 1 and several chunks,
    grad_scale != 1, four steps against the float64 trajectory."""
    assert ops.ADAM_MAX_TENSORS == 64 and CH == 16384
    sizes = [[1, CH - 1, CH, CH + 1, 3 * CH + 5, 33, 256][i % 7] for i in range(70)]
    ts = adam_tensors(sizes, 11)
    lr, b1, b2, eps = f32(2e-4), f32(0.5), f32(0.999), f32(1e-8)
    state = [(p.double(), m.double(), v.double()) for _, p, _, m, v in ts]
    for step in range(1, 5):
        gs = 0.5 if step % 2 else 1.0
        if step > 1:
            g = gen(step)
            for t in ts:
                t[2].copy_(torch.randn(t[2].shape, device=DEV, generator=g))
        ops.adam_step([t[1] for t in ts], [t[2] for t in ts], [t[3] for t in ts], [t[4] for t in ts], step, lr, b1,
                      b2, eps, gs)
        state = [R.adam(p, t[2], m, v, step, lr, b1, b2, eps, gs) for (p, m, v), t in zip(state, ts)]
    torch.cuda.synchronize()
    for i, (t, (p, m, v)) in enumerate(zip(ts, state)):
        assert all(gd.intact() for gd in t[0]), i
    cat = lambda xs: torch.cat([x.reshape(-1) for x in xs])
    check(margin, 'adam', '70 tensors, 4 steps: p', cat([t[1] for t in ts]), cat([s[0] for s in state]))
    check(margin, 'adam', '70 tensors, 4 steps: m', cat([t[3] for t in ts]), cat([s[1] for s in state]))
    check(margin, 'adam', '70 tensors, 4 steps: v', cat([t[4] for t in ts]), cat([s[2] for s in state]))
    # the step against its own float64 update from the same fp32 state: the per-step kernel error
    for i in (0, 1, 4):
        t = ts[i]
        p0, m0, v0 = t[1].clone(), t[3].clone(), t[4].clone()
        ops.adam_step([t[1]], [t[2]], [t[3]], [t[4]], 5, lr, b1, b2, eps, 0.25)
        pr, mr, vr = R.adam(p0, t[2], m0, v0, 5, lr, b1, b2, eps, 0.25)
        for name, out, ref in (('p', t[1], pr), ('m', t[3], mr), ('v', t[4], vr)):
            check(margin, 'adam', 'one step from fp32 state, numel=%d: %s' % (sizes[i], name), out, ref)


@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
def test_adam_step_dev_matches_adam_step(grad_scale):
    """adam_step_dev fed with FusedAdam.hyper_values is what step_captured replays: the same bits as adam_step."""
    sizes = [1, CH + 1, 70 * 3, 5]
    params = [torch.nn.Parameter(torch.randn(n, device=DEV, generator=gen(n))) for n in sizes * 17]   # 68 tensors
    opt = FusedAdam(params, lr=2e-4, betas=(0.5, 0.999))
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen(p.numel() + 1))
    opt.step()                                                   # step 1: creates the state
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen(p.numel() + 2))
    A = [(p.data.clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for p in params]
    hyper = torch.tensor(opt.hyper_values(grad_scale), dtype=torch.float32, device=DEV)
    assert all(opt.state[p]['step'] == 2 for p in params)
    ops.adam_step([a[0] for a in A], [p.grad for p in params], [a[1] for a in A], [a[2] for a in A], 2, 2e-4, 0.5,
                  0.999, 1e-8, grad_scale)
    opt.step_captured(hyper)
    torch.cuda.synchronize()
    for p, (pa, ma, va) in zip(params, A):
        assert torch.equal(p.data, pa) and torch.equal(opt.state[p]['exp_avg'], ma)
        assert torch.equal(opt.state[p]['exp_avg_sq'], va)


@pytest.mark.parametrize('n', [1, 1000003])
def test_axpby(margin, n):
    g = gen(n)
    y0 = torch.randn(n, device=DEV, generator=g)
    gyy, y = flat((n,), fill=y0)
    gx, x = flat((n,), fill=torch.randn(n, device=DEV, generator=g))
    a, b = f32(0.999), f32(0.001)
    ops.axpby_(y, x, a, b)
    torch.cuda.synchronize()
    assert gyy.intact() and gx.intact()
    check(margin, 'axpby', 'n=%d' % n, y, a * y0.double() + b * x.double())


@pytest.mark.parametrize('n,pad', [(1, 4), (255, 4), (257, 1), (1024 * 256 + 3, 3)])
def test_pull_host_is_a_copy_bit_for_bit(n, pad):
    """contrad_pull_host (pull_kernel: the hand-over of the per-step draws, contrad_amd/hostio.py) reads device-mapped pinned
    host memory and writes n floats: bit patterns (NaN payloads, -0, denormals) arrive unchanged, nothing else is written.
    Sizes: one float, a ragged block, a misaligned destination, and one float more than the 1024 x 256 threads of the capped
    grid move in their first trip."""
    g = torch.Generator().manual_seed(n)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    bits[0] = -2 ** 31                                            # -0.0
    if n > 3:
        bits[1], bits[2], bits[3] = 0x7fc01234, 0x00000001, 0x7f800000          # a NaN payload, a denormal, +inf
    src = bits.view(torch.float32).pin_memory()
    gd, dst = flat((n,), pad=pad)
    call('contrad_pull_host', src.data_ptr(), dst.data_ptr(), n, ops._stream())             # (as hostio._pull calls it)
    torch.cuda.synchronize()
    assert gd.intact()
    assert torch.equal(dst.cpu().view(torch.int32), bits)
    assert torch.equal(src.view(torch.int32), bits)               # the source is read only
