"""GPU parity of every kernel family the conv planner can send a layer to, against float64 (tests/conv_ref64.py: an im2col
GEMM on float64 CUDA tensors that uses none of this project's kernels).

One case per reachable (path, mode, split-K) triple of ``contrad_conv2d_path`` (tests/test_conv_plan_cpu.py proves, without a
GPU, that PATH_CASES reach every triple the planner returns over the BASELINE layers and a grid of odd shapes, and that each
case's declared path is what the planner says), plus ragged variants.  Each case runs the calls the models make with every
epilogue term on -- ops.conv2d_fwd with bias, slope 0.2, gain sqrt2 and an addend; ops.conv2d_dgrad with act_ref;
ops.conv2d_wgrad with dbias -- and once with no epilogue at all.  Checked on the whole tensor:
  * max-norm error max|e| / max|ref| below the 1e-3 contract, and below a per-family tight bound, as is the rel-L2 error
    ||e||_2 / ||ref||_2 (FAMILY_TOL, set at about 5x the worst observed on an MI355X);
  * outputs are channel slices of NaN-filled buffers with a leading dimension above the channel count and a whole spare image
    before and after (dwp: spare rows and columns past K; dbias: spare floats either side): every sentinel must stay NaN;
  * a Winograd-planned case (paths 7 - 11) gives BITWISE the result of the forced entry point of the family the path query
    names (ops.conv2d_wino / conv2d_wino_wgrad): the kernel that ran is the one the query reports.

INSTANCE_CASES: inside a Winograd family the host picks a template instance by arithmetic no plan query reports (csrc/wino_host.h:
the raw-box pieces per mover thread of wino22 / wino23, the raw-box width of wino44 / wino44n).  The instances that neither
PATH_CASES nor the walks of tests/test_wino_walks_gpu.py launch (the record profiles/kernel_ledger.txt) run here through the
forced entry point on the smallest geometry that selects them; tests/kernel_ledger.py restates the selection and
tests/test_kernel_ledger_cpu.py holds each case to the instance it names.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import conv_ref64 as R
import kernel_ledger as L
from contrad_amd import ops
from contrad_amd._lib import lib

pytestmark = pytest.mark.gpu

CONTRACT = 1e-3
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))             # (the fp32 values the kernels receive)
GAIN = float(torch.tensor(math.sqrt(2.0), dtype=torch.float32))

# (path, mode, split, N, H, W, C, K, k, stride, pad, xq, yq, wq, what)
PATH_CASES = [
    (0, 0, False, 3, 5, 7, 3, 8, 3, 1, 1, 0, 1, 1, 'Cin = 3: scalar gathers, odd non-square map'),
    (0, 1, False, 2, 5, 5, 3, 5, 3, 1, 1, 1, 0, 1, 'dx of a 3-channel input'),
    (0, 2, False, 1, 1, 1, 3, 1, 1, 1, 0, 0, 0, 1, 'single pixel, Cout = 1'),
    (0, 2, True, 5, 9, 9, 3, 8, 3, 1, 1, 0, 0, 1, 'scalar gathers over split slabs'),
    (1, 0, False, 2, 3, 3, 8, 8, 1, 1, 0, 0, 1, 1, ''),
    (1, 1, False, 2, 3, 3, 8, 12, 1, 1, 0, 1, 0, 1, ''),
    (1, 2, False, 1, 1, 1, 8, 8, 1, 1, 0, 0, 0, 1, ''),
    (1, 2, True, 1, 9, 9, 8, 8, 1, 1, 0, 0, 0, 1, ''),
    (2, 0, False, 3, 4, 4, 16, 8, 1, 1, 0, 0, 1, 1, ''),
    (2, 0, True, 2, 1, 1, 512, 64, 1, 1, 0, 0, 1, 1, 'split-K head GEMM'),
    (2, 1, False, 3, 4, 4, 16, 32, 1, 1, 0, 1, 0, 1, ''),
    (2, 1, True, 2, 1, 1, 48, 512, 1, 1, 0, 1, 0, 1, 'split-K dgrad'),
    (2, 2, False, 1, 4, 4, 8, 8, 1, 1, 0, 0, 0, 1, ''),
    (2, 2, True, 5, 4, 4, 8, 8, 1, 1, 0, 0, 0, 1, ''),
    (3, 0, False, 192, 1, 1, 16, 8, 3, 1, 1, 0, 1, 1, 'pixel-major tiles, every tap but one is padding'),
    (3, 1, False, 192, 1, 1, 8, 32, 3, 1, 1, 1, 0, 1, ''),
    (3, 2, False, 16, 2, 2, 128, 8, 3, 1, 1, 0, 0, 1, ''),
    (3, 2, True, 48, 2, 2, 128, 8, 3, 1, 1, 0, 0, 1, ''),
    (4, 2, True, 16, 64, 64, 32, 32, 3, 1, 1, 0, 0, 0, 'wgrad_c32'),
    (5, 0, False, 5, 1, 1, 16, 1, 1, 1, 0, 0, 1, 1, 'the logit: one output channel'),
    (6, 0, False, 16, 64, 64, 32, 32, 3, 1, 1, 0, 0, 0, 'conv_c32'),
    (6, 1, False, 16, 64, 64, 32, 32, 3, 1, 1, 0, 0, 0, ''),
    (7, 0, False, 5, 32, 32, 16, 512, 3, 1, 1, 0, 1, 1, 'F(2x2,3x3)'),
    (7, 1, False, 5, 32, 32, 512, 32, 3, 1, 1, 1, 0, 1, ''),
    (7, 2, True, 1, 64, 64, 256, 512, 3, 1, 1, 0, 0, 1, 'F(3x3,2x2)'),
    (8, 0, False, 48, 32, 32, 8, 512, 4, 2, 1, 0, 1, 1, 'F(2x2,2x2) phases'),
    (8, 1, False, 48, 16, 16, 512, 32, 4, 2, 1, 1, 0, 1, ''),
    (8, 2, True, 16, 16, 16, 512, 512, 4, 2, 1, 0, 0, 1, ''),
    (9, 0, False, 16, 32, 32, 32, 512, 3, 1, 1, 0, 1, 1, 'F(4x4,3x3)'),
    (9, 1, False, 16, 32, 32, 512, 32, 3, 1, 1, 1, 0, 1, ''),
    (10, 0, False, 192, 33, 33, 16, 256, 3, 2, 0, 0, 1, 1, 'strided 3x3 phases'),
    (11, 0, False, 1536, 4, 4, 32, 160, 3, 1, 1, 0, 1, 1, 'F(4x4,3x3), 32-wide cout blocks'),
    (11, 1, False, 1536, 4, 4, 160, 32, 3, 1, 1, 1, 0, 1, ''),
    # ragged variants
    (2, 0, True, 4, 8, 8, 64, 96, 3, 1, 1, 1, 2, 1, 'ragged Cout: 96 of a 128-wide tile'),
    (2, 0, True, 3, 17, 17, 64, 64, 3, 1, 1, 0, 1, 1, 'odd 17 x 17 map'),
    (2, 1, True, 3, 17, 17, 64, 64, 3, 1, 1, 1, 0, 1, 'odd 17 x 17 map'),
    (9, 0, False, 229, 8, 8, 32, 512, 3, 1, 1, 0, 1, 1, 'F(4x4,3x3) 8 x 8: 8 images per item, ragged last block'),
    (7, 0, False, 75, 8, 8, 16, 512, 3, 1, 1, 0, 1, 1, 'F(2x2,3x3) 8 x 8: 4 images per item, ragged last block'),
    (7, 1, False, 75, 8, 8, 512, 16, 3, 1, 1, 1, 0, 1, ''),
]


# the same layout with the path replaced by the family of the forced entry point and `what` by the instance the host selects:
# one full image group and a ragged one (wino44n: 8 images per item on 8 x 8 maps; 32 x 32 maps: two items per image)
INSTANCE_CASES = [
    (11, 1, False, 11, 8, 8, 96, 32, 3, 1, 1, 1, 1, 1, 'wino44n::wino44n_kernel<1, 10>'),
    (11, 1, False, 3, 32, 32, 96, 32, 3, 1, 1, 1, 1, 1, 'wino44n::wino44n_kernel<1, 34>'),
]


def round4(v):
    return (v + 3) // 4 * 4


def case_lds(case):
    """(ldx, ldy, ldw) of a case: 4 * q floats past the channel count rounded to 4 (q = 0: dense)."""
    _, _, _, N, H, W, C, K, k, s, p, xq, yq, wq, _ = case
    return round4(C) + 4 * xq, round4(K) + 4 * yq, round4(K) + 4 * wq


def case_desc(case):
    _, _, _, N, H, W, C, K, k, s, p, _, _, _, _ = case
    ldx, ldy, ldw = case_lds(case)
    return ops.make_desc(N, H, W, C, K, k, k, s, p, ldx, ldy, ldw)


def case_id(case):
    P, m, sp, N, H, W, C, K, k, s, p = case[:11]
    return 'p%d-m%d%s-%dx%dx%dx%d-%d-k%ds%dp%d' % (P, m, '-split' if sp else '', N, H, W, C, K, k, s, p)


# per-family tight bounds against float64, about 5x the worst observed on an MI355X over this module (all tighter than the
# 2e-5 / 1e-4 the older tests assert for the same paths)
FAMILY_TOL = {                 # path: (max-norm, rel-L2)      observed worst (max-norm, rel-L2)
    0: (1e-6, 5e-7),           # 1.9e-7, 9.5e-8
    1: (1e-6, 7e-7),           # 2.1e-7, 1.5e-7
    2: (3e-6, 1.5e-6),         # 6.3e-7, 3.0e-7
    3: (1.5e-6, 6e-7),         # 3.1e-7, 1.2e-7
    4: (1e-6, 8e-7),           # 2.0e-7, 1.6e-7
    5: (5e-7, 5e-7),           # 9.9e-8, 9.6e-8
    6: (4e-6, 1.5e-6),         # 8.8e-7, 3.0e-7
    7: (2e-6, 1.8e-6),         # 3.9e-7, 3.6e-7
    8: (3.5e-6, 2e-6),         # 6.9e-7, 4.3e-7
    10: (3.5e-6, 1.5e-6),      # 7.0e-7, 2.9e-7
    9: (3.5e-5, 7e-6),         # 7.4e-6, 1.4e-6
    11: (3.5e-5, 7.5e-6),      # 7.3e-6, 1.5e-6
}


def check(margin, family, what, out, ref):
    emax, el2 = R.errors(out, ref)
    assert emax < CONTRACT, (what, emax)
    tmax, tl2 = FAMILY_TOL[family]
    margin('conv path %2d  max-norm' % family, emax, tmax)
    margin('conv path %2d  rel-L2' % family, el2, tl2)


class Guarded(object):
    """An NHWC tensor as the channel slice [off, off + C) of a (N + 2, H, W, ld) buffer: a spare image either side."""

    def __init__(self, N, H, W, C, ld, fill, dev):
        self.off = 4 if ld - C >= 4 else 0
        self.buf = torch.full((N + 2, H, W, ld), fill, device=dev)
        self.t = self.buf[1:N + 1, :, :, self.off:self.off + C]
        self.C = C

    def sentinels_intact(self):
        mask = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        mask[1:-1, :, :, self.off:self.off + self.C] = False
        return bool(torch.isnan(self.buf[mask]).all())


def _rand(shape, g, dev, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _input(N, H, W, C, ld, g, dev):
    """Random input in a channel slice; the spare columns / images hold 1e3 (a kernel reading them shows in the error)."""
    t = Guarded(N, H, W, C, ld, 1e3, dev)
    t.t.copy_(_rand((N, H, W, C), g, dev))
    return t.t


def _weights(case, g, dev):
    _, _, _, N, H, W, C, K, k, s, p = case[:11]
    ldw = case_lds(case)[2]
    w = torch.randn(K, C, k, k, generator=g) / math.sqrt(C * k * k)
    wp = torch.zeros(k * k * C, ldw)
    wp[:, :K] = ops.pack_weight(w)[:, :K]
    return w.to(dev), wp.to(dev)


def _forced(P, mode, inp, wp, C, K, bias, ref, slope, gain, out):
    return ops.conv2d_wino(mode, inp, wp, C, K, bias=bias, ref=ref, slope=slope, gain=gain, out=out,
                           f44=P in (9, 11), k4s2=P == 8, k3s2=P == 10)


def case_tensors(case, dev):
    """The operands of a PATH_CASES entry, drawn from the case's own generator: w, wp and, by mode, x / bias / add (forward),
    gy / act (data gradient), x / gy (weight gradient).  (Shared with tests/test_workspace_contract_gpu.py.)"""
    P, mode, split, N, H, W, C, K, k, s, p = case[:11]
    ldx, ldy, ldw = case_lds(case)
    d = case_desc(case)
    g = torch.Generator().manual_seed(1000 + PATH_CASES.index(case))
    t = {}
    t['w'], t['wp'] = _weights(case, g, dev)
    if mode == 0:
        t['x'] = _input(N, H, W, C, ldx, g, dev)
        t['bias'] = _rand((K,), g, dev, 0.3)
        t['add'] = _input(N, d.Ho, d.Wo, K, ldy, g, dev)
    elif mode == 1:
        t['gy'] = _input(N, d.Ho, d.Wo, K, ldy, g, dev)
        t['act'] = _input(N, H, W, C, ldx, g, dev)
    else:
        t['x'] = _input(N, H, W, C, ldx, g, dev)
        t['gy'] = _input(N, d.Ho, d.Wo, K, ldy, g, dev)
    return t


@pytest.mark.parametrize('case', PATH_CASES, ids=case_id)
def test_conv_path_matches_float64(case, margin):
    P, mode, split, N, H, W, C, K, k, s, p = case[:11]
    dev = torch.device('cuda')
    ldx, ldy, ldw = case_lds(case)
    d = case_desc(case)
    assert lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode) == P
    Ho, Wo = d.Ho, d.Wo
    t = case_tensors(case, dev)
    w, wp = t['w'], t['wp']
    if mode == 0:
        x, bias, add = t['x'], t['bias'], t['add']
        for epi in (True, False):
            y = Guarded(N, Ho, Wo, K, ldy, float('nan'), dev)
            kw = dict(slope=SLOPE, gain=GAIN, addend=add) if epi else {}
            ops.conv2d_fwd(x, wp, bias if epi else None, K, k, k, s, p, out=y.t, **kw)
            torch.cuda.synchronize()
            assert y.sentinels_intact(), 'forward wrote outside y'
            ref = R.fwd(x, w, bias if epi else None, s, p, **kw)
            check(margin, P, 'fwd', y.t, ref)
            if P >= 7:
                y2 = Guarded(N, Ho, Wo, K, ldy, float('nan'), dev)
                _forced(P, 0, x, wp, C, K, bias if epi else None, add if epi else None, SLOPE if epi else 1.0,
                        GAIN if epi else 1.0, y2.t)
                assert torch.equal(y.t, y2.t), 'the planned forward is not the kernel path %d names' % P
    elif mode == 1:
        gy, act = t['gy'], t['act']
        for epi in (True, False):
            dx = Guarded(N, H, W, C, ldx, float('nan'), dev)
            kw = dict(act_ref=act, slope=SLOPE, gain=GAIN) if epi else {}
            ops.conv2d_dgrad(gy, wp, (N, H, W, C), k, k, s, p, out=dx.t, **kw)
            torch.cuda.synchronize()
            assert dx.sentinels_intact(), 'data gradient wrote outside dx'
            ref = R.dgrad(gy, w, (H, W), s, p, **kw)
            check(margin, P, 'dgrad', dx.t, ref)
            if P >= 7:
                dx2 = Guarded(N, H, W, C, ldx, float('nan'), dev)
                _forced(P, 1, gy, wp, C, K, None, act if epi else None, SLOPE if epi else 1.0, GAIN if epi else 1.0, dx2.t)
                assert torch.equal(dx.t, dx2.t), 'the planned data gradient is not the kernel path %d names' % P
    else:
        x, gy = t['x'], t['gy']
        refw, refb = R.wgrad(x, gy, k, k, s, p)
        refw = refw.permute(2, 3, 1, 0).reshape(k * k * C, K)         # packed layout
        # (the fused bias gradient needs C, K and the leading dimensions in multiples of 4: an argument error otherwise)
        bias_ok = C % 4 == 0 and K % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0
        if not bias_ok:
            with pytest.raises(RuntimeError):
                ops.conv2d_wgrad(x, gy, k, k, s, p, dbias=torch.empty(K, device=dev))
        for with_bias in ((True, False) if bias_ok else (False,)):
            dwb = torch.full((k * k * C + 2, ldw), float('nan'), device=dev)
            dbb = torch.full((K + 8,), float('nan'), device=dev)
            dwp, dbias = dwb[1:-1], (dbb[4:4 + K] if with_bias else None)
            ops.conv2d_wgrad(x, gy, k, k, s, p, out=dwp, dbias=dbias)
            torch.cuda.synchronize()
            inner = torch.zeros_like(dwb, dtype=torch.bool)
            inner[1:-1, :K] = True
            assert torch.isnan(dwb[~inner]).all(), 'weight gradient wrote outside dwp[:, :K]'
            check(margin, P, 'wgrad', dwp[:, :K], refw)
            if with_bias:
                assert torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all(), 'dbias written out of range'
                check(margin, P, 'dbias', dbias, refb)
            if P in (7, 8):
                dwb2 = torch.full_like(dwb, float('nan'))
                db2 = torch.empty(K, device=dev) if with_bias else None
                ops.conv2d_wino_wgrad(x, gy, out=dwb2[1:-1], dbias=db2)
                assert torch.equal(dwp[:, :K], dwb2[1:-1, :K]), 'the planned weight gradient is not the kernel path %d names' % P
                if with_bias:
                    assert torch.equal(dbias, db2)


@pytest.mark.parametrize('case', INSTANCE_CASES, ids=lambda c: c[14])
def test_forced_winograd_instance_matches_float64(case, margin):
    """A host-selected template instance on the forced entry point: float64 parity at the family's bound with every epilogue
    term on and with none, sentinels intact, bitwise equal to a repeat."""
    P, mode, _, N, H, W, C, K, k, s, p = case[:11]
    assert L.wino_instance((N, H, W, C, K, k, s, p), mode, f44=P in (9, 11)) == case[14]
    dev = torch.device('cuda')
    ldx, ldy, ldw = case_lds(case)
    d = case_desc(case)
    Ho, Wo = d.Ho, d.Wo
    g = torch.Generator().manual_seed(2000 + INSTANCE_CASES.index(case))
    w, wp = _weights(case, g, dev)
    if mode == 0:
        inp, oshape, ldo = _input(N, H, W, C, ldx, g, dev), (N, Ho, Wo, K), ldy
        bias = _rand((K,), g, dev, 0.3)
    else:
        inp, oshape, ldo = _input(N, Ho, Wo, K, ldy, g, dev), (N, H, W, C), ldx
        bias = None
    side = _input(*oshape, ldo, g, dev)                 # the forward's addend / the data gradient's activation reference
    for epi in (True, False):
        outs = []
        for _rep in range(2):
            out = Guarded(*oshape, ldo, float('nan'), dev)
            _forced(P, mode, inp, wp, C, K, bias if epi else None, side if epi else None, SLOPE if epi else 1.0,
                    GAIN if epi else 1.0, out.t)
            torch.cuda.synchronize()
            assert out.sentinels_intact(), '%s wrote outside its output' % case[14]
            outs.append(out.t)
        if mode == 0:
            ref = R.fwd(inp, w, bias if epi else None, s, p, **(dict(slope=SLOPE, gain=GAIN, addend=side) if epi else {}))
        else:
            ref = R.dgrad(inp, w, (H, W), s, p, **(dict(act_ref=side, slope=SLOPE, gain=GAIN) if epi else {}))
        check(margin, P, case[14], outs[0], ref)
        assert torch.equal(outs[0], outs[1]), '%s is not repeatable' % case[14]


def test_the_float64_references_agree():
    """The GPU im2col references against CPU float64 F.conv2d / conv_transpose2d / autograd on one small strided shape."""
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(7)
    N, H, C, K, k, s, p = 3, 9, 5, 6, 3, 2, 1
    x = torch.randn(N, H, H, C, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(K, generator=g, dtype=torch.float64)
    Ho = (H + 2 * p - k) // s + 1
    add = torch.randn(N, Ho, Ho, K, generator=g, dtype=torch.float64)
    act = torch.randn(N, H, H, C, generator=g, dtype=torch.float64)
    gy = torch.randn(N, Ho, Ho, K, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2)
    y = F.leaky_relu(F.conv2d(xc, w, b, stride=s, padding=p), SLOPE) * GAIN + add.permute(0, 3, 1, 2)
    yg = R.fwd(x.to(dev), w, b, s, p, SLOPE, GAIN, add.to(dev))
    dx = F.conv_transpose2d(gy.permute(0, 3, 1, 2), w, stride=s, padding=p, output_padding=H - ((Ho - 1) * s - 2 * p + k))
    dx = dx * torch.where(act.permute(0, 3, 1, 2) > 0, torch.tensor(GAIN, dtype=torch.float64),
                          torch.tensor(GAIN * SLOPE, dtype=torch.float64))
    dxg = R.dgrad(gy.to(dev), w, (H, H), s, p, act.to(dev), SLOPE, GAIN)
    w0 = w.clone().requires_grad_()
    b0 = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    F.conv2d(xc, w0, b0, stride=s, padding=p).backward(gy.permute(0, 3, 1, 2))
    dwg, dbg = R.wgrad(x.to(dev), gy.to(dev), k, k, s, p)
    for got, want in ((yg, y.permute(0, 2, 3, 1)), (dxg, dx.permute(0, 2, 3, 1)), (dwg, w0.grad), (dbg, b0.grad)):
        assert R.errors(got, want.to(dev))[0] < 1e-12


def test_a_null_workspace_runs_the_direct_kernels(margin):
    """The path query describes the plan WITH a workspace of *_workspace_bytes (include/contrad_hip.h).  Without one a
    Winograd-planned shape runs the direct kernels: the results hold the direct families' bound against float64, and differ
    from the Winograd result (a different kernel ran)."""
    dev = torch.device('cuda')
    case = next(c for c in PATH_CASES if c[:2] == (9, 0))
    P, _, _, N, H, W, C, K, k, s, p = case[:11]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, H, W, C, generator=g).to(dev)
    w = (torch.randn(K, C, 3, 3, generator=g) / math.sqrt(9 * C)).to(dev)
    wp = ops.pack_weight(w.cpu()).to(dev)
    b = torch.randn(K, generator=g).to(dev)
    d = ops.make_desc(N, H, W, C, K, 3, 3, 1, 1, C, K, wp.stride(0))
    assert lib().raw('contrad_conv2d_path')(ctypes.byref(d), 0) == 9
    y = torch.empty(N, H, W, K, device=dev)
    lib().call('contrad_conv2d_fwd_add', ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(b), ops._p(None), ops._p(y),
               SLOPE, GAIN, ops._p(None), ctypes.c_longlong(0), ops._stream())
    yw = ops.conv2d_fwd(x, wp, b, K, 3, 3, 1, 1, slope=SLOPE, gain=GAIN)
    ref = R.fwd(x, w, b, 1, 1, SLOPE, GAIN)
    check(margin, 2, 'fwd without workspace', y, ref)
    check(margin, 9, 'fwd with workspace', yw, ref)
    assert not torch.equal(y, yw)
    # data gradient of the mirrored shape (gy has the 512 channels)
    dd = ops.make_desc(N, H, W, K, C, 3, 3, 1, 1, K, C, round4(C))
    wt = (torch.randn(C, K, 3, 3, generator=g) / math.sqrt(9 * C)).to(dev)
    wpt = ops.pack_weight(wt.cpu()).to(dev)
    assert lib().raw('contrad_conv2d_path')(ctypes.byref(dd), 1) == 9
    gy = torch.randn(N, H, W, C, generator=g).to(dev)
    act = torch.randn(N, H, W, K, generator=g).to(dev)
    dx = torch.empty(N, H, W, K, device=dev)
    lib().call('contrad_conv2d_dgrad_ws', ctypes.byref(dd), ops._p(gy), ops._p(wpt), ops._p(dx), ops._p(act),
               SLOPE, GAIN, ops._p(None), ctypes.c_longlong(0), ops._stream())
    dxw = ops.conv2d_dgrad(gy, wpt, (N, H, W, K), 3, 3, 1, 1, act_ref=act, slope=SLOPE, gain=GAIN)
    refd = R.dgrad(gy, wt, (H, W), 1, 1, act, SLOPE, GAIN)
    check(margin, 2, 'dgrad without workspace', dx, refd)
    check(margin, 9, 'dgrad with workspace', dxw, refd)
    assert not torch.equal(dx, dxw)
