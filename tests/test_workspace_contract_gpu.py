"""The workspace contract of include/contrad_hip.h on the GPU: every launch that takes scratch runs with EXACTLY
``*_workspace_bytes`` bytes, 16-byte (not 32-byte) aligned, poisoned, between guard bands (tests/ws_guard.py).

Each case runs its op through the ``ops`` wrapper once plainly (the ordinary grow-only cache) and three times under the
harness, once per poison word (a quiet NaN, all ones, zero), on the inputs, guarded outputs and float64 reference of the op's
own parity module (imported, not copied).  It asserts
  * both guard bands of every request intact (no write outside [workspace, workspace + workspace_bytes));
  * the requests that were logged: how many, and each ``nbytes`` equal to the query's answer;
  * the output under the NaN poison within the op's existing float64 bound (the ``check`` of its parity module);
  * the three poisoned outputs and the plain one bitwise equal (nothing unwritten is read, nothing depends on what an earlier
    call left, and the exact-size workspace took the planned path, not the direct kernels a too-small one falls to);
  * the output's own NaN sentinels intact.
A case whose query answers 0 makes no request: it asserts that, and that the outputs equal the plain ones.

CASE_TABLES lists every case id; tests/test_ws_guard_cpu.py holds a table from every ``contrad_*_workspace_bytes`` prototype
of the header to the ids here that exercise it.  ``test_zz_request_counts`` prints the requests logged per family.
"""
import collections
import ctypes
import math

import numpy as np
import pytest
import torch

from contrad_amd import ops
from contrad_amd._lib import lib
from ws_guard import POISONS, WorkspaceGuard

import test_conv_paths_gpu as TC
import test_dstep_kernels_gpu as TD
import test_augment_kernels_gpu as TA
import test_baselines_gpu as TB
import test_sg2_ops_kernels_gpu as TS
import test_gp_kernels_gpu as TG
import test_linhead_gpu as TL
import test_knn_gpu as TK
import test_swd_kernels_gpu as TW
import test_kid_kernels_gpu as TKK
import test_fd_gpu as TF
import test_contrast_stats_gpu as TCS

import aug_ref64 as A
import baselines_ref64 as RB
import conv_ref64 as R
import dstep_ref64 as RD
import gp_ref64 as RG
import kid_ref64 as RK
import knn_ref64 as RN
import linhead_ref64 as RL
import sg2_ref64 as S
import swd_ref64 as RW

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
REQUESTS = collections.Counter()          # family -> workspace requests logged under the harness in this session


def query(name, *args):
    return int(lib().raw(name)(*args))


def LL(v):
    return ctypes.c_longlong(v)


def bits(t):
    t = t.detach().contiguous()
    if t.is_floating_point():
        return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Run(object):
    """What one run of a case leaves: ``outs`` (tensors, compared bitwise between runs and handed to the case's ``verify``)
    and ``intact`` (callables that say whether the outputs' own NaN sentinels survived)."""

    def __init__(self, outs, intact=()):
        self.outs, self.intact = list(outs), list(intact)


def contract(family, run, verify, expect):
    """``run()`` once plainly and once per poison under the harness.  ``expect``: the ``nbytes`` of the requests one run
    must make, in order ([]: every query involved answers 0, and then only equality with the plain run is asserted).
    Returns the plain run."""
    plain = run()
    torch.cuda.synchronize()
    assert all(ok() for ok in plain.intact), '%s: the plain run wrote outside its output' % family
    runs = {}
    for name, word in POISONS.items():
        with WorkspaceGuard(word) as g:
            r = run()
            g.check()
        assert [q.nbytes for q in g.log] == list(expect), (family, name, [repr(q) for q in g.log], expect)
        REQUESTS[family] += len(g.log)
        assert all(ok() for ok in r.intact), '%s (%s): wrote outside its output' % (family, name)
        assert len(r.outs) == len(plain.outs)
        for i, (a, b) in enumerate(zip(r.outs, plain.outs)):
            assert same_bits(a, b), '%s: output %d under the %s poison differs from the plain run (%d elements, NaN: %s)' % (
                family, i, name, int((bits(a) != bits(b)).sum()), bool(torch.isnan(a).any()) if a.is_floating_point() else False)
        runs[name] = r
    if expect:
        verify(runs['qnan'])
    return plain


# ======================================================================================================================
# conv engine: every PATH_CASES entry with the epilogue on; paths 7 - 11 on the forced entry point as well
# ======================================================================================================================
def _wino_query(P, d, mode):
    if P in (9, 11):
        return query('contrad_conv2d_wino44_workspace_bytes', ctypes.byref(d))
    return query('contrad_conv2d_wino_workspace_bytes', ctypes.byref(d), mode)


CONV_NEEDS_REQUEST = [c for c in TC.PATH_CASES if c[2] or c[0] >= 7]


def test_conv_cases_that_must_ask_for_scratch():
    assert len(CONV_NEEDS_REQUEST) == 24
    for case in TC.PATH_CASES:
        d, mode = TC.case_desc(case), case[1]
        q = query(('contrad_conv2d_fwd_workspace_bytes', 'contrad_conv2d_dgrad_workspace_bytes',
                   'contrad_conv2d_wgrad_workspace_bytes')[mode], ctypes.byref(d))
        assert q >= 0
        if case in CONV_NEEDS_REQUEST:
            assert q > 0, TC.case_id(case)


@pytest.mark.parametrize('case', TC.PATH_CASES, ids=TC.case_id)
def test_conv_workspace_contract(case, margin):
    P, mode, split, N, H, W, C, K, k, s, p = case[:11]
    ldx, ldy, ldw = TC.case_lds(case)
    t = TC.case_tensors(case, DEV)
    d, w, wp = TC.case_desc(case), t['w'], t['wp']
    assert query('contrad_conv2d_path', ctypes.byref(d), mode) == P
    Ho, Wo = d.Ho, d.Wo
    SLOPE, GAIN = TC.SLOPE, TC.GAIN
    fam = 'conv'
    if mode == 0:
        q = query('contrad_conv2d_fwd_workspace_bytes', ctypes.byref(d))

        def run(forced=False):
            y = TC.Guarded(N, Ho, Wo, K, ldy, NAN, DEV)
            if forced:
                TC._forced(P, 0, t['x'], wp, C, K, t['bias'], t['add'], SLOPE, GAIN, y.t)
            else:
                ops.conv2d_fwd(t['x'], wp, t['bias'], K, k, k, s, p, slope=SLOPE, gain=GAIN, out=y.t, addend=t['add'])
            return Run([y.t], [y.sentinels_intact])
        ref = []

        def verify(r):
            if not ref:
                ref.append(R.fwd(t['x'], w, t['bias'], s, p, slope=SLOPE, gain=GAIN, addend=t['add']))
            TC.check(margin, P, 'fwd', r.outs[0], ref[0])
    elif mode == 1:
        q = query('contrad_conv2d_dgrad_workspace_bytes', ctypes.byref(d))

        def run(forced=False):
            dx = TC.Guarded(N, H, W, C, ldx, NAN, DEV)
            if forced:
                TC._forced(P, 1, t['gy'], wp, C, K, None, t['act'], SLOPE, GAIN, dx.t)
            else:
                ops.conv2d_dgrad(t['gy'], wp, (N, H, W, C), k, k, s, p, act_ref=t['act'], slope=SLOPE, gain=GAIN, out=dx.t)
            return Run([dx.t], [dx.sentinels_intact])
        ref = []

        def verify(r):
            if not ref:
                ref.append(R.dgrad(t['gy'], w, (H, W), s, p, act_ref=t['act'], slope=SLOPE, gain=GAIN))
            TC.check(margin, P, 'dgrad', r.outs[0], ref[0])
    else:
        q = query('contrad_conv2d_wgrad_workspace_bytes', ctypes.byref(d))
        bias_ok = C % 4 == 0 and K % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0      # (as the parity module: an argument error otherwise)

        def run(forced=False):
            dwb = torch.full((k * k * C + 2, ldw), NAN, device=DEV)
            dbb = torch.full((K + 8,), NAN, device=DEV)
            dwp, dbias = dwb[1:-1], (dbb[4:4 + K] if bias_ok else None)
            if forced:
                ops.conv2d_wino_wgrad(t['x'], t['gy'], out=dwp, dbias=dbias)
            else:
                ops.conv2d_wgrad(t['x'], t['gy'], k, k, s, p, out=dwp, dbias=dbias)
            inner = torch.zeros_like(dwb, dtype=torch.bool)
            inner[1:-1, :K] = True
            intact = [lambda: bool(torch.isnan(dwb[~inner]).all())]
            if bias_ok:
                intact.append(lambda: bool(torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all()))
            return Run([dwp[:, :K]] + ([dbias] if bias_ok else []), intact)
        ref = []

        def verify(r):
            if not ref:
                refw, refb = R.wgrad(t['x'], t['gy'], k, k, s, p)
                ref.extend([refw.permute(2, 3, 1, 0).reshape(k * k * C, K), refb])
            TC.check(margin, P, 'wgrad', r.outs[0], ref[0])
            if bias_ok:
                TC.check(margin, P, 'dbias', r.outs[1], ref[1])
    assert q >= 0
    if case in CONV_NEEDS_REQUEST:
        assert q > 0, 'the plan of this case needs scratch'
    # (ops.conv2d_wgrad asks whatever the query says; forward and data gradient make no request when it says 0)
    expect = [q] if (q > 0 or mode == 2) else []
    plain = contract(fam, run, verify, expect)
    if P >= 7 and (mode < 2 or P in (7, 8)):
        qf = _wino_query(P, d, mode)
        assert qf >= 0
        forced = contract('conv forced', lambda: run(True), verify, [qf])
        for a, b in zip(plain.outs, forced.outs):
            assert same_bits(a, b), 'the planned call is not the kernel path %d names' % P


# ======================================================================================================================
# ntxent.hip through ops.contrast_fwd / contrast_bwd and the paired two-problem launch
# ======================================================================================================================
def _contrast_case(what):
    return next(c for c in TD.CONTRAST_CASES if c[3].startswith(what))


CONTRAST_WS_CASES = [_contrast_case('DP=64, R=100'), _contrast_case('DP=128, R=192'), _contrast_case('DP=256, R=210'),
                     _contrast_case('DP=64, D=3: scalar staging'), _contrast_case('NT-Xent N=1'),
                     _contrast_case('R=8256 > 8192')]
# the other problem of the paired launch (the case's mode -> N, mode), at the case's own D: csrc/ntxent.hip pairs two problems
# in ONE launch only when they share a kernel instance, and the partner's R differs, so the grid is the larger problem's
_CONTRAST_PARTNER = {0: (33, 1), 1: (50, 0)}
CONTRAST_ID = lambda c: 'N%d-D%d-m%d' % c[:3]


def _contrast_problem(N, D, mode):
    z = TD.contrast_z(N, D, mode)
    return z, z.shape[0]


@pytest.mark.parametrize('case', CONTRAST_WS_CASES, ids=CONTRAST_ID)
def test_contrast_workspace_contract(case, margin):
    N, D, mode, _ = case
    temp, gs_val = 0.1, 0.375
    z, R_ = _contrast_problem(N, D, mode)
    if N >= 4128:
        assert TD.contrast_splits(R_) == 1
    gs = torch.full((1,), gs_val, device=DEV)
    q = query('contrad_contrast_workspace_bytes', R_, D)
    assert q > 0
    refs = {}

    def reference(key, zz, n, m):
        if key not in refs:
            refs[key] = RD.contrast(zz, n, m, temp)
        return refs[key]

    def check_problem(tag, zz, n, m, loss, lse, dz, dz_scale):
        loss_ref, lse_ref, dz_ref = reference(tag, zz, n, m)
        what = '%s N=%d D=%d mode=%d' % (tag, n, zz.shape[1], m)
        TD.check(margin, 'contrast_loss', what, loss, loss_ref.reshape(1))
        TD.check(margin, 'contrast_lse', what, lse, lse_ref)
        TD.check(margin, 'contrast_dz', what, dz, dz_ref * dz_scale)

    def run():
        loss, lse = ops.contrast_fwd(z, N, mode, temp)
        dz = ops.contrast_bwd(z, lse, N, mode, temp)
        dz2 = ops.contrast_bwd(z, lse, N, mode, temp, grad_scale=gs)
        return Run([loss, lse, dz, dz2])

    def verify(r):
        loss, lse, dz, dz2 = r.outs
        check_problem('single', z, N, mode, loss, lse, dz, 1.0)
        TD.check(margin, 'contrast_dz', 'single grad_scale', dz2, reference('single', z, N, mode)[2] * gs_val)
    single = contract('ntxent', run, verify, [q, q, q])

    (Np, mp), Dp = _CONTRAST_PARTNER[mode], D
    zp, Rp = _contrast_problem(Np, Dp, mp)
    assert Rp != R_
    both = ops.round_up(q, 16) + ops.round_up(query('contrad_contrast_workspace_bytes', Rp, Dp), 16)

    def run_pair():
        l1, lse1, l2, lse2 = ops.contrast_fwd_pair(z, N, mode, zp, Np, mp, temp)
        dz1, dzp = ops.contrast_bwd_pair(z, lse1, N, mode, None, zp, lse2, Np, mp, gs, temp)
        return Run([l1, lse1, dz1, l2, lse2, dzp])

    def verify_pair(r):
        l1, lse1, dz1, l2, lse2, dzp = r.outs
        check_problem('single', z, N, mode, l1, lse1, dz1, 1.0)
        check_problem('partner', zp, Np, mp, l2, lse2, dzp, gs_val)
    pair = contract('ntxent pair', run_pair, verify_pair, [both, both])
    for a, b in zip(single.outs[:3], pair.outs[:3]):
        assert same_bits(a, b), 'the paired launch is not bitwise the single call'


# ======================================================================================================================
# elementwise.hip / conv_small.hip: colstats, the fused BatchNorm statistics, bn_relu_bwd, rgb_conv_wgrad
# ======================================================================================================================
COLSTATS_ID = lambda c: 'M%d-K%d-ld%d-m%d-a%d' % c[:5]


@pytest.mark.parametrize('case', TD.COLSTATS_CASES, ids=COLSTATS_ID)
@pytest.mark.parametrize('with_sq', [True, False], ids=['sq', 'nosq'])
def test_colstats_workspace_contract(case, with_sq, margin):
    M, K, ld, mis, acc, _ = case
    x, base = TD.colstats_inputs(case, with_sq)
    nstat = 2 if with_sq else 1
    q = query('contrad_colstats_workspace_bytes', LL(M), K, int(with_sq))
    assert q > 0

    def run():
        gout, out = TD.flat((nstat, K), fill=base)
        ops.colstats(x, with_sq=with_sq, out=out, accumulate=acc)
        return Run([out], [gout.intact])

    def verify(r):
        ref = RD.colstats(x)[:nstat]
        if acc:
            ref = ref + base.double()
        what = 'M=%d K=%d ld=%d sq=%d' % (M, K, ld, with_sq)
        TD.check(margin, 'colstats', what + ' sum', r.outs[0][0], ref[0])
        if with_sq:
            TD.check(margin, 'colstats', what + ' sumsq', r.outs[0][1], ref[1])
    contract('colstats', run, verify, [q])


# (M, K, conv bias): G_SNDCGAN's 8 x 8 BatchNorm at N = 64, and the odd sizes of tests/test_bn_fused_gpu.py (scalar partial kernel,
# a last partial block that is not full, fewer channels than a block of the reduce)
BN_WS_CASES = [(64 * 64, 256, True), (1000, 37, True), (33, 5, False), (70000, 130, True)]


@pytest.mark.parametrize('M,K,has_bias', BN_WS_CASES)
def test_bn_batch_stats_workspace_contract(M, K, has_bias, margin):
    """ops.bn_batch_stats (the statistics reduce and the running update in one pair of launches) and ops.bn_relu_bwd (the
    same workspace query) against the float64 references and bounds of tests/test_dstep_kernels_gpu.py's test_bn_relu."""
    x0, gamma, beta = TD.bn_inputs(M, K, 0.0, M + K)
    x = x0.contiguous()
    g = TD.gen(7)
    rm0, rv0 = torch.randn(K, device=DEV, generator=g), torch.rand(K, device=DEV, generator=g) + 0.5
    cb = torch.randn(K, device=DEV, generator=g) * 0.1 if has_bias else None
    dy = torch.randn(M, K, device=DEV, generator=g)
    eps = 1e-5
    q = query('contrad_colstats_workspace_bytes', LL(M), K, 1)

    def run():
        grm, rm = TD.flat((K,), fill=rm0)
        grv, rv = TD.flat((K,), fill=rv0)
        nbt = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        nbt[1] = 41
        stats = ops.bn_batch_stats(x, cb, 0.1, rm, rv, nbt[1:2])
        y = torch.empty_like(x)
        ops.bn_relu_apply(x, y, stats, float(M), gamma, beta, eps)
        dx, dgamma, dbeta = ops.bn_relu_bwd(dy, x, stats, float(M), gamma, beta, eps)
        return Run([stats, rm, rv, nbt, y, dx, dgamma, dbeta], [grm.intact, grv.intact])

    def verify(r):
        stats, rm, rv, nbt, y, dx, dgamma, dbeta = r.outs
        what = 'fused M=%d K=%d' % (M, K)
        ref = RD.colstats(x)
        TD.check(margin, 'colstats', what + ' sum', stats[0], ref[0])
        TD.check(margin, 'colstats', what + ' sumsq', stats[1], ref[1])
        rm_ref, rv_ref = RD.bn_running(rm0, rv0, x, cb, 0.1)
        TD.check(margin, 'bn_running', what + ' mean', rm, rm_ref)
        TD.check(margin, 'bn_running', what + ' var', rv, rv_ref)
        assert nbt.tolist() == [-7, 42, -7]
        dx_ref, dg_ref, db_ref = RD.bn_relu_bwd(dy, x, gamma, beta, eps, mask=y > 0)
        TD.check(margin, 'bn_bwd', what + ' dx', dx, dx_ref)
        TD.check(margin, 'bn_bwd', what + ' dgamma', dgamma, dg_ref)
        TD.check(margin, 'bn_bwd', what + ' dbeta', dbeta, db_ref)
    contract('bn stats', run, verify, [q, q])


RGB_ID = lambda c: 'N%d-%dx%d-K%d-k%d' % c[:5]


@pytest.mark.parametrize('case', TD.RGB_FWD_CASES, ids=RGB_ID)
def test_rgb_conv_wgrad_workspace_contract(case, margin):
    N, H, W, K, k, has_bias, ye, _ = case
    img, _w, _gb, _bias, gyv = TD.rgb_inputs(case)
    q = query('contrad_rgb_conv_wgrad_workspace_bytes', N, 3, H, W, K, k)
    assert q > 0

    def run():
        gdw = TD.Guard(k * k * 3, K, ld=K + 8)
        gdb, db = TD.flat((K,))
        ops.rgb_conv_wgrad(img, gyv, k, 2.0, -1.0, gdw.view, db)
        return Run([gdw.view, db], [gdw.intact, gdb.intact])

    def verify(r):
        dw_ref, db_ref = RD.rgb_wgrad(img, gyv, k, 2.0, -1.0)
        what = 'N=%d %dx%d K=%d k=%d' % (N, H, W, K, k)
        TD.check(margin, 'rgb_wgrad', what + ' dw', ops.unpack_weight(r.outs[0], K, 3, k, k), dw_ref)
        TD.check(margin, 'rgb_wgrad', what + ' dbias', r.outs[1], db_ref)
    contract('rgb wgrad', run, verify, [q])


# ======================================================================================================================
# augment.hip / baseline_aug.hip
# ======================================================================================================================
def _aug_case(H, W, cf, hc):
    return next(c for c in TA.AUG_CASES if c[1:5] == (H, W, cf, hc))


# the CIFAR size (LDS form) and the smallest multi-pass forward (nparts = 2, ragged)
SIMCLR_FWD_CASES = [_aug_case(32, 32, -1, 1), _aug_case(74, 74, 0, 1)]
# the smallest image whose backward takes the four-launch form, and one size below it (the largest LDS backward)
SIMCLR_BWD_CASES = [_aug_case(43, 43, -1, 1), _aug_case(42, 42, -1, 1)]
AUG_ID = lambda c: '%dx%d-cf%d-c%d' % c[1:5]


def test_simclr_cases_sit_on_the_form_boundary():
    assert [TA.fwd_form(c[1], c[2]) for c in SIMCLR_FWD_CASES] == ['lds', 'multipass']
    assert [TA.bwd_form(c[1], c[2]) for c in SIMCLR_BWD_CASES] == ['multipass', 'lds']
    small, large = SIMCLR_BWD_CASES[1], SIMCLR_BWD_CASES[0]
    assert large[1] == small[1] + 1 and large[2] == small[2] + 1
    q = lambda c: query('contrad_simclr_augment_bwd_workspace_bytes', c[0], c[1], c[2])
    assert q(large) > q(small)


@pytest.mark.parametrize('case', SIMCLR_FWD_CASES, ids=AUG_ID)
def test_simclr_forward_workspace_contract(case, margin):
    B, H, W, cf, hc, _ = case
    P, x, _ = TA.case_inputs(case)
    xd, Pd = x.to(DEV), P.to(DEV)
    q = query('contrad_simclr_workspace_bytes', B, H, W)

    def run():
        gy = TA.Guard(tuple(xd.shape))
        ops.simclr_augment(xd, Pd, cf, hc, out=gy.view)
        return Run([gy.view], [gy.intact])

    def verify(r):
        TA.check(margin, 'aug_fwd', '%dx%d cf=%d contrast=%d %s' % (H, W, cf, hc, TA.fwd_form(H, W)), r.outs[0],
                 A.simclr(xd, Pd, cf, hc))
    contract('simclr fwd', run, verify, [q])


@pytest.mark.parametrize('case', SIMCLR_BWD_CASES, ids=AUG_ID)
def test_simclr_backward_workspace_contract(case, margin):
    B, H, W, cf, hc, _ = case
    P, x, gout = TA.case_inputs(case)
    xd, Pd, gd = x.to(DEV), P.to(DEV), gout.to(DEV)
    q = query('contrad_simclr_augment_bwd_workspace_bytes', B, H, W)

    def run():
        return Run([ops.simclr_augment_bwd(xd, Pd, gd, cf, hc)])

    def verify(r):
        gi = r.outs[0]
        ref, nK, flips = A.resolve_kinks(xd, Pd, gd, cf, hc, gi)
        assert nK < 0.005 * x.numel(), nK
        TA.check(margin, 'aug_bwd', '%dx%d cf=%d contrast=%d %s |K|=%d flipped %d' % (H, W, cf, hc, TA.bwd_form(H, W), nK, flips),
                 gi, ref)
    contract('simclr bwd', run, verify, [q])


@pytest.mark.parametrize('H,W', [(64, 64), (32, 32)])
def test_diffaug_workspace_contract(H, W, margin):
    B, policy = 5, 'color,translation,cutout'
    x, gy, P = TB.diffaug_inputs(H, W, B)
    bits_ = ops.diffaug_policy_bits(policy)
    q = query('contrad_diffaug_workspace_bytes', B, H, W)
    assert q == (B * 3 * 4 if not TB.small_form(H, W) else 16)
    gx, ggy, gp = TB.Guard(tuple(x.shape), x), TB.Guard(tuple(x.shape), gy), TB.Guard(tuple(P.shape), P)

    def run():
        go, gb = TB.Guard(tuple(x.shape)), TB.Guard(tuple(x.shape))
        ops.diffaug(gx.view, gp.view, bits_, out=go.view)
        ops.diffaug(ggy.view, gp.view, bits_, backward=True, out=gb.view)
        return Run([go.view, gb.view], [go.intact, gb.intact, gx.intact, ggy.intact, gp.intact])

    def verify(r):
        what = '%dx%d B=%d %s' % (H, W, B, policy)
        TB.check(margin, 'diffaug_fwd', what, r.outs[0].cpu(), RB.diffaug_forward(x, P, policy))
        TB.check(margin, 'diffaug_bwd', what, r.outs[1].cpu(), RB.diffaug_backward(gy, P, policy))
    contract('diffaug', run, verify, [q, q])


# ======================================================================================================================
# stylegan2_ops.hip: sumsq, nhwc_dot; gp.hip: gp_penalty
# ======================================================================================================================
@pytest.mark.parametrize('n', [1, 4095, 4096 * 1024 + 3])
def test_sumsq_workspace_contract(n, margin):
    gx = TS.Guard((n,), fill=TS.randn(n, seed=n))
    scale = 0.125
    q = query('contrad_sumsq_workspace_bytes', LL(n))
    assert q == min(-(-n // 4096), 1024) * 4

    def run():
        return Run([ops.sumsq(gx.view, scale)])

    def verify(r):
        TS.check(margin, 'sumsq', 'n=%d' % n, r.outs[0].view(1), S.sumsq(gx.view, scale).view(1))
    contract('sumsq', run, verify, [q])


DOT_ID = lambda c: 'N%d-HW%d-C%d-b%d' % c[:4]


@pytest.mark.parametrize('case', TS.DOT_CASES, ids=DOT_ID)
def test_nhwc_dot_workspace_contract(case, margin):
    N, HW, C, bpc, what = case
    S_ = TS.nhwc_dot_segments(N, HW)
    ga = TS.Guard((N, HW, C), fill=TS.randn(N, HW, C, seed=HW))
    gb = TS.Guard((N, HW, C) if bpc else (N, HW), fill=TS.randn(*((N, HW, C) if bpc else (N, HW)), seed=HW + 1))
    q = query('contrad_nhwc_dot_workspace_bytes', N, LL(HW), C)
    assert q == N * S_ * C * 4
    a4 = ga.view.view(N, HW, 1, C)
    b4 = gb.view.view(N, HW, 1, C) if bpc else gb.view

    def run():
        return Run([ops.nhwc_dot(a4, b4, per_channel=bool(bpc))])

    def verify(r):
        TS.check(margin, 'nhwc_dot', '%s S=%d' % (what, S_), r.outs[0], S.nhwc_dot(ga.view, gb.view, N, HW, C, bpc))
    contract('nhwc_dot', run, verify, [q])


# the one-workgroup form at the workload's image, and the two-launch form (a row just above 16 KiB)
@pytest.mark.parametrize('shape', [(6, 3, 32, 32), (3, 3, 66, 66)], ids=lambda s: 'x'.join(map(str, s)))
def test_gp_penalty_workspace_contract(shape, margin):
    N = shape[0]
    grad = TG.penalty_inputs(shape, sum(shape))
    gg = TG.Guard(grad.shape, grad)
    q = query('contrad_gp_penalty_workspace_bytes', N, LL(math.prod(shape[1:])))
    assert q == (16 if TG.small_form(shape) else N * 4 * 4)

    def run():
        gc = TG.Guard(grad.shape, None)
        out, norms, cot = ops.gp_penalty(gg.view, TG.LBD, cot=gc.view)
        return Run([out, norms, cot], [gc.intact, gg.intact])

    def verify(r):
        out, norms, cot = (o.cpu() for o in r.outs)
        value, rnorms, rcot = RG.penalty(grad, TG.LBD)
        what = '%s workspace contract' % (shape,)
        TG.check(margin, 'gp_penalty_fwd', what + ' norms', norms, rnorms)
        zero = rnorms == 0
        assert zero.any() and (norms[zero] == 0).all() and (cot[zero] == 0).all(), what
        TG.check(margin, 'gp_penalty_fwd', what + ' value', out, value.reshape(1))
        TG.check(margin, 'gp_penalty_cot', what + ' cot', cot, rcot)
    contract('gp_penalty', run, verify, [q])


# ======================================================================================================================
# linhead.hip: the counter line and the per-row words of the workspace start poisoned, twice on the same meters
# ======================================================================================================================
def _linhead_case(N, K, C):
    return next(c for c, _form in TL.CASES if c[:3] == (N, K, C))


LINHEAD_WS_CASES = [_linhead_case(70, 200, 3), _linhead_case(37, 301, 7), _linhead_case(5, 8192, 128)]
LINHEAD_ID = lambda c: '%dx%dx%d' % c[:3]


@pytest.mark.parametrize('case', LINHEAD_WS_CASES, ids=LINHEAD_ID)
def test_linhead_workspace_contract(case, margin):
    N, K, C, dld, c0, scale = case
    Sp, ct, _rt = ops.linhead_plan(N, K, C)
    if (N, K, C) == (5, 8192, 128):
        assert Sp > 1 and ct == 8
    if (N, K, C) == (37, 301, 7):
        assert c0 % 4 != 0
    F_, W_, b_, y = TL.draw(N, K, C, seed=TL.SEEDS.get((N, K, C), N + K + C), scale=scale)
    ref = RL.head_ref64(F_, W_, b_, y, lr=0.1)
    Fd = TL.strided(F_.to(DEV), K + dld, c0)
    gW, gb, yd = TL.Guard((C, K), 4, W_), TL.Guard((C,), 4, b_), y.to(DEV)
    q = query('contrad_linhead_workspace_bytes', N, K, C)
    assert q == 4 * (64 + 4 * N + Sp * N * C)

    def run():
        gl, gd = TL.Guard((N, C)), TL.Guard((N, C))
        gm = TL.Guard((4,), 1, torch.zeros(4, dtype=TL.f64), dtype=TL.f64)
        seen = []
        for _ in range(2):              # twice on the same meters: the arrival counter is reset from a poisoned start both times
            ops.linhead_fwd(Fd, gW.view, gb.view, y=yd, logits=gl.view, dlogits=gd.view, meters=gm.view)
            seen.append(gm.view.clone())
        return Run([gl.view, gd.view] + seen, [gl.intact, gd.intact, gm.intact, gW.intact, gb.intact])

    def verify(r):
        logits, dlogits, m1, m2 = r.outs
        TL.check(margin, 'logits', logits, ref['logits'])
        TL.check(margin, 'dlogits', dlogits, ref['dlogits'])
        margin('linhead loss max-norm', abs(m1[0].item() / N - ref['loss'].item()) / abs(ref['loss'].item()), TL.FAMILY_TOL['loss'][0])
        assert int(RL.near_tie_rows(ref['logits'], y).sum()) == 0
        TL.check_hits(m1, ref, y, N)
        assert same_bits(m2, m1 * 2)                                   # (the second call adds the very same four numbers)
    contract('linhead', run, verify, [q, q])


# ======================================================================================================================
# the evaluators: knn_select, swd gather / abs-diff, the kid_sums family
# ======================================================================================================================
def test_knn_select_workspace_contract():
    """contrad_knn_select_workspace_bytes answers 0 at every valid shape (this form keeps its selection state in LDS), so there
    is no smallest shape with scratch: the case asserts the 0, that no request is made, and the outputs of the plain run."""
    for shape in TK.SHAPES:
        assert query('contrad_knn_select_workspace_bytes', *shape) == 0
    shape = (5, 300, 200, 10)
    M, n, k, C = shape
    variants, labels = TK._inputs(shape)
    S_dev, labels_dev = torch.from_numpy(variants['ties']).cuda(), torch.from_numpy(labels).cuda()

    def run():
        return Run(ops.knn_select(S_dev, n, labels_dev, C, k, TK.INV_TEMP))
    plain = contract('knn_select', run, None, [])
    r_idx, r_val, _r_sc, r_pred = RN.select_and_vote(variants['ties'], labels, C, k, TK.INV_TEMP)
    assert np.array_equal(plain.outs[0].cpu().numpy(), r_idx) and np.array_equal(plain.outs[3].cpu().numpy(), r_pred)
    assert np.array_equal(plain.outs[1].cpu().numpy().view(np.uint32), r_val.view(np.uint32))


@pytest.mark.parametrize('n,size,nhoods', [(3, 16, 5), (2, 64, 300)])
def test_swd_gather_workspace_contract(n, size, nhoods, margin):
    level, pos, dev_level, cx, cy = TW._gather_inputs(n, size, nhoods)
    n_desc = n * nhoods
    n_pad = (n_desc + 3) // 4 * 4
    q = query('contrad_swd_gather_workspace_bytes', LL(n_desc))
    assert q > 0

    def run():
        bank, cb = TW._guarded((148, n_pad))
        stats, cs = TW._guarded((6,), torch.float64)
        ops.swd_gather(dev_level, cx, cy, nhoods, bank=bank, stats=stats)

        def intact():
            cb(); cs()
            return True
        return Run([bank, stats], [intact])

    def verify(run_):
        bank, stats = run_.outs[0].cpu().numpy(), run_.outs[1].cpu().numpy()
        want = RW.descriptors(level, pos, nhoods)
        assert np.array_equal(bank[:147, :n_desc].view(np.uint32), np.ascontiguousarray(want.T).view(np.uint32))
        assert np.all(bank[147].view(np.uint32) == 0) and np.all(bank[:, n_desc:].view(np.uint32) == 0)
        d = want.astype(np.float64).reshape(n_desc, 3, 49)
        for c in range(3):
            v = d[:, c].ravel()
            margin('swd gather sum %dx%dx%d c%d' % (n, size, nhoods, c), abs(stats[c] - RW.fsum(v)),
                   RW.fsum_bound(n_desc * 49, RW.fsum(np.abs(v))))
            margin('swd gather sumsq %dx%dx%d c%d' % (n, size, nhoods, c), abs(stats[3 + c] - RW.fsum(v * v)),
                   RW.fsum_bound(n_desc * 49, RW.fsum(v * v)))
    contract('swd gather', run, verify, [q])


@pytest.mark.parametrize('rows,n', [(5, 4097), (128, 999)])
def test_swd_absdiff_workspace_contract(rows, n, margin):
    A_, B_, off, dev = TW._absdiff_inputs(rows, n)
    o_dev = torch.from_numpy(off).cuda()
    q = query('contrad_swd_absdiff_workspace_bytes', rows, n)
    assert q > 0

    def run():
        buf = torch.full((3,), NAN, device=DEV, dtype=torch.float64)
        ops.swd_absdiff_sums(dev[0], dev[1], n, row_offset=o_dev, out=buf[1:2])
        return Run([buf[1:2]], [lambda: bool(torch.isnan(buf[0]) and torch.isnan(buf[2]))])

    def verify(run_):
        terms = RW.absdiff_terms(A_, B_, off)
        ref = RW.fsum(terms)
        margin('swd absdiff %dx%d off=True' % (rows, n), abs(float(run_.outs[0]) - ref), RW.fsum_bound(rows * n + 1, RW.fsum(terms)))
    contract('swd absdiff', run, verify, [q])


def _sums_run(fn, *args, **kw):
    """One call of a ``kid_sums``-family wrapper into a guarded float64 cell."""
    def run():
        buf = torch.full((3,), NAN, device=DEV, dtype=torch.float64)
        fn(*args, out=buf[1:2], **kw)
        return Run([buf[1:2]], [lambda: bool(torch.isnan(buf[0]) and torch.isnan(buf[2]))])
    return run


SUMS_WS_CASES = ['kid_sums', 'mmd_sums', 'dot_sums', 'gauss_sums']


@pytest.mark.parametrize('who', SUMS_WS_CASES)
def test_sums_workspace_contract(who, margin):
    """One shape each of the four wrappers over csrc/kid.hip's sum kernel.  Their parity modules already put guard bands round an
    exact-size workspace (finite fill); the NaN poison is what is new here."""
    if who in ('kid_sums', 'mmd_sums'):
        M, n, self0 = shape = (257, 1025, 5)
        S_ = TKK._sum_inputs(shape)['random'][0]
        view = TKK._device_S(S_, 3)
        if who == 'kid_sums':
            run = _sums_run(ops.kid_sums, view, n, self0=self0, gamma=0.5, coef0=2.0)
            ref, bound = RK.block_sum(S_, self0, 0.5, 2.0), RK.block_bound(S_, self0, 0.5, 2.0)
        else:
            run = _sums_run(ops.mmd_sums, view, n, 'rq', self0=self0)
            ref, bound = TKK._sum_inputs(shape)['random'][1:]
    elif who == 'dot_sums':
        M, n = 65, 300
        A_, B_, ref, bound = TF._dot_inputs((M, n))['randn'][:4]
        run = _sums_run(ops.dot_sums, TF._device_operand(A_, 3, 0)[1], TF._device_operand(B_, 0, 0)[1], n)
    else:
        shape = (65, 300, 300, 3)
        M, n, ld, self0 = shape
        S_, ref, bound = TCS._sum_inputs(shape)[('random', 2.0)]
        run = _sums_run(ops.gauss_sums, TCS._device_S(S_, ld, 0), n, 2.0, self0=self0)
    q = query('contrad_kid_sums_workspace_bytes', M, n)
    assert q >= 8

    def verify(r):
        got = float(r.outs[0])
        print('%s workspace contract: device %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (who, got, ref, abs(got - ref), bound))
        margin('%s workspace contract' % who, abs(got - ref), bound)
    contract(who, run, verify, [q])


# ======================================================================================================================
# the case tables (tests/test_ws_guard_cpu.py maps every *_workspace_bytes prototype of the header to ids listed here)
# ======================================================================================================================
def _ids(prefix, cases, fn):
    return ['%s/%s' % (prefix, fn(c)) for c in cases]


CASE_TABLES = {
    'conv': _ids('conv', TC.PATH_CASES, TC.case_id),
    'conv forced': _ids('conv forced', [c for c in TC.PATH_CASES if c[0] >= 7 and (c[1] < 2 or c[0] in (7, 8))], TC.case_id),
    'ntxent': _ids('ntxent', CONTRAST_WS_CASES, CONTRAST_ID),
    'colstats': _ids('colstats', TD.COLSTATS_CASES, COLSTATS_ID),
    'bn stats': _ids('bn stats', BN_WS_CASES, lambda c: 'M%d-K%d' % c[:2]),
    'rgb wgrad': _ids('rgb wgrad', TD.RGB_FWD_CASES, RGB_ID),
    'simclr fwd': _ids('simclr fwd', SIMCLR_FWD_CASES, AUG_ID),
    'simclr bwd': _ids('simclr bwd', SIMCLR_BWD_CASES, AUG_ID),
    'diffaug': ['diffaug/5x64x64', 'diffaug/5x32x32'],
    'sumsq': ['sumsq/n1', 'sumsq/n4095', 'sumsq/n%d' % (4096 * 1024 + 3)],
    'nhwc_dot': _ids('nhwc_dot', TS.DOT_CASES, DOT_ID),
    'gp_penalty': ['gp_penalty/6x3x32x32', 'gp_penalty/3x3x66x66'],
    'linhead': _ids('linhead', LINHEAD_WS_CASES, LINHEAD_ID),
    'knn_select': ['knn_select/5x300x200x10'],
    'swd gather': ['swd gather/3x16x5', 'swd gather/2x64x300'],
    'swd absdiff': ['swd absdiff/5x4097', 'swd absdiff/128x999'],
    'sums': ['sums/%s' % w for w in SUMS_WS_CASES],
}


def test_zz_request_counts():
    """(Runs last in this module.)  The workspace requests logged under the harness per family, for DESIGN.md section 4."""
    for fam, cnt in sorted(REQUESTS.items()):
        print('workspace requests under the harness: %-14s %d' % (fam, cnt))
    print('workspace requests under the harness: %-14s %d' % ('total', sum(REQUESTS.values())))
