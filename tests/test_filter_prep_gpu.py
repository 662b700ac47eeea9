"""Transformed Winograd filters made once per weight prep (contrad_conv2d_filter_prep + the *_u conv entry points) against
the per-call transform: U and the conv outputs bitwise equal for every Winograd family and mode the three workloads plan,
the fall-back when the plan of the call is not the one the filter was made for, and freshness of the prepared filters over
optimizer steps of D and weight changes of G, eager and captured."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from contrad_amd import ops
from contrad_amd._lib import FilterBatch, FilterJob, lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (N, H, C, K, k, stride, pad): the six trunk layers of SNDCGAN's D at the headline batch (3N = 1536) and at a per-rank batch
# of 64 (3N = 192), G's three transposed convs (data-gradient calls) at N = 512, and StyleGAN2 shapes that plan the families
# the SNDCGAN step does not (F(4x4,3x3) with 64-wide blocks on big maps, the strided 3x3 layer).
_TRUNK = [(32, 64, 128, 4, 2, 1), (16, 128, 128, 3, 1, 1), (16, 128, 256, 4, 2, 1), (8, 256, 256, 3, 1, 1),
          (8, 256, 512, 4, 2, 1), (4, 512, 512, 3, 1, 1)]
_SHAPES = [(n,) + s for n in (1536, 192) for s in _TRUNK] + \
          [(512, 8, 256, 512, 4, 2, 1), (512, 16, 128, 256, 4, 2, 1), (512, 32, 64, 128, 4, 2, 1)] + \
          [(4, 64, 32, 512, 3, 1, 1), (4, 64, 32, 256, 3, 1, 1), (4, 64, 512, 64, 3, 1, 1), (4, 129, 32, 512, 3, 2, 0)]
_KIND_NAME = {7: 'wino', 8: 'wino22', 9: 'wino44', 10: 'wino23'}


def _cases():
    out = []
    for shp in _SHAPES:
        for mode in (0, 1):
            out.append(pytest.param(shp, mode, id='%s-m%d' % ('x'.join(map(str, shp)), mode)))
    return out


def _desc(shp):
    N, H, C, K, k, s, p = shp
    return ops.make_desc(N, H, H, C, K, k, k, s, p, C, K, K)


def _run(shp, mode, filters, seed=0):
    """conv2d_fwd (mode 0) / conv2d_dgrad (mode 1) on the planned path; returns (out, wp, x)."""
    N, H, C, K, k, s, p = shp
    g = torch.Generator().manual_seed(seed)
    Ho = ops.out_size(H, k, s, p)
    wp = (torch.randn(k * k * C, K, generator=g) * 0.05).to(DEV)
    if mode == 0:
        x = torch.randn(N, H, H, C, generator=g).to(DEV)
        bias = torch.randn(K, generator=g).to(DEV)
        return lambda f: ops.conv2d_fwd(x, wp, bias, K, k, k, s, p, 0.1, 1.0, filters=f), wp
    gy = torch.randn(N, Ho, Ho, K, generator=g).to(DEV)
    ref = torch.randn(N, H, H, C, generator=g).to(DEV)
    return lambda f: ops.conv2d_dgrad(gy, wp, (N, H, H, C), k, k, s, p, act_ref=ref, slope=0.1, gain=1.0, filters=f), wp


@pytest.mark.parametrize('shp,mode', _cases())
def test_prepared_filter_equals_per_call(shp, mode):
    d = _desc(shp)
    kind, nbytes = ops.filter_kind(d, mode)
    path = lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode)
    call, wp = _run(shp, mode, None)
    scratch = {}
    with ops.private_workspace(scratch):
        y_ref = call(None).clone()
        torch.cuda.synchronize()
        ws = next(iter(scratch.values())) if scratch else None
        u_ref = ws[:nbytes // 4].clone() if kind else None      # the per-call transform wrote U at the head of the scratch
    pf = ops.filter_prep([(mode, d, wp)], torch.device(DEV))
    if kind == 0:
        assert pf.get(mode, wp) is None and path not in (7, 8, 9, 10, 11)
        assert torch.equal(call(pf), y_ref)
        return
    job = pf.get(mode, wp)
    assert job is not None and job.kind == kind
    u_new = pf.buf[:nbytes // 4]
    assert torch.equal(u_new, u_ref), 'U differs: %s mode %d' % (_KIND_NAME[kind], mode)
    scratch2 = {}
    with ops.private_workspace(scratch2):
        y_new = call(pf)
        torch.cuda.synchronize()
        ws2 = next(iter(scratch2.values()))
        ws2.fill_(float('nan'))          # the prepared call must not depend on what the scratch holds
        y_new2 = call(pf)
    assert torch.equal(y_new, y_ref) and torch.equal(y_new2, y_ref)


def test_the_cases_cover_every_planned_family():
    """The shape list reaches every Winograd family and mode the workloads plan: (filter kind, path, mode)."""
    seen = set()
    for shp in _SHAPES:
        for mode in (0, 1):
            d = _desc(shp)
            seen.add((ops.filter_kind(d, mode)[0], lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode), mode))
    want = {(8, 8, 0), (8, 8, 1), (9, 9, 0), (9, 9, 1), (9, 11, 0), (9, 11, 1), (7, 7, 0), (7, 7, 1), (10, 10, 0)}
    assert want <= seen, want - seen


@pytest.mark.parametrize('mode', [0, 1])
def test_filter_for_another_plan_falls_back(mode):
    """A U made at the headline batch handed to calls whose plan is a direct kernel (small N) or whose channels are odd:
    the call transforms per call / runs the direct kernel as without it, and matches."""
    for shp in [(2, 16, 128, 128, 3, 1, 1), (192, 8, 256, 256, 3, 1, 1)]:      # direct kernel; F(2x2,3x3) instead of F(4x4,3x3)
        call, wp = _run(shp, mode, None)
        y_ref = call(None).clone()
        src = ops.filter_prep([(mode, ops.make_desc(1536, shp[1], shp[1], shp[2], shp[3], 3, 3, 1, 1, shp[2], shp[3], shp[3]), wp)],
                              torch.device(DEV))
        job = src.get(mode, wp)
        assert job is not None and job.kind == 9
        assert ops.filter_kind(_desc(shp), mode)[0] != 9
        assert torch.equal(call(src), y_ref)
    # odd channels: no Winograd family takes 100 -> 72 channels; a job (of another layer) with the same wp pointer is ignored
    shp = (64, 16, 100, 72, 3, 1, 1)
    call, wp = _run(shp, mode, None)
    y_ref = call(None).clone()
    fake = ops.PreparedFilters()
    u = torch.zeros(36 * 128 * 128, device=DEV)
    fake.buf = u
    fake.jobs[(mode, wp.data_ptr())] = FilterJob(wp.data_ptr(), u.data_ptr(), 9, mode, 128, 128, 128)
    assert torch.equal(call(fake), y_ref)


def test_filter_prep_argument_errors():
    b = FilterBatch()
    b.n = 1
    u = torch.zeros(1024, device=DEV)
    b.jobs[0] = FilterJob(u.data_ptr(), u.data_ptr(), 5, 0, 64, 64, 64)       # unknown kind
    assert lib().raw('contrad_conv2d_filter_prep')(ctypes.byref(b), None) == -22
    b.jobs[0] = FilterJob(u.data_ptr(), u.data_ptr(), 10, 1, 64, 64, 64)      # the strided 3x3 family is forward only
    assert lib().raw('contrad_conv2d_filter_prep')(ctypes.byref(b), None) == -22
    b.n = 17
    assert lib().raw('contrad_conv2d_filter_prep')(ctypes.byref(b), None) == -22


# ---------------------------------------------------------------------------------------------------------------------
# freshness: the prepared filters follow the weights
# ---------------------------------------------------------------------------------------------------------------------
def _setup(N):
    from contrad_amd import config
    from contrad_amd.augment import get_augment
    from contrad_amd.engine import set_grad
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.optim import FusedAdam
    from contrad_amd.training.gan import setup
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'gan', 'cifar10', 'c10_b64.gin')])
    torch.manual_seed(0); np.random.seed(0)
    G, D = get_architecture('sndcgan', (32, 32, 3))
    G, D = G.to(DEV).train(), D.to(DEV).train()
    P = setup(argparse.Namespace(mode='contrad', aug='simclr', temp=0.1, lbd_a=1.0, distributed=False))
    P.augment_fn = get_augment(mode='simclr').to(DEV)
    opt = FusedAdam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    set_grad(G, False); set_grad(D, True)
    x = torch.rand(N, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    return P, G, D, opt, x


def _perturb_g(G, step):
    """A generator update between two D-steps: through the version counter (in-place op) and, the second time, a raw
    write followed by invalidate_cache()."""
    with torch.no_grad():
        if step == 0:
            for j in range(3):
                G.main[3 * j].weight.mul_(1.05)
        else:
            for j in range(3):
                w = G.main[3 * j].weight
                ops.axpby_(w.data, w.data, 0.9, 0.0)
            G.invalidate_cache()


def _steps(N, graphed, prep, touch_g, K=3):
    from contrad_amd.engine import GraphedDStep, d_step
    old = ops.FILTER_PREP
    ops.FILTER_PREP = prep
    try:
        P, G, D, opt, x = _setup(N)
        torch.manual_seed(7); np.random.seed(7)
        step = GraphedDStep(P, G, D, opt, {'loss': 'nonsat'}, x, warmup=1) if graphed else \
            (lambda: d_step(P, G, D, opt, {'loss': 'nonsat'}, x))
        out = []
        for i in range(K):
            dl, aux = step()
            out.append((dl.item(), aux['penalty'].item(), [p.detach().clone() for p in D.parameters()]))
            if touch_g and i < 2:
                _perturb_g(G, i)
        return out
    finally:
        ops.FILTER_PREP = old


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('N,touch_g', [(64, False), (512, True)], ids=['b64', 'b512-G-changes'])
def test_prepared_filters_follow_the_weights(N, graphed, touch_g):
    """D-steps with Adam between them (and G's weights changed between them, N = 512: the batch at which G's transposed
    convs plan Winograd): losses and every parameter equal the per-call path step for step."""
    new = _steps(N, graphed, True, touch_g)
    ref = _steps(N, graphed, False, touch_g)
    for i, ((l1, g1, p1), (l0, g0, p0)) in enumerate(zip(new, ref)):
        assert (l1, g1) == (l0, g0), (i, l1, l0, g1, g0)
        for a, b in zip(p1, p0):
            assert torch.equal(a, b), i
    assert new[0][0] != new[1][0]          # the steps did move
