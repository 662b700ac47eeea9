"""GPU parity of every tile, split and block-order form of the direct conv kernels (paths 0 - 3: csrc/igemm.hip, igemm_lean.h)
against float64 -- the matrix of tests/test_conv_paths_gpu.py one level down.  That module has one case per (path, mode, split)
triple; one triple is up to five kernel templates and several block-to-tile decodes.  tests/igemm_forms.py lists one case per
sub-form (path, mode, bm, bn, split, tile-order table, data-gradient stride), each at the smallest shape on which the form still
has a ragged last M-tile, a ragged last N-tile and, where it splits, a ragged last split; tests/test_conv_plan_cpu.py proves
without a GPU that the table reaches every sub-form the shipped planner returns.

The machinery is that of test_conv_paths_gpu.py, imported: conv_ref64 as the reference, NaN-filled guard buffers with a spare
image either side and a leading dimension above the channel count, inputs in channel slices whose spare columns hold 1e3,
every epilogue term on and once none.  Added here:
  * a case asserts its form from the public plan queries BEFORE it runs (path, tile, workspace bytes, tile-order table, grid
    blocks); a case whose declared form is not what the library reports fails;
  * the larger tiles are planned for large batches only, so most cases force tile and split count with
    contrad_dev_plan_override of the development library -- always a plan the planner emits at some shape (splits of >= 8
    K-tiles with >= 32 in all, no 128-wide N-tile on <= 64 columns);
  * every split form runs twice and must give bitwise the same result (the reduce kernels sum in a fixed order).
The development switches are read once per process: one parent test per environment group (igemm_forms.GROUPS) starts one
child pytest on the development library, children strictly one after another; the cases themselves are skipped outside their
group's child, so a plain `-m gpu` run executes each exactly once.

Bounds: the 1e-3 contract, and the tight per-family bound of test_conv_paths_gpu.FAMILY_TOL (max-norm, rel-L2: about 5x the
worst that module observes).  Those bounds were measured at nominal contraction depths of up to 81 (path 1), 576 (path 2) and 288 (path
3) products per output, so the unsplit cases here stay at or below those depths; a split case is deeper, each of its slabs is
not.  No form needed a bound of its own.  Worst observed on an MI355X over this module, per family and form:
    path  form                                        cases   max-norm  rel-L2     bound of the family
    0     strided data gradient                           1    7.8e-08  6.7e-08    1e-6    5e-7
    1     forward, four tiles                             4    3.5e-07  1.5e-07    1e-6    7e-7
    1     data gradient, four tiles                       4    3.2e-07  1.5e-07
    1     strided data gradient, four tiles               4    2.4e-07  8.7e-08
    1     weight gradient, one slab / several         4 + 4    3.4e-07  1.4e-07
    2     forward, unsplit / split                    4 + 5    8.2e-07  3.6e-07    3e-6    1.5e-6
    2     data gradient, unsplit / split              4 + 5    8.0e-07  3.5e-07
    2     strided data gradient, class groups            14    1.0e-06  4.2e-07
    2     strided data gradient, balanced order           8    1.2e-06  3.6e-07
    2     weight gradient, one slab / several         5 + 5    2.7e-07  1.5e-07
    3     pixel-major, per-block table (fwd / dgrad)  4 + 4    7.4e-07  2.7e-07    1.5e-6  6e-7
    3     pixel-major, whole-launch table             5 + 5    6.8e-07  2.7e-07
    3     strided data gradient, class-major table        5    7.9e-07  2.7e-07
    3     border classes (fwd / dgrad)                6 + 4    6.3e-07  2.7e-07
    3     weight gradient on pixel-major positions    2 + 3    3.2e-07  1.5e-07
Within a family the tiles of one shape agree to a few per cent in rel-L2 (e.g. the four lean split forwards: 3.06e-7 .. 3.14e-7);
the spread in max-norm is that of one element.  The per-case figures go to the margins file through the `margin` fixture, one
line per case id.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

import conv_ref64 as R
import igemm_forms as IF
import test_conv_paths_gpu as P
from contrad_amd import ops
from contrad_amd._lib import lib

pytestmark = pytest.mark.gpu

GROUP = os.environ.get(IF.CHILD_ENV)            # set in a child process only: the group whose cases run here
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FATAL = (124, 134, 137, 139)                   # time limit, abort, kill, segmentation fault


def check(margin, case, what, out, ref):
    emax, el2 = R.errors(out, ref)
    print('%s %s: max-norm %.3e rel-L2 %.3e' % (case.id, what, emax, el2))
    assert emax < P.CONTRACT, (case.id, what, emax)
    tmax, tl2 = P.FAMILY_TOL[case.path]
    margin('conv form %s  max-norm' % case.id, emax, tmax)
    margin('conv form %s  rel-L2' % case.id, el2, tl2)


def _run(case, margin):
    N, H, W, C, K, k, s, p = case.shape
    mode, dev = case.mode, torch.device('cuda')
    ldx, ldy, ldw = case.lds
    pc = (case.path, mode, case.split) + case.shape + (1, 1, 1, case.what)          # (a PATH_CASES row: same leading dimensions)
    assert P.case_lds(pc) == case.lds
    d = case.desc()
    Ho, Wo = d.Ho, d.Wo
    g = torch.Generator().manual_seed(5000 + IF.FORM_CASES.index(case))
    w, wp = P._weights(pc, g, dev)
    runs = 2 if case.split else 1                  # (a split form twice: fixed summation order)
    if mode == 0:
        x = P._input(N, H, W, C, ldx, g, dev)
        bias = P._rand((K,), g, dev, 0.3)
        add = P._input(N, Ho, Wo, K, ldy, g, dev)
        for epi in (True, False):
            kw = dict(slope=P.SLOPE, gain=P.GAIN, addend=add) if epi else {}
            ref = R.fwd(x, w, bias if epi else None, s, p, **kw)
            ys = []
            for _ in range(runs):
                y = P.Guarded(N, Ho, Wo, K, ldy, float('nan'), dev)
                ops.conv2d_fwd(x, wp, bias if epi else None, K, k, k, s, p, out=y.t, **kw)
                torch.cuda.synchronize()
                assert y.sentinels_intact(), 'forward wrote outside y'
                check(margin, case, 'fwd', y.t, ref)
                ys.append(y.t)
            assert torch.equal(ys[0], ys[-1]), 'a repeated split-K forward differs'
    elif mode == 1:
        gy = P._input(N, Ho, Wo, K, ldy, g, dev)
        act = P._input(N, H, W, C, ldx, g, dev)
        for epi in (True, False):
            kw = dict(act_ref=act, slope=P.SLOPE, gain=P.GAIN) if epi else {}
            ref = R.dgrad(gy, w, (H, W), s, p, **kw)
            dxs = []
            for _ in range(runs):
                dx = P.Guarded(N, H, W, C, ldx, float('nan'), dev)
                ops.conv2d_dgrad(gy, wp, (N, H, W, C), k, k, s, p, out=dx.t, **kw)
                torch.cuda.synchronize()
                assert dx.sentinels_intact(), 'data gradient wrote outside dx'
                check(margin, case, 'dgrad', dx.t, ref)
                dxs.append(dx.t)
            assert torch.equal(dxs[0], dxs[-1]), 'a repeated split-K data gradient differs'
    else:
        x = P._input(N, H, W, C, ldx, g, dev)
        gy = P._input(N, Ho, Wo, K, ldy, g, dev)
        refw, refb = R.wgrad(x, gy, k, k, s, p)
        refw = refw.permute(2, 3, 1, 0).reshape(k * k * C, K)         # packed layout
        for with_bias in (True, False):
            outs = []
            for _ in range(runs):
                dwb = torch.full((k * k * C + 2, ldw), float('nan'), device=dev)
                dbb = torch.full((K + 8,), float('nan'), device=dev)
                dwp, dbias = dwb[1:-1], (dbb[4:4 + K] if with_bias else None)
                ops.conv2d_wgrad(x, gy, k, k, s, p, out=dwp, dbias=dbias)
                torch.cuda.synchronize()
                inner = torch.zeros_like(dwb, dtype=torch.bool)
                inner[1:-1, :K] = True
                assert torch.isnan(dwb[~inner]).all(), 'weight gradient wrote outside dwp[:, :K]'
                check(margin, case, 'wgrad', dwp[:, :K], refw)
                if with_bias:
                    assert torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all(), 'dbias written out of range'
                    check(margin, case, 'dbias', dbias, refb)
                outs.append((dwp[:, :K], dbias))
            assert torch.equal(outs[0][0], outs[-1][0]), 'a repeated weight gradient over several slabs differs'
            if with_bias:
                assert torch.equal(outs[0][1], outs[-1][1])


@pytest.mark.parametrize('case', IF.FORM_CASES, ids=lambda c: c.id)
def test_form_matches_float64(case, margin):
    if GROUP != case.group:
        pytest.skip('runs in the child process of group %r (test_group_in_a_fresh_process)' % case.group)
    for name, value in IF.GROUPS[case.group].items():
        assert os.environ.get(name) == value
    L = lib()
    IF.set_override(L, case.ov)
    try:
        r = IF.report(L, case.desc(), case.mode)
        assert r is not None and r['path'] < 4
        assert not IF.mismatch(case, r), IF.mismatch(case, r)
        _run(case, margin)
    finally:
        IF.set_override(L, None)


@pytest.mark.parametrize('group', sorted(IF.GROUPS))
def test_group_in_a_fresh_process(group):
    """One child pytest per environment group, on the development library: every case of the group passes, none is skipped."""
    if GROUP:
        pytest.skip('a child process starts no children')
    from contrad_amd import build
    assert os.path.exists(build.DEV_LIB), 'run __graft_entry__.build() first'
    n = sum(c.group == group for c in IF.FORM_CASES)
    env = dict(os.environ)
    for name in IF.SWITCHES:
        env.pop(name, None)
    env.update(IF.GROUPS[group])
    env.update({'CONTRAD_HIP_LIB': build.DEV_LIB, IF.CHILD_ENV: group})
    cmd = [sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-s', '-m', 'gpu', '-x', '-k', 'form_%s_' % group]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=60 + 2 * n, cwd=_ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit('the child of group %r ran into its time limit: nothing more is started on the GPU\n%s'
                    % (group, (e.stdout or b'')[-2000:]), returncode=3)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    if r.returncode in _FATAL or r.returncode < 0:
        pytest.exit('the child of group %r ended with status %d: nothing more is started on the GPU\n%s'
                    % (group, r.returncode, tail), returncode=3)
    assert r.returncode == 0, tail
    assert re.search(r'\b%d passed' % n, r.stdout), tail
