"""GPU parity of the persistent item walk of the Winograd forward / data-gradient kernels (csrc/wino.h, wino44.h, wino44n.h,
wino22.h, wino23.h) against float64, on launches whose blocks walk two and three items (tests/wino_walks.py: the case table
and a restatement of the walk; tests/test_wino_walks_cpu.py proves without a GPU which walk forms the table reaches).

Every case follows the protocol of tests/test_conv_paths_gpu.py -- the calls the models make (ops.conv2d_fwd with bias, slope
0.2, gain sqrt2 and an addend; ops.conv2d_dgrad with act_ref) and once no epilogue at all, the path query asserted first,
operands as channel slices of wider buffers, 1e3 around the inputs, a NaN image before and after every output, whole tensors
against the im2col float64 reference, the 1e-3 contract and that module's FAMILY_TOL (imported, unchanged) -- and adds, all
BITWISE:
  * a repeat of the call, and the forced entry point of the family the path query names;
  * place-in-walk independence: the same call on the images with the whole image groups in reverse order (the ragged group
    stays last) gives, un-permuted, the same bits -- every tile block then sits in another XCD list, slot and walk position;
  * one item per block: the same images through the forced entry point in launches of whole image groups, each so small that
    every block walks ONE item, give the same bits as the full launch.

Items, items per block (walk lengths over the 256 blocks) and the worst error of the two epilogue runs on an MI355X:

  case                                  items   blocks x items walked    max-norm   rel-L2
  p7-m0-2987x4x4x16-192-k3s1p1           561    207 x 2, 49 x 3         2.3e-07    1.7e-07
  p7-m0-747x8x8x16-192-k3s1p1            561    207 x 2, 49 x 3         2.4e-07    1.6e-07
  p7-m0-187x16x16x16-192-k3s1p1          561    207 x 2, 49 x 3         2.1e-07    1.6e-07
  p7-m0-47x32x32x16-192-k3s1p1           564    204 x 2, 52 x 3         2.1e-07    1.6e-07
  p7-m1-2987x4x4x192-16-k3s1p1           561    207 x 2, 49 x 3         2.5e-07    1.7e-07
  p7-m1-747x8x8x192-16-k3s1p1            561    207 x 2, 49 x 3         2.6e-07    1.7e-07
  p9-m0-1493x8x8x32-192-k3s1p1           561    207 x 2, 49 x 3         7.1e-06    1.4e-06
  p9-m0-373x16x16x32-192-k3s1p1          561    207 x 2, 49 x 3         7.0e-06    1.3e-06
  p9-m0-94x32x32x32-192-k3s1p1           564    204 x 2, 52 x 3         7.7e-06    1.3e-06
  p9-m1-1493x8x8x192-32-k3s1p1           561    207 x 2, 49 x 3         6.1e-06    1.4e-06
  p9-m1-373x16x16x192-32-k3s1p1          561    207 x 2, 49 x 3         6.6e-06    1.3e-06
  p11-m0-5977x4x4x32-96-k3s1p1           561    207 x 2, 49 x 3         6.4e-06    1.5e-06
  p11-m0-1493x8x8x32-96-k3s1p1           561    207 x 2, 49 x 3         6.0e-06    1.4e-06
  p11-m0-373x16x16x32-96-k3s1p1          561    207 x 2, 49 x 3         6.2e-06    1.3e-06
  p11-m0-94x32x32x32-96-k3s1p1           564    204 x 2, 52 x 3         6.4e-06    1.3e-06
  p11-m1-5977x4x4x96-32-k3s1p1           561    207 x 2, 49 x 3         7.4e-06    1.5e-06
  p11-m1-373x16x16x96-32-k3s1p1          561    207 x 2, 49 x 3         5.9e-06    1.3e-06
  p8-m0-6583x8x8x8-192-k4s2p1            618    150 x 2, 106 x 3        4.9e-07    2.3e-07
  p8-m0-1645x16x16x8-192-k4s2p1          618    150 x 2, 106 x 3        5.0e-07    2.3e-07
  p8-m0-411x32x32x8-192-k4s2p1           618    150 x 2, 106 x 3        4.5e-07    2.2e-07
  p8-m1-1655x8x8x192-16-k4s2p1           624    144 x 2, 112 x 3        3.3e-07    1.8e-07
  p8-m1-413x16x16x192-16-k4s2p1          624    144 x 2, 112 x 3        4.2e-07    1.7e-07
  p8-m1-103x32x32x192-16-k4s2p1          624    144 x 2, 112 x 3        3.8e-07    1.7e-07
  p10-m0-5977x9x9x16-192-k3s2p0          561    207 x 2, 49 x 3         7.8e-07    2.9e-07
  p10-m0-1493x17x17x16-192-k3s2p0        561    207 x 2, 49 x 3         7.6e-07    2.9e-07
  p10-m0-373x33x33x16-192-k3s2p0         561    207 x 2, 49 x 3         7.4e-07    2.9e-07
  p10-m0-94x65x65x16-192-k3s2p0          564    204 x 2, 52 x 3         6.6e-07    2.9e-07
  p9-m0-383x16x16x32-128-k3s1p1          384    128 x 1, 128 x 2        5.3e-06    1.3e-06
  p7-m0-383x16x16x16-128-k3s1p1          766    2 x 2, 254 x 3          2.2e-07    1.6e-07
"""
import ctypes

import pytest
import torch

import conv_ref64 as R
import test_conv_paths_gpu as M
import wino_walks as WW
from contrad_amd import ops
from contrad_amd._lib import lib

pytestmark = pytest.mark.gpu


def _path_case(case):
    """The case in the layout of test_conv_paths_gpu.PATH_CASES (every leading dimension 4 floats past the channel count)."""
    P, mode, N, H, W, C, K, k, s, p, what = case
    return (P, mode, False, N, H, W, C, K, k, s, p, 1, 1, 1, what)


def _sliced(data, ld, dev):
    """``data`` (N,H,W,C) as the channel slice of a 1e3-filled buffer with a spare image either side."""
    N, H, W, C = data.shape
    t = M.Guarded(N, H, W, C, ld, 1e3, dev)
    t.t.copy_(data)
    return t.t


def _check(margin, case, out, ref):
    emax, el2 = R.errors(out, ref)
    print('%s  max-norm %.2e  rel-L2 %.2e' % (WW.case_id(case), emax, el2))
    assert emax < M.CONTRACT, (WW.case_id(case), emax)
    tmax, tl2 = M.FAMILY_TOL[case[0]]
    margin('wino walk %-34s max-norm' % WW.case_id(case), emax, tmax)
    margin('wino walk %-34s rel-L2' % WW.case_id(case), el2, tl2)


@pytest.mark.parametrize('case', WW.WALK_CASES, ids=WW.case_id)
def test_wino_walk_matches_float64_wherever_an_item_sits(case, margin):
    P, mode, N, H, W, C, K, k, s, p = case[:10]
    dev = torch.device('cuda')
    pc = _path_case(case)
    ldx, ldy, ldw = M.case_lds(pc)
    assert (ldx, ldy, ldw) == WW.lds(case)
    d = M.case_desc(pc)
    assert lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode) == P
    geo = WW.geometry(case)
    assert lib().raw('contrad_conv2d_grid_blocks')(ctypes.byref(d), mode, 1) == WW.grid(geo.NP, geo.NSUB) == 256
    Ho, Wo = d.Ho, d.Wo
    g = torch.Generator().manual_seed(3000 + WW.WALK_CASES.index(case))
    w, wp = M._weights(pc, g, dev)
    order = torch.tensor(WW.group_permutation(case), device=dev)
    cuts = WW.sub_launches(case)
    if mode == 0:
        inp = M._input(N, H, W, C, ldx, g, dev)                        # x
        side = M._input(N, Ho, Wo, K, ldy, g, dev)                     # the addend
        bias = M._rand((K,), g, dev, 0.3)
        oshape, ldo = (N, Ho, Wo, K), ldy
    else:
        inp = M._input(N, Ho, Wo, K, ldy, g, dev)                      # gy
        side = M._input(N, H, W, C, ldx, g, dev)                       # act_ref
        bias = None
        oshape, ldo = (N, H, W, C), ldx
    inp_p, side_p = _sliced(inp[order], inp.stride(2), dev), _sliced(side[order], side.stride(2), dev)

    def planned(i, r, out, epi):
        if mode == 0:
            kw = dict(slope=M.SLOPE, gain=M.GAIN, addend=r) if epi else {}
            ops.conv2d_fwd(i, wp, bias if epi else None, K, k, k, s, p, out=out, **kw)
        else:
            kw = dict(act_ref=r, slope=M.SLOPE, gain=M.GAIN) if epi else {}
            ops.conv2d_dgrad(i, wp, (i.shape[0], H, W, C), k, k, s, p, out=out, **kw)

    def forced(i, r, out, epi):
        M._forced(P, mode, i, wp, C, K, bias if epi and mode == 0 else None, r if epi else None,
                  M.SLOPE if epi else 1.0, M.GAIN if epi else 1.0, out)

    def fresh():
        return M.Guarded(oshape[0], oshape[1], oshape[2], oshape[3], ldo, float('nan'), dev)

    for epi in (True, False):
        y = fresh()
        planned(inp, side, y.t, epi)
        torch.cuda.synchronize()
        assert y.sentinels_intact(), 'the launch wrote outside its output'
        if mode == 0:
            ref = R.fwd(inp, w, bias if epi else None, s, p, **(dict(slope=M.SLOPE, gain=M.GAIN, addend=side) if epi else {}))
        else:
            ref = R.dgrad(inp, w, (H, W), s, p, **(dict(act_ref=side, slope=M.SLOPE, gain=M.GAIN) if epi else {}))
        _check(margin, case, y.t, ref)
        del ref
        y2 = fresh()
        planned(inp, side, y2.t, epi)
        assert torch.equal(y.t, y2.t), 'a repeat of the call differs'
        y2 = fresh()
        forced(inp, side, y2.t, epi)
        assert torch.equal(y.t, y2.t), 'the planned call is not the kernel path %d names' % P
        # the image groups in reverse order: every tile block in another XCD list, slot and position of a walk
        y2 = fresh()
        planned(inp_p, side_p, y2.t, epi)
        assert y2.sentinels_intact()
        assert torch.equal(y.t[order], y2.t), 'the result of an item depends on its place in the walk'
        # one item per block
        y2 = fresh()
        for a, b in cuts:
            forced(inp[a:b], side[a:b], y2.t[a:b], epi)
        assert y2.sentinels_intact(), 'a sub-launch wrote outside its images'
        assert torch.equal(y.t, y2.t), 'a multi-item walk differs from one-item-per-block launches of the same images'
        del y, y2
