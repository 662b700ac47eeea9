"""GPU parity of the two Winograd weight-gradient kernels at the smallest shapes that reach every case of their staging
(csrc/wino22.h, csrc/wino.h: raw boxes whose pieces wrap, one or two phases per row block, ragged image groups, one or
several splits of the tile axis, an odd number of chunks per split, several row and K blocks), against float64
(tests/conv_ref64.py).

Every case calls ops.conv2d_wino_wgrad (the forced entry point) with dbias.  x and gy are channel slices of wider buffers
whose spare columns hold 1e3; dwp and dbias are slices of NaN-filled buffers with a spare row / spare floats either side
and spare columns past K: every sentinel must stay NaN.  The bounds are test_conv_paths_gpu.FAMILY_TOL of paths 8 (4x4
stride 2) and 7 (3x3), and the same call must give the same bits twice.
"""
import pytest
import torch

import conv_ref64 as R
from contrad_amd import ops
from test_conv_paths_gpu import FAMILY_TOL, _input, check      # noqa: F401  (FAMILY_TOL: the bounds `check` applies)

pytestmark = pytest.mark.gpu

# (family, N, H, C, K, k, stride, what)        chunk = 8 tiles of 2x2 gy pixels; splits fill the chip once at most
CASES = [
    (8, 5, 8, 64, 64, 4, 2, 'C = 64: two phases per row block; 2 images per chunk, 5 images: a ragged group; 1 chunk per split'),
    (8, 3, 32, 128, 64, 4, 2, '16 x 16 gy map: 5 x 9 boxes (raw pieces wrap), one phase per row block'),
    (8, 16, 16, 256, 128, 4, 2, '8 row blocks x 2 K blocks, 16 splits of 2 chunks'),
    (8, 23, 16, 256, 128, 4, 2, '46 chunks in splits of 3: an odd chunk count, the last split has 1'),
    (7, 5, 4, 64, 64, 3, 1, '4 x 4 maps: 2 images per chunk, a ragged group'),
    (7, 3, 16, 128, 64, 3, 1, '16 x 16 maps: boxes with a halo on every side'),
    (7, 7, 8, 256, 128, 3, 1, '4 C blocks x 2 K blocks, 14 splits'),
]


def case_id(case):
    P, N, H, C, K, k, s, _ = case
    return 'p%d-%dx%dx%dx%d-%d-k%ds%d' % (P, N, H, H, C, K, k, s)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_wino_wgrad_staging_matches_float64(case, margin):
    P, N, H, C, K, k, s, _ = case
    assert P in FAMILY_TOL
    dev = torch.device('cuda')
    Ho = H // s
    g = torch.Generator().manual_seed(4200 + CASES.index(case))
    x = _input(N, H, H, C, C + 4, g, dev)
    gy = _input(N, Ho, Ho, K, K + 4, g, dev)
    refw, refb = R.wgrad(x, gy, k, k, s, 1)
    refw = refw.permute(2, 3, 1, 0).reshape(k * k * C, K)         # packed layout
    ldw = K + 4
    runs = []
    for _ in range(2):
        dwb = torch.full((k * k * C + 2, ldw), float('nan'), device=dev)
        dbb = torch.full((K + 8,), float('nan'), device=dev)
        ops.conv2d_wino_wgrad(x, gy, out=dwb[1:-1], dbias=dbb[4:4 + K])
        torch.cuda.synchronize()
        inner = torch.zeros_like(dwb, dtype=torch.bool)
        inner[1:-1, :K] = True
        assert torch.isnan(dwb[~inner]).all(), 'weight gradient wrote outside dwp[:, :K]'
        assert torch.isnan(dbb[:4]).all() and torch.isnan(dbb[4 + K:]).all(), 'dbias written out of range'
        runs.append((dwb[1:-1, :K].clone(), dbb[4:4 + K].clone()))
    check(margin, P, 'wgrad', runs[0][0], refw)
    check(margin, P, 'dbias', runs[0][1], refb)
    assert torch.equal(runs[0][0], runs[1][0]), 'the weight gradient differs between two identical calls'
    assert torch.equal(runs[0][1], runs[1][1]), 'the bias gradient differs between two identical calls'
