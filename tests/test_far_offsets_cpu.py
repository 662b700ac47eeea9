"""The far cases of tests/test_far_offsets_gpu.py against the host logic (no GPU), and the addressing limits of
include/contrad_hip.h from both sides.

* Every far conv case plans the (path, mode, split-K) it declares, its declared far operands span more than 2^32 bytes
  plus one image with fewer than 2^31 elements, and the period of its image patterns divides the number of images in
  neither 2^31 nor 2^32 bytes of any operand (an access that wraps by exactly that distance must land on other data).
* The far cases reach every (path, mode) pair -- and every split-K triple -- of the small parity matrix
  (tests/test_conv_paths_gpu.py: PATH_CASES).
* The element limit sits where the header says: 2^31 elements of x, of y and of the packed filter are refused by the path
  query, the workspace queries and the *_ok queries; one descriptor below is accepted.
* Each block-relative guard (the ok() of every Winograd family, the weight-gradient families, lean_ok) is taken from both
  sides of nimg * H * W * max(ldi, ldo) * 4 = 2^31: just under plans the family, just over a direct path.  The same for the
  per-image 2^31-byte rule of the branch-free FIR forms.
"""
import ctypes
import importlib.util
import os
import sys

import pytest

from contrad_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    """A test module beside this one, loaded for its tables and helpers only (touches no GPU)."""
    spec = importlib.util.spec_from_file_location('_far_cpu_' + name, os.path.join(_HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, _HERE)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(_HERE)
    return mod


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def M():
    return _load('test_far_offsets_gpu')


@pytest.fixture(scope='module')
def plan():
    return _load('test_conv_plan_cpu')


def _sides(case, d):
    """{'x': (images, bytes per image), 'y': ...} of a far conv case."""
    N, H, W, ldx, ldy = case[3], case[4], case[5], case[7], case[9]
    return {'x': (N, H * W * ldx * 4), 'y': (N, d.Ho * d.Wo * ldy * 4)}


def test_every_far_conv_case_plans_what_it_declares(L, M, plan):
    for case in M.FAR_CASES:
        d = M.far_desc(case)
        assert plan.triple(L, d, case[1]) == tuple(case[:3]), (M.far_id(case), plan.triple(L, d, case[1]))
    assert len({M.far_id(c) for c in M.FAR_CASES}) == len(M.FAR_CASES)


def test_declared_far_operands_are_far(L, M):
    for case in M.FAR_CASES:
        d = M.far_desc(case)
        for side, (n, img) in _sides(case, d).items():
            assert n * img // 4 < 2 ** 31, (M.far_id(case), side)
            if side in case[13]:
                assert n * img > 2 ** 32 + img, (M.far_id(case), side, n * img)
    assert sum(1 for c in M.FAR_CASES if c[13] == 'xy') >= len(M.FAR_CASES) - 8       # (the exceptions are named in the table)
    # the dense far operands of the other kernels
    for case in M.UF_FAR_CASES:
        cfg = M.uf_cfg(case)
        oh, ow = M.S.out_size(*cfg[1:3], *cfg[4:])
        major, minor = cfg[0], cfg[3]
        big = max(cfg[1] * cfg[2], oh * ow) * minor * 4
        assert major * big >= 2 ** 32 and major * big // 4 < 2 ** 31, case[0]
        assert ('_ptr' in case[0]) == (big >= 2 ** 31)
    assert M.FLAT_N * 4 > 2 ** 32 + M.ROW * 4 and M.FLAT_N < 2 ** 31 and (M.FLAT_N // 4) * 4 * 4 > 2 ** 32
    N, HW, C = M.NHWC_FAR
    assert N * HW * C * 4 > 2 ** 32 + HW * C * 4 and N * HW * C < 2 ** 31
    # rgb_conv_dgrad's far output: images of more than 2^32 bytes from a gy of more than 2^31 elements (no element limit there)
    N, H, W, K, C, k = M.RGB_DGRAD_FAR_OUT
    assert N * C * H * W * 4 > 2 ** 32 + C * H * W * 4 and N * C * H * W < 2 ** 31 < N * H * W * K
    assert (N * H * W * K + N * C * H * W) * 4 < 22 * 2 ** 30 and C <= 4 and K >= 16
    rows, K, ld = M.ROWS_FAR
    assert rows * ld * 4 > 2 ** 32 + ld * 4 and rows * ld < 2 ** 31


def _period_ok(images_bytes, P):
    for dist in (2 ** 31, 2 ** 32):
        if dist % images_bytes == 0 and (dist // images_bytes) % P == 0:
            return False
    return True


def test_the_pattern_period_hides_no_wrap(L, M):
    # (With P = 7 and images of a power of two of bytes this holds by itself -- 7 divides no power of two -- and an image that
    # divides neither distance cannot be hit by such a wrap at all: the assertions guard later edits of P and of the shapes.
    # An operand of no more than P images has no period: all its images differ.)
    assert M.P in (7, 13)
    for case in M.FAR_CASES:
        d = M.far_desc(case)
        for side, (n, img) in _sides(case, d).items():
            if n > M.P:
                assert _period_ok(img, M.P), (M.far_id(case), side)
    for case in M.UF_FAR_CASES:
        cfg = M.uf_cfg(case)
        oh, ow = M.S.out_size(*cfg[1:3], *cfg[4:])
        for img in (cfg[1] * cfg[2] * cfg[3] * 4, oh * ow * cfg[3] * 4):
            assert cfg[0] <= M.P or _period_ok(img, M.P), case[0]
    for (N, H, W, K, ldy, k, _) in M.RGB_FAR_CASES:
        assert _period_ok(H * W * ldy * 4, M.P) and _period_ok(3 * H * W * 4, M.P)
    N, H, W, K, C, k = M.RGB_DGRAD_FAR_OUT
    assert _period_ok(H * W * K * 4, M.P) and _period_ok(C * H * W * 4, M.P)
    # flat ops: a row of an odd length divides no power of two (their data is random over the whole tensor anyway)
    assert M.ROW % 2 == 1 and M.ROW > 1 and M.NHWC_FAR[1] % 2 == 1


def test_the_far_cases_reach_every_path_and_mode_of_the_small_matrix(L, M):
    small = _load('test_conv_paths_gpu').PATH_CASES
    far_pairs = {(c[0], c[1]) for c in M.FAR_CASES}
    far_triples = {tuple(c[:3]) for c in M.FAR_CASES}
    assert {(c[0], c[1]) for c in small} <= far_pairs, sorted({(c[0], c[1]) for c in small} - far_pairs)
    # split-K: every split triple of the small matrix has a far descriptor that plans it
    assert {tuple(c[:3]) for c in small if c[2]} <= far_triples, sorted({tuple(c[:3]) for c in small if c[2]} - far_triples)
    # the prepared-filter entry points run on a far Winograd forward and a far Winograd data gradient
    assert any(c[14] and c[1] == 0 and c[0] >= 7 for c in M.FAR_CASES)
    assert any(c[14] and c[1] == 1 and c[0] >= 7 for c in M.FAR_CASES)


def _desc(N, H, W, C, K, k, s, p, ldx=None, ldy=None, ldw=None):
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return _lib.ConvDesc(N, H, W, C, ldx or C, Ho, Wo, K, ldy or K, k, k, s, p, ldw or (K + 3) // 4 * 4)


def _queries(L, d):
    """Every plan query of a descriptor: paths of the three modes, the three workspace queries, the *_ok queries."""
    r = ctypes.byref(d)
    return ([L.raw('contrad_conv2d_path')(r, m) for m in (0, 1, 2)],
            [L.raw('contrad_conv2d_fwd_workspace_bytes')(r), L.raw('contrad_conv2d_dgrad_workspace_bytes')(r),
             L.raw('contrad_conv2d_wgrad_workspace_bytes')(r)],
            [L.raw('contrad_conv2d_wino_ok')(r, m) for m in (0, 1, 2)] + [L.raw('contrad_conv2d_wino44_ok')(r, m) for m in (0, 1)])


def _refused(L, d):
    paths, ws, oks = _queries(L, d)
    return all(v == -22 for v in paths + ws + oks)


def _accepted(L, d):
    paths, ws, oks = _queries(L, d)
    return all(v >= 0 for v in paths + ws) and all(v in (0, 1) for v in oks)


def test_the_element_limit_sits_at_two_to_the_31(L):
    """include/contrad_hip.h: each of x, y and the packed filter has fewer than 2^31 elements (leading dimensions counted)."""
    # x side: N * H * W * ldx
    assert _refused(L, _desc(2 ** 19, 1, 1, 16, 8, 1, 1, 0, ldx=4096))
    d = _desc(2 ** 19 - 1, 1, 1, 16, 8, 1, 1, 0, ldx=4096)
    assert _accepted(L, d) and _queries(L, d)[0] == [2, 1, 1]
    # y side: N * Ho * Wo * ldy
    assert _refused(L, _desc(2 ** 19, 1, 1, 8, 8, 1, 1, 0, ldy=4096))
    assert _accepted(L, _desc(2 ** 19 - 1, 1, 1, 8, 8, 1, 1, 0, ldy=4096))
    # a 3x3 layer the Winograd queries accept one image below the limit: 32768 images of 4 x 4 x 4096
    assert _refused(L, _desc(32768, 4, 4, 16, 64, 3, 1, 1, ldx=4096))
    d = _desc(32767, 4, 4, 16, 64, 3, 1, 1, ldx=4096)
    assert _accepted(L, d) and L.raw('contrad_conv2d_wino_ok')(ctypes.byref(d), 0) == 1
    assert _refused(L, _desc(32768, 4, 4, 64, 16, 3, 1, 1, ldy=4096))
    d = _desc(32767, 4, 4, 64, 16, 3, 1, 1, ldy=4096)
    assert _accepted(L, d) and L.raw('contrad_conv2d_wino_ok')(ctypes.byref(d), 1) == 1
    # the packed filter: KH * KW * C * ldw
    assert _refused(L, _desc(2, 4, 4, 4096, 8, 1, 1, 0, ldw=2 ** 19))
    assert _accepted(L, _desc(2, 4, 4, 4096, 8, 1, 1, 0, ldw=2 ** 19 - 4))


# Block-relative guards, one shape per family: (path, mode, N, H, C, K, k, stride, pad, images per block, which ld grows)
# N is small enough for the grown operand to stay below 2^31 elements and the channel counts large enough for the launch to
# fill the chip (the plan rule of the family), so that the guard alone decides.
GUARD_SHAPES = [
    (7, 0, 3, 32, 16, 1024, 3, 1, 1, 1, 'y'),           # Wino::ok, 32 x 32: one image per block
    (7, 1, 3, 32, 1024, 16, 3, 1, 1, 1, 'x'),
    (9, 0, 3, 32, 32, 2560, 3, 1, 1, 1, 'y'),           # Wino44::ok, W >= 32: one image
    (9, 1, 3, 32, 2560, 32, 3, 1, 1, 1, 'y'),
    (11, 0, 3, 32, 32, 1248, 3, 1, 1, 1, 'x'),          # the same guard, 32-wide cout blocks
    (8, 0, 7, 32, 8, 3200, 4, 2, 1, 2, 'x'),            # Wino22::ok, 16 x 16 grid: 128 / 64 = 2 images
    (8, 1, 7, 32, 768, 16, 4, 2, 1, 2, 'x'),
    (10, 0, 7, 33, 16, 3712, 3, 2, 0, 2, 'x'),          # Wino23::ok, 16 x 16 grid: 2 images
    (7, 2, 7, 32, 512, 256, 3, 1, 1, 2, 'y'),           # WinoWgrad::ok: chunks of at most 2 images
    (8, 2, 7, 32, 512, 512, 4, 2, 1, 2, 'x'),           # Wino22Wgrad::ok
]


def _around(nimg, H, W):
    """(under, over): the leading dimensions (multiples of 4) either side of nimg * H * W * ld * 4 = 2^31."""
    over = -(-2 ** 31 // (nimg * H * W * 4))
    over = (over + 3) // 4 * 4
    assert nimg * H * W * (over - 4) * 4 < 2 ** 31 <= nimg * H * W * over * 4
    return over - 4, over


@pytest.mark.parametrize('shape', GUARD_SHAPES, ids=lambda s: 'p%d-m%d-%s' % (s[0], s[1], s[-1]))
def test_block_relative_guards_from_both_sides(L, shape):
    P, mode, N, H, C, K, k, s, p, nimg, side = shape
    under, over = _around(nimg, H, H)
    paths = []
    for ld in (under, over):
        d = _desc(N, H, H, C, K, k, s, p, **{'ld' + side: ld})
        assert N * H * H * ld < 2 ** 31
        paths.append(L.raw('contrad_conv2d_path')(ctypes.byref(d), mode))
    assert paths[0] == P, (shape, paths)
    assert 0 <= paths[1] < 4, (shape, paths)            # over: a direct family of the igemm engine
    dense = _desc(N, H, H, C, K, k, s, p)
    assert L.raw('contrad_conv2d_path')(ctypes.byref(dense), mode) == P


def test_lean_guard_from_both_sides(L):
    """lean_ok (csrc/igemm.hip): the images one 128-row tile can touch stay below 2^31 bytes -- under plans the lean loop
    (paths 2 / 3), over the general kernel (path 1)."""
    # forward, 8 x 8 maps: 128 / 64 + 2 = 4 images
    under, over = _around(4, 8, 8)
    assert L.raw('contrad_conv2d_path')(ctypes.byref(_desc(15, 8, 8, 16, 8, 1, 1, 0, ldx=under)), 0) in (2, 3)
    assert L.raw('contrad_conv2d_path')(ctypes.byref(_desc(15, 8, 8, 16, 8, 1, 1, 0, ldx=over)), 0) == 1
    # data gradient: the same count over gy
    assert L.raw('contrad_conv2d_path')(ctypes.byref(_desc(15, 8, 8, 8, 16, 1, 1, 0, ldy=under)), 1) in (2, 3)
    assert L.raw('contrad_conv2d_path')(ctypes.byref(_desc(15, 8, 8, 8, 16, 1, 1, 0, ldy=over)), 1) == 1


def test_fir_forms_of_the_far_cases_and_the_per_image_rule(M):
    form = _load('test_aug_sg2_ref64_cpu').upfirdn_form
    seen = set()
    for case in M.UF_FAR_CASES:
        assert form(*M.uf_cfg(case)) == case[0], case
        seen.add(case[0])
    assert seen == {'u1d1_buf', 'u1d2_buf', 'u2d1_buf', 'u1d1_ptr', 'u1d2_ptr', 'u2d1_ptr'}
    for case in M.MODCONV_FAR_CASES:
        assert form(case[1], case[2], case[3], case[4], 4, 4, 1, 1, 1, 1, *M.FIR_PADS[(1, 1)]) == case[0]
    # one image of exactly 2^31 bytes takes the pointer form, 512 KiB less the branch-free one (input side, output side)
    pads = M.FIR_PADS[(1, 1)]
    assert form(1, 4096, 4096, 32, 4, 4, 1, 1, 1, 1, *pads) == 'u1d1_ptr'
    assert form(1, 4096, 4095, 32, 4, 4, 1, 1, 1, 1, *pads) == 'u1d1_buf'
    assert form(1, 4096, 4096, 32, 4, 4, 1, 1, 2, 2, *M.FIR_PADS[(1, 2)]) == 'u1d2_ptr'
    assert form(1, 4096, 4095, 32, 4, 4, 1, 1, 2, 2, *M.FIR_PADS[(1, 2)]) == 'u1d2_buf'
    assert form(1, 2048, 2048, 32, 4, 4, 2, 2, 1, 1, *M.FIR_PADS[(2, 1)]) == 'u2d1_ptr'
    assert form(1, 2048, 2047, 32, 4, 4, 2, 2, 1, 1, *M.FIR_PADS[(2, 1)]) == 'u2d1_buf'
