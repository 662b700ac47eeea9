"""Sub-forms of the direct conv families (paths 0 - 3: csrc/igemm.hip, igemm_lean.h) and the table of cases that runs each of
them against float64 (tests/test_igemm_forms_gpu.py).  No GPU and no torch here: tests/test_conv_plan_cpu.py reads the same
table to prove, from the plan queries alone, that it reaches every sub-form the shipped planner returns.

A sub-form is what the public queries tell apart below the (path, mode, split) triple:
    (path, mode, bm, bn, split, tile-order table present, stride of a data gradient -- 0 in the other modes)
One "path 2" is five kernel templates per mode (igemm_lean_kernel<MODE, 128 | 64, 128 | 64 | 32>), path 1 four
(igemm_kernel<MODE, BM, BN, true>), path 3 three tile walks, and a strided data gradient decodes its block id in one of three
orders.  The larger tiles are planned for large batches only, so most cases force their tile and split count on the development
library (contrad_dev_plan_override); the development switches are read once per process, hence one child process per GROUP.
"""
import ctypes

# environment of the child process of each group: the tile mode is pinned everywhere, so that a form is unambiguous
GROUPS = {
    'img': {'CONTRAD_TILEMODE': '0'},                                       # image-major tiles, plain strided order
    'bal': {'CONTRAD_TILEMODE': '0', 'CONTRAD_DGRAD_BALANCE': '2'},         # ... balanced strided order
    'pix': {'CONTRAD_TILEMODE': '1'},                                       # pixel-major tiles, whole-launch tables
    'pixblk': {'CONTRAD_TILEMODE': '1', 'CONTRAD_PIXORDER_FULL': '0'},      # ... per-block tables only
    'border': {'CONTRAD_TILEMODE': '2'},                                    # border classes
}
SWITCHES = ('CONTRAD_TILEMODE', 'CONTRAD_DGRAD_BALANCE', 'CONTRAD_PIXORDER_FULL', 'CONTRAD_PIXMAJOR_STRIDED',
            'CONTRAD_TEST_EXPECT_DGRAD_PATH')
CHILD_ENV = 'CONTRAD_TEST_FORM_GROUP'           # set by the parent tests: the group whose cases this process runs


def cdiv(a, b):
    return (a + b - 1) // b


def round4(v):
    return (v + 3) // 4 * 4


class Form(object):
    """One case: `kind` names the block-to-tile decode (and with it the expected grid), `ov` the forced (bm, bn, splits) or
    None for the library's own plan, `shape` = (N, H, W, C, K, k, stride, pad); path / bm / bn / split / table are DECLARED and
    checked against the queries before the case runs."""

    def __init__(self, group, kind, mode, ov, shape, path, bm, bn, split, table, what=''):
        self.group, self.kind, self.mode, self.ov, self.shape = group, kind, mode, ov, shape
        self.path, self.bm, self.bn, self.split, self.table, self.what = path, bm, bn, split, table, what

    @property
    def lds(self):
        """(ldx, ldy, ldw): 4 floats past the channel count rounded to 4 -- every output has sentinel columns."""
        N, H, W, C, K = self.shape[:5]
        return round4(C) + 4, round4(K) + 4, round4(K) + 4

    @property
    def signature(self):
        return (self.path, self.mode, self.bm, self.bn, self.split, self.table, self.shape[6] if self.mode == 1 else 0)

    @property
    def id(self):
        ov = 'plan' if self.ov is None else 'ov%dx%dx%d' % self.ov
        return 'form_%s_%s-m%d-%s-%s' % (self.group, self.kind, self.mode, ov, 'x'.join(map(str, self.shape)))

    def desc(self):
        from contrad_amd import _lib
        N, H, W, C, K, k, s, p = self.shape
        ldx, ldy, ldw = self.lds
        return _lib.ConvDesc(N, H, W, C, ldx, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, K, ldy, k, k, s, p, ldw)

    def expected_blocks(self):
        """Workgroups of the main launch, from the declared form alone (igemm.hip: fwd_setup / dgrad_setup / wgrad_setup)."""
        N, H, W, C, K, k, s, p = self.shape
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        bm, bn = self.bm, self.bn
        if self.mode == 2:
            ptiles = cdiv(N * Ho * Wo, 16)
            tiles = cdiv(k * k * C, bm) * cdiv(K, bn)
            pps = min(ptiles, max(4, cdiv(ptiles, max(1, 1024 // tiles))))
            return tiles * cdiv(ptiles, pps)
        ncol, sd = (K, 1) if self.mode == 0 else (C, s)
        npix = Ho * Wo if self.mode == 0 else cdiv(H, sd) * cdiv(W, sd)
        tn = cdiv(ncol, bn)
        tm = cdiv(N * npix, bm)
        if self.kind in ('pix', 'pixfull'):
            return cdiv(N, bm) * npix * tn
        if self.kind == 'pixcls':                      # class-major: every parity class walks the whole table
            return cdiv(N, bm) * npix * tn * 4
        if self.kind == 'border':
            return self._border_blocks(Ho, Wo) * tn
        if self.kind == 'bal':                         # groups of 8 tile indices: 8 + 4 + 4 + 2 blocks of the four classes
            return cdiv(tm, 8) * 18 * tn
        if self.kind == 'plain':                       # class groups padded to whole groups, four classes
            g = min(max(1, 32 // tn), tm)
            return cdiv(tm, g) * g * tn * 4
        splits = 1
        if self.split:
            depth = K if self.mode == 1 else C
            t_total = k * k * depth // 16
            splits = cdiv(t_total, cdiv(t_total, self.ov[2]))
        return tm * tn * splits


    def _border_blocks(self, Ho, Wo):
        """Border classes (igemm.hip: fill_border_classes): the pixels of a map fall into rectangles whose pixels read padding
        at the same taps; every XCD walks an eighth of each class's tiles, the grid is 8 x the largest such share."""
        N, H, W, C, K, k, s, p = self.shape

        def runs(extent, in_ext):
            lens, prev = [], None
            for o in range(extent):
                pos = [o * s - p + t if self.mode == 0 else o + p - t for t in range(k)]
                m = tuple(0 <= i < in_ext for i in pos)
                if m != prev:
                    lens.append(0)
                    prev = m
                lens[-1] += 1
            return lens
        hl, wl = (runs(Ho, H), runs(Wo, W)) if self.mode == 0 else (runs(H, Ho), runs(W, Wo))
        tiles = [cdiv(N * a * b, self.bm) for a in hl for b in wl]
        return 8 * max(sum(((x + 1) * n >> 3) - (x * n >> 3) for n in tiles) for x in range(8))


def _cases():
    F = Form
    T4 = ((128, 128), (64, 128), (128, 64), (64, 64))
    out = []
    # ---- lean loop, image-major, stride 1: forward and data gradient, four tiles, unsplit and split ----------------------
    # 243 rows (ragged at 64 and at 128), 136 columns (128 + 8, 2 x 64 + 8), 81 K-tiles in 4 splits of 21 / 21 / 21 / 18
    # (unsplit: 48 channels deep, 27 K-tiles -- the contraction depths stay inside what FAMILY_TOL was measured at)
    for (bm, bn) in T4:
        out.append(F('img', 'img', 0, (bm, bn, 0), (3, 9, 9, 48, 136, 3, 1, 1), 2, bm, bn, False, False))
        out.append(F('img', 'img', 1, (bm, bn, 0), (3, 9, 9, 136, 48, 3, 1, 1), 2, bm, bn, False, False))
        out.append(F('img', 'img', 0, (bm, bn, 4), (3, 9, 9, 144, 136, 3, 1, 1), 2, bm, bn, True, False))
        out.append(F('img', 'img', 1, (bm, bn, 4), (3, 9, 9, 136, 144, 3, 1, 1), 2, bm, bn, True, False))
    # the deep linear layer (merged heads): 5 rows, 65 K-tiles in 8 splits of 9 .. 9, 2
    out.append(F('img', 'img', 0, (128, 128, 8), (5, 1, 1, 1040, 136, 1, 1, 0), 2, 128, 128, True, False, 'deep linear'))
    out.append(F('img', 'img', 1, (64, 128, 8), (5, 1, 1, 136, 1040, 1, 1, 0), 2, 64, 128, True, False, 'deep linear'))
    # ---- lean weight gradient: the tile follows Kg and K (wgrad_plan), one slab (<= 4 position tiles) and several ---------
    for (C, K, k, bm, bn) in ((24, 136, 3, 128, 128), (40, 136, 1, 64, 128), (24, 40, 3, 128, 64), (40, 40, 1, 64, 64),
                              (24, 20, 3, 128, 32)):
        p = 1 if k == 3 else 0
        out.append(F('img', 'wgrad', 2, None, (1, 8, 8, C, K, k, 1, p), 2, bm, bn, False, False, 'one slab'))
        out.append(F('img', 'wgrad', 2, None, (5, 4, 4, C, K, k, 1, p), 2, bm, bn, True, False, '5 position tiles: slabs of 4 and 1'))
    # ---- general float4 loop (path 1): channels a multiple of 4, not of 16 (8: the depth FAMILY_TOL was measured at) ---------
    for (bm, bn) in T4:
        out.append(F('img', 'img', 0, (bm, bn, 0), (3, 9, 9, 8, 136, 3, 1, 1), 1, bm, bn, False, False))
        out.append(F('img', 'img', 1, (bm, bn, 0), (3, 9, 9, 136, 8, 3, 1, 1), 1, bm, bn, False, False))
    for (C, K, k, bm, bn) in ((24, 136, 3, 128, 128), (24, 136, 1, 64, 128), (24, 40, 3, 128, 64), (24, 40, 1, 64, 64)):
        p = 1 if k == 3 else 0
        out.append(F('img', 'wgrad', 2, None, (1, 7, 7, C, K, k, 1, p), 1, bm, bn, False, False, '49 positions: one ragged slab'))
        out.append(F('img', 'wgrad', 2, None, (1, 9, 9, C, K, k, 1, p), 1, bm, bn, True, False, '81 positions: slabs of 4 and 2 tiles'))
    # ---- strided data gradient, plain class-group order ---------------------------------------------------------------------
    for (bm, bn) in T4:
        out.append(F('img', 'plain', 1, (bm, bn, 0), (3, 17, 17, 80, 144, 3, 2, 0), 2, bm, bn, False, False, '3x3 s2 p0, odd map'))
        out.append(F('img', 'plain', 1, (bm, bn, 0), (3, 10, 10, 80, 144, 4, 2, 1), 2, bm, bn, False, False, '4x4 s2 p1'))
    for (bm, bn) in ((128, 128), (64, 64)):
        out.append(F('img', 'plain', 1, (bm, bn, 0), (3, 9, 9, 80, 144, 1, 2, 0), 2, bm, bn, False, False,
                     '1x1 s2: three empty parity classes write zeros'))
    out.append(F('img', 'plain', 1, None, (3, 17, 17, 24, 144, 3, 2, 0), 2, 128, 32, False, False, '128x32'))
    out.append(F('img', 'plain', 1, (64, 64, 0), (83, 9, 9, 40, 48, 3, 2, 0), 2, 64, 64, False, False,
                 'cgroup 32: 33 M-tiles, groups of 32 and 1'))
    out.append(F('img', 'plain', 1, (128, 128, 0), (83, 9, 9, 136, 48, 3, 2, 0), 2, 128, 128, False, False,
                 'cgroup 16: 17 M-tiles x 2 N-tiles'))
    out.append(F('img', 'plain', 1, (128, 64, 0), (21, 9, 9, 456, 48, 3, 2, 0), 2, 128, 64, False, False,
                 'cgroup 4: 5 M-tiles x 8 N-tiles'))
    out.append(F('img', 'plain', 1, None, (2, 7, 7, 3, 5, 3, 2, 1), 0, 64, 64, False, False, 'path 0, strided'))
    for (bm, bn) in T4:                             # the general loop walks the same class groups (8 gy channels: not lean)
        out.append(F('img', 'plain', 1, (bm, bn, 0), (3, 17, 17, 80, 8, 3, 2, 0), 1, bm, bn, False, False, 'general loop, strided'))
    # ---- balanced order (3x3 stride 2) ---------------------------------------------------------------------------------------
    for (bm, bn) in T4:
        for pad in (0, 1):
            out.append(F('bal', 'bal', 1, (bm, bn, 0), (7, 17, 17, 80, 144, 3, 2, pad), 2, bm, bn, False, False))
    # ---- pixel-major tiles -----------------------------------------------------------------------------------------------------
    # 130 images: ragged last image block at 64 and at 128 rows; the whole-launch table exists where 32 % N-tiles == 0
    for (bm, bn) in T4:
        full = bn == 128
        out.append(F('pix', 'pixfull' if full else 'pix', 0, (bm, bn, 0), (130, 4, 4, 16, 136, 3, 1, 1), 3, bm, bn, False, full))
        out.append(F('pix', 'pixfull' if full else 'pix', 1, (bm, bn, 0), (130, 4, 4, 136, 32, 3, 1, 1), 3, bm, bn, False, full))
    # one N-tile: the table exists at the 64-wide tiles too; <= 32 columns: the 128x32 tile (the library's own plan)
    for (bm, bn) in ((128, 64), (64, 64)):
        out.append(F('pix', 'pixfull', 0, (bm, bn, 0), (130, 4, 4, 16, 64, 3, 1, 1), 3, bm, bn, False, True))
        out.append(F('pix', 'pixfull', 1, (bm, bn, 0), (130, 4, 4, 64, 32, 3, 1, 1), 3, bm, bn, False, True))
    out.append(F('pix', 'pixfull', 0, None, (130, 4, 4, 16, 24, 3, 1, 1), 3, 128, 32, False, True, '128x32'))
    out.append(F('pix', 'pixfull', 1, None, (130, 4, 4, 24, 32, 3, 1, 1), 3, 128, 32, False, True, '128x32'))
    for (bm, bn) in ((128, 128), (64, 128)):
        out.append(F('pixblk', 'pix', 0, (bm, bn, 0), (130, 4, 4, 16, 136, 3, 1, 1), 3, bm, bn, False, False))
        out.append(F('pixblk', 'pix', 1, (bm, bn, 0), (130, 4, 4, 136, 32, 3, 1, 1), 3, bm, bn, False, False))
    for (bm, bn) in ((128, 64), (64, 64)):
        out.append(F('pix', 'pixcls', 1, (bm, bn, 0), (130, 8, 8, 40, 64, 4, 2, 1), 3, bm, bn, False, True,
                     'class-major mirrored table'))
    for (bm, bn) in ((128, 128), (64, 128)):
        out.append(F('pix', 'pixcls', 1, (bm, bn, 0), (130, 8, 8, 136, 64, 4, 2, 1), 3, bm, bn, False, True,
                     'class-major mirrored table, two N-tiles'))
    out.append(F('pix', 'pixcls', 1, None, (130, 8, 8, 24, 64, 4, 2, 1), 3, 128, 32, False, True, 'class-major, 128x32'))
    for (K, bn) in ((72, 128), (40, 64), (20, 32)):
        out.append(F('pix', 'wgrad', 2, None, (144, 4, 4, 128, K, 3, 1, 1), 3, 128, bn, True, False, 'pixel-major positions'))
    for (K, bn) in ((72, 128), (40, 64)):
        out.append(F('pix', 'wgrad', 2, None, (16, 2, 2, 128, K, 3, 1, 1), 3, 128, bn, False, False, 'pixel-major positions, one slab'))
    # ---- border classes ------------------------------------------------------------------------------------------------------
    for (bm, bn) in T4:
        out.append(F('border', 'border', 0, (bm, bn, 0), (130, 8, 8, 16, 72, 3, 1, 1), 3, bm, bn, False, False))
        out.append(F('border', 'border', 1, (bm, bn, 0), (130, 8, 8, 72, 16, 3, 1, 1), 3, bm, bn, False, False))
    for (bm, bn) in ((128, 128), (64, 64)):
        out.append(F('border', 'border', 0, (bm, bn, 0), (130, 12, 20, 16, 72, 4, 2, 1), 3, bm, bn, False, False,
                     '4x4 s2 onto a 6 x 10 map'))
    return out


FORM_CASES = _cases()


def report(L, d, mode):
    """What the public plan queries say about (d, mode): dict(path, bm, bn, split, table, blocks); None for a rejected one."""
    P = L.raw('contrad_conv2d_path')(ctypes.byref(d), mode)
    if P < 0:
        return None
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    assert L.raw('contrad_conv2d_tile')(ctypes.byref(d), mode, ctypes.byref(bm), ctypes.byref(bn)) == 0
    if mode == 0:
        split = L.raw('contrad_conv2d_fwd_workspace_bytes')(ctypes.byref(d)) > 0
    elif mode == 1:
        split = L.raw('contrad_conv2d_dgrad_workspace_bytes')(ctypes.byref(d)) > 0
    else:                                                 # more than one slab of the packed gradient + bias partials
        split = L.raw('contrad_conv2d_wgrad_workspace_bytes')(ctypes.byref(d)) > (d.KH * d.KW * d.C + 1) * d.K * 4
    table = False
    if mode != 2:
        buf = (ctypes.c_ubyte * 256)()
        n = L.raw('contrad_conv2d_tile_order')(ctypes.byref(d), mode, buf, 256)
        assert n >= 0
        table = n > 0
    blocks = L.raw('contrad_conv2d_grid_blocks')(ctypes.byref(d), mode, 1)
    return dict(path=P, bm=bm.value, bn=bn.value, split=split, table=table, blocks=blocks)


def signature(L, d, mode):
    """The sub-form of (d, mode) on the direct families; None when the layer is rejected or another family's."""
    r = report(L, d, mode)
    if r is None or r['path'] >= 4:
        return None
    return (r['path'], mode, r['bm'], r['bn'], r['split'], r['table'], d.stride if mode == 1 else 0)


def set_override(L, ov):
    """contrad_dev_plan_override of the development library (a runtime global: reset it to (0, 0, 0) in a finally)."""
    fn = L._dll.contrad_dev_plan_override
    fn.restype, fn.argtypes = None, [ctypes.c_int] * 3
    fn(*(ov or (0, 0, 0)))


def form_report(L, case):
    """report() of a case under its forced plan (the caller's process carries the group's environment)."""
    set_override(L, case.ov)
    try:
        return report(L, case.desc(), case.mode)
    finally:
        set_override(L, None)


def mismatch(case, r):
    """'' when the queries report the declared form, else what differs."""
    if r is None:
        return 'rejected descriptor'
    want = dict(path=case.path, bm=case.bm, bn=case.bn, split=case.split, table=case.table)
    bad = ['%s: declared %s, reported %s' % (k, want[k], r[k]) for k in sorted(want) if want[k] != r[k]]
    eb = case.expected_blocks()
    if eb is not None and eb != r['blocks']:
        bad.append('blocks: declared form gives %d, reported %d' % (eb, r['blocks']))
    return '; '.join(bad)


if __name__ == '__main__':          # python tests/igemm_forms.py GROUP: the reports of a group's cases as JSON (no GPU needed)
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from contrad_amd import _lib
    print(json.dumps([form_report(_lib.lib(), c) for c in FORM_CASES if c.group == sys.argv[1]]))
