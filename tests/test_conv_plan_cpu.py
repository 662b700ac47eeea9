"""Plan coverage of the conv engine, host logic only (no GPU): the path / workspace / *_ok queries of include/contrad_hip.h.

* Every (path, mode, split-K) triple the planner returns over the BASELINE layers and a grid of small and odd shapes is
  reached by a case of the GPU parity matrix (tests/test_conv_paths_gpu.py: PATH_CASES), and each case's declared path is
  what the planner says -- a planner change that opens a path, or moves a case off its path, fails here.
* Below the triple, on the direct families (paths 0 - 3): every sub-form (path, mode, bm, bn, split, tile-order table,
  data-gradient stride) the planner returns over the same descriptors is declared by a case of PATH_CASES or of the form
  table (tests/igemm_forms.py, run on the GPU by tests/test_igemm_forms_gpu.py), and each form case's declared form is what
  the library reports in that case's environment -- a planner change that opens a sub-form fails here.
* The Winograd workspace queries return -22 exactly where the matching *_ok query rejects the shape.
* The supported-map statement of include/contrad_hip.h (F(2x2,3x3) / F(4x4,3x3)) is what wino_ok / wino44_ok do.
"""
import ctypes
import importlib.util
import os

import pytest

from contrad_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu_matrix():
    """The GPU matrix module, loaded for its case table only (importing it touches no GPU)."""
    spec = importlib.util.spec_from_file_location('_conv_paths_cases', os.path.join(_HERE, 'test_conv_paths_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.path.insert(0, _HERE)          # (its fp64 helper module lives beside it)
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


def _desc(N, H, W, C, K, k, s, p, ldx=None, ldy=None, ldw=None):
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return _lib.ConvDesc(N, H, W, C, ldx or C, Ho, Wo, K, ldy or K, k, k, s, p, ldw or (K + 3) // 4 * 4)


def triple(L, d, mode):
    """(path, mode, split-K) of a descriptor, from the public queries only; None for a rejected one."""
    P = L.raw('contrad_conv2d_path')(ctypes.byref(d), mode)
    if P < 0:
        return None
    if P >= 7 and mode != 2:
        split = False                                     # (Winograd: the workspace holds the transformed filter)
    elif mode == 0:
        split = L.raw('contrad_conv2d_fwd_workspace_bytes')(ctypes.byref(d)) > 0
    elif mode == 1:
        split = L.raw('contrad_conv2d_dgrad_workspace_bytes')(ctypes.byref(d)) > 0
    else:                                                 # more than one slab of the packed gradient + bias partials
        split = L.raw('contrad_conv2d_wgrad_workspace_bytes')(ctypes.byref(d)) > (d.KH * d.KW * d.C + 1) * d.K * 4
    return (P, mode, split)


# (H, Cin, Cout, k, stride, pad) of every conv-engine layer of the BASELINE discriminators
_SNDCGAN = [(32, 3, 64, 3, 1, 1), (32, 64, 128, 4, 2, 1), (16, 128, 128, 3, 1, 1), (16, 128, 256, 4, 2, 1),
            (8, 256, 256, 3, 1, 1), (8, 256, 512, 4, 2, 1), (4, 512, 512, 3, 1, 1),
            (1, 8192, 1536, 1, 1, 0), (1, 512, 1, 1, 1, 0), (1, 512, 128, 1, 1, 0)]        # (merged heads, logit, projection)


def _stylegan2(size, ch):
    layers = []
    R = size
    while R > 4:
        ci, co = ch[R], ch[R // 2]
        layers += [(R, ci, ci, 3, 1, 1), (R + 1, ci, co, 3, 2, 0), (R // 2, ci, co, 1, 1, 0)]
        R //= 2
    layers += [(4, 528, 512, 3, 1, 1), (1, 8192, 512, 1, 1, 0), (1, 512, 1, 1, 1, 0), (1, 512, 128, 1, 1, 0)]
    return layers


_SG2_32 = _stylegan2(32, {32: 512, 16: 512, 8: 512, 4: 512}) + _stylegan2(32, {32: 128, 16: 256, 8: 512, 4: 512})
_SG2_512 = _stylegan2(512, {512: 64, 256: 128, 128: 256, 64: 512, 32: 512, 16: 512, 8: 512, 4: 512}) + \
    _stylegan2(512, {512: 32, 256: 64, 128: 128, 64: 256, 32: 512, 16: 512, 8: 512, 4: 512})


def baseline_descs():
    for N in (1536, 192):
        for (H, C, K, k, s, p) in _SNDCGAN:
            yield _desc(N, H, H, C, K, k, s, p)
    for N in (48, 16, 4):
        for (H, C, K, k, s, p) in _SG2_32 + _SG2_512:
            yield _desc(N, H, H, C, K, k, s, p)


def grid_descs():
    for N in (1, 2, 5, 16, 48, 192, 1536):
        for H in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 64):
            for C in (3, 8, 16, 32, 48, 64, 96, 128, 160, 256, 512):
                for K in (1, 8, 32, 64, 96, 128, 160, 256, 512):
                    for (k, s, p) in ((1, 1, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1), (4, 2, 1)):
                        if H + 2 * p >= k:
                            yield _desc(N, H, H, C, K, k, s, p)
    for (H, W) in ((4, 8), (8, 4), (16, 32), (32, 16), (64, 32), (32, 64), (16, 64), (8, 32), (5, 9)):
        for (C, K) in ((16, 64), (32, 64), (32, 32), (64, 128), (48, 192)):
            for N in (2, 48, 192):
                yield _desc(N, H, W, C, K, 3, 1, 1)


def reachable(L):
    found = set()
    for d in list(baseline_descs()) + list(grid_descs()):
        for mode in (0, 1, 2):
            t = triple(L, d, mode)
            if t is not None:
                found.add(t)
    return found


def test_the_gpu_matrix_reaches_every_planned_path(L):
    M = _gpu_matrix()
    declared = set()
    for case in M.PATH_CASES:
        P, mode, split = case[:3]
        d = M.case_desc(case)
        assert triple(L, d, mode) == (P, mode, split), (M.case_id(case), triple(L, d, mode))
        declared.add((P, mode, split))
    missing = reachable(L) - declared
    assert not missing, 'planner triples no GPU parity case reaches: %s' % sorted(missing)
    assert {P for (P, _, _) in declared} == set(range(12))       # (and every family of contrad_conv2d_path's list)


def _forms():
    """tests/igemm_forms.py (it lives beside this module)."""
    import sys
    sys.path.insert(0, _HERE)
    try:
        import igemm_forms
    finally:
        sys.path.remove(_HERE)
    return igemm_forms


def test_the_form_table_reaches_every_planned_sub_form(L):
    """Shipped library: nothing the planner returns on paths 0 - 3 is left without a float64 case."""
    M, IF = _gpu_matrix(), _forms()
    declared = {c.signature for c in IF.FORM_CASES}
    for case in M.PATH_CASES:
        sig = IF.signature(L, M.case_desc(case), case[1])
        if sig is not None:
            declared.add(sig)
    reached = set()
    for d in list(baseline_descs()) + list(grid_descs()):
        for mode in (0, 1, 2):
            reached.add(IF.signature(L, d, mode))
    reached.discard(None)
    missing = reached - declared
    assert missing == set(), 'planner sub-forms no float64 case runs: %s' % sorted(missing)
    assert {c.path for c in IF.FORM_CASES} == {0, 1, 2, 3}
    assert len({c.id for c in IF.FORM_CASES}) == len(IF.FORM_CASES)


@pytest.mark.parametrize('group', ['bal', 'border', 'img', 'pix', 'pixblk'])
def test_every_form_case_declares_what_the_library_reports(L, group):
    """In a child process with the group's environment, on the development library (host queries only: no GPU)."""
    import json
    import subprocess
    import sys
    from contrad_amd import build
    IF = _forms()
    assert sorted(IF.GROUPS) == ['bal', 'border', 'img', 'pix', 'pixblk']
    assert os.path.exists(build.DEV_LIB)
    env = dict(os.environ)
    for name in IF.SWITCHES:
        env.pop(name, None)
    env.update(IF.GROUPS[group])
    env['CONTRAD_HIP_LIB'] = build.DEV_LIB
    r = subprocess.run([sys.executable, os.path.join(_HERE, 'igemm_forms.py'), group], env=env, capture_output=True, text=True,
                       timeout=120, cwd=os.path.dirname(_HERE))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cases = [c for c in IF.FORM_CASES if c.group == group]
    reports = json.loads(r.stdout)
    assert len(reports) == len(cases) > 0
    for case, rep in zip(cases, reports):
        assert not IF.mismatch(case, rep), (case.id, IF.mismatch(case, rep))
        assert rep['path'] < 4
        # a forced plan stays inside what the planner emits at some shape (igemm.hip: pick_tile, split_plan)
        N, H, W, C, K, k, s, p = case.shape
        if case.mode != 2:
            ncol, depth = (K, C) if case.mode == 0 else (C, K)
            assert case.bn <= 64 or ncol > 64, case.id
            if case.split:
                t_total = k * k * depth // 16
                assert t_total >= 32 and -(-t_total // case.ov[2]) >= 8, case.id


def test_the_plan_queries_agree_with_one_another(L):
    """The queries read one route decision (csrc/igemm.hip: conv_route): over the same descriptors, modes 0 and 1, the
    transformed-filter kind is the path's family (11 reads 9's filter) and non-zero exactly on the Winograd paths, its bytes
    are the mode's workspace, and only a path-3 plan -- or the direct route a Winograd plan falls through to without its
    workspace -- has a tile-order table."""
    path, kind, order = L.raw('contrad_conv2d_path'), L.raw('contrad_conv2d_filter_kind'), L.raw('contrad_conv2d_tile_order')
    ws = (L.raw('contrad_conv2d_fwd_workspace_bytes'), L.raw('contrad_conv2d_dgrad_workspace_bytes'))
    buf = (ctypes.c_ubyte * 256)()
    rows = fallback = 0
    for d in list(baseline_descs()) + list(grid_descs()):
        for mode in (0, 1):
            P = path(ctypes.byref(d), mode)
            if P < 0:
                continue
            rows += 1
            nb = ctypes.c_longlong(-1)
            k = kind(ctypes.byref(d), mode, ctypes.byref(nb))
            what = (d.N, d.H, d.W, d.C, d.K, d.KH, d.stride, d.pad, mode, P, k)
            assert (k != 0) == (7 <= P <= 11), what
            assert k == (0 if P < 7 else 9 if P == 11 else P), what
            assert nb.value == (ws[mode](ctypes.byref(d)) if k else 0), what
            n = order(ctypes.byref(d), mode, buf, 256)
            assert n >= 0, what
            if n > 0:
                assert P == 3 or 7 <= P <= 11, what
                fallback += P != 3
    assert rows > 80000 and fallback > 0          # (the grid reaches the fall-through kind too)


def test_the_gpu_matrix_has_guard_bands_where_the_layout_allows(L):
    """Every output has a leading dimension above its channel count (sentinel columns) unless its family needs dense rows."""
    M = _gpu_matrix()
    for case in M.PATH_CASES:
        P, mode = case[:2]
        ldx, ldy, ldw = M.case_lds(case)
        C, K = case[6], case[7]
        out_ld, out_c = {0: (ldy, K), 1: (ldx, C), 2: (ldw, K)}[mode]
        assert out_ld > out_c or P in (4, 6), M.case_id(case)
        assert ldx % 4 == 0 and ldy % 4 == 0 and ldw % 4 == 0        # (slice offsets of 4 floats: 16-byte alignment kept)


_MAPS = (2, 4, 8, 16, 32, 64)
_CHANNELS = (8, 16, 32, 48, 64, 96, 128, 160)


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def wino22_supported(H, W, cin, cout):
    """F(2x2, 3x3) (include/contrad_hip.h): H, W powers of two >= 4; input channels % 16, output channels % 64."""
    return _pow2(H) and _pow2(W) and H >= 4 and W >= 4 and cin % 16 == 0 and cout % 64 == 0


def wino44_supported(H, W, cin, cout):
    """F(4x4, 3x3) (include/contrad_hip.h): powers of two, square 4 / 8 / 16 or W >= 32 and H >= 16; channels % 32."""
    maps = _pow2(H) and _pow2(W) and ((H == W and H in (4, 8, 16)) or (W >= 32 and H >= 16))
    return maps and cin % 32 == 0 and cout % 32 == 0


def _shapes():
    for H in _MAPS:
        for W in _MAPS:
            for C in _CHANNELS:
                for K in _CHANNELS:
                    yield H, W, C, K


def test_winograd_workspace_bytes_reject_exactly_what_ok_rejects(L):
    ok, ws = L.raw('contrad_conv2d_wino_ok'), L.raw('contrad_conv2d_wino_workspace_bytes')
    ok44, ws44 = L.raw('contrad_conv2d_wino44_ok'), L.raw('contrad_conv2d_wino44_workspace_bytes')
    geos = [(3, 1, 1), (4, 2, 1)]
    for (H, W, C, K) in _shapes():
        for (k, s, p) in geos:
            d = _desc(4, H, W, C, K, k, s, p)
            for mode in (0, 1, 2):
                assert (ws(ctypes.byref(d), mode) == -22) == (ok(ctypes.byref(d), mode) == 0), (H, W, C, K, k, mode)
                if ok(ctypes.byref(d), mode):
                    assert ws(ctypes.byref(d), mode) > 0
            any44 = ok44(ctypes.byref(d), 0) or ok44(ctypes.byref(d), 1)
            assert (ws44(ctypes.byref(d)) == -22) == (not any44), (H, W, C, K, k)
        if H == W:                                    # 3x3 stride 2 pad 0 on a (2G + 1)^2 map
            d = _desc(4, 2 * H + 1, 2 * W + 1, C, K, 3, 2, 0)
            for mode in (0, 1, 2):
                assert (ws(ctypes.byref(d), mode) == -22) == (ok(ctypes.byref(d), mode) == 0), (H, C, K, mode)


def test_the_supported_map_statement_is_what_the_kernels_accept(L):
    """Table-driven: the statement in include/contrad_hip.h, ops.conv2d_wino and csrc/wino44.h against wino_ok / wino44_ok
    on 3x3 stride-1 pad-1 layers (mode 1 swaps the roles: gy's K channels are the input)."""
    ok, ok44 = L.raw('contrad_conv2d_wino_ok'), L.raw('contrad_conv2d_wino44_ok')
    for (H, W, C, K) in _shapes():
        d = _desc(4, H, W, C, K, 3, 1, 1)
        for mode in (0, 1):
            cin, cout = (C, K) if mode == 0 else (K, C)
            assert ok(ctypes.byref(d), mode) == int(wino22_supported(H, W, cin, cout)), (H, W, C, K, mode)
            assert ok44(ctypes.byref(d), mode) == int(wino44_supported(H, W, cin, cout)), (H, W, C, K, mode)
    # the statements of the three places name the same maps
    root = os.path.dirname(_HERE)
    header = open(os.path.join(root, 'include', 'contrad_hip.h')).read()
    doc = open(os.path.join(root, 'contrad_amd', 'ops.py')).read()
    w44 = open(os.path.join(root, 'contrad_amd', 'csrc', 'wino44.h')).read()
    for text in (header, doc, w44):
        flat = ' '.join(text.replace('//', ' ').replace('*', ' ').split())
        assert 'square 4x4 / 8x8 / 16x16, or W >= 32 and H >= 16' in flat
    for text in (header, doc):
        flat = ' '.join(text.replace('*', ' ').split())
        assert 'H and W powers of two >= 4, any aspect ratio; input channels a multiple of 16, output channels' in flat
