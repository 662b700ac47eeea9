"""The conv engine's plan as a table, host only (no GPU): one TSV row per accepted (descriptor, mode) over the BASELINE
layers and the shape grid of tests/test_conv_plan_cpu.py, from the public plan queries of include/contrad_hip.h.

    python tools/plan_table.py OUT.tsv            # the library contrad_amd loads (CONTRAD_HIP_LIB=<path> for another build)

Two builds plan alike exactly when their tables are the same bytes; the last line printed is `rows sha256 library`.  Behind
profiles/conv_route_identity.txt and profiles/wino_host_identity.txt (dev-library switches such as CONTRAD_WINO=0 go into the environment of the call).
"""
import ctypes
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from contrad_amd import _lib  # noqa: E402

COLUMNS = ('N H W C ldx Ho Wo K ldy KH KW stride pad ldw mode path bm bn workspace_bytes grid_ws grid_nows '
           'executed_fraction filter_kind filter_bytes order_len order_hash '
           'wino_ok wino_workspace_bytes wino44_ok wino44_workspace_bytes').split()
_WS = ('contrad_conv2d_fwd_workspace_bytes', 'contrad_conv2d_dgrad_workspace_bytes', 'contrad_conv2d_wgrad_workspace_bytes')


def _plan_cases():
    spec = importlib.util.spec_from_file_location('_conv_plan_cases', os.path.join(ROOT, 'tests', 'test_conv_plan_cpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.baseline_descs()) + list(mod.grid_descs())


def rows(L):
    path, tile, grid = L.raw('contrad_conv2d_path'), L.raw('contrad_conv2d_tile'), L.raw('contrad_conv2d_grid_blocks')
    frac, kind, order = (L.raw('contrad_conv2d_executed_fraction'), L.raw('contrad_conv2d_filter_kind'),
                         L.raw('contrad_conv2d_tile_order'))
    # the forced entry points' own queries (they answer for shapes the plan sends elsewhere, too)
    wok, wws, w44ok, w44ws = (L.raw('contrad_conv2d_wino_ok'), L.raw('contrad_conv2d_wino_workspace_bytes'),
                              L.raw('contrad_conv2d_wino44_ok'), L.raw('contrad_conv2d_wino44_workspace_bytes'))
    buf = (ctypes.c_ubyte * 256)()
    for d in _plan_cases():
        p = ctypes.byref(d)
        for mode in (0, 1, 2):
            P = path(p, mode)
            if P < 0:
                continue
            bm, bn, nb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0)
            tile(p, mode, ctypes.byref(bm), ctypes.byref(bn))
            fk = kind(p, mode, ctypes.byref(nb))
            n = order(p, mode, buf, 256) if mode != 2 else 0
            oh = hashlib.sha256(bytes(buf[:n])).hexdigest()[:16] if n > 0 else '-'
            yield [getattr(d, f) for f, _ in d._fields_] + [
                mode, P, bm.value, bn.value, L.raw(_WS[mode])(p), grid(p, mode, 1), grid(p, mode, 0),
                repr(frac(p, mode)), fk, nb.value, n, oh, wok(p, mode), wws(p, mode), w44ok(p, mode), w44ws(p)]


def main(out):
    L = _lib.lib()
    h, n = hashlib.sha256(), 0
    with open(out, 'wb') as f:
        for r in [COLUMNS] + list(rows(L)):
            line = ('\t'.join(str(v) for v in r) + '\n').encode()
            f.write(line)
            h.update(line)
            n += 1
    print('%d %s %s' % (n - 1, h.hexdigest(), os.path.basename(_lib.LIB_PATH)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'plan_table.tsv')
