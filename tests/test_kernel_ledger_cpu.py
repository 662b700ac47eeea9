"""The kernel ledger (tests/kernel_ledger.py) against the built object files, the record profiles/kernel_ledger.txt and the
library's plan queries.  No GPU.

* the kernel instances the compiler emitted are exactly LEDGER | UNCOVERED: a new template instance without a parity module
  that launches it fails here, and so does a ledger line for a kernel that no longer exists;
* the development objects hold the same instances as the shipped ones;
* every ledger line names parity modules only, each inside the sources it is a parity module for, and the record has a
  non-zero dispatch count for every (instance, module) pair the ledger claims;
* every case the ledger names for a host-selected instance is in the table it names and selects that instance under the
  restated host arithmetic, which agrees with the library's queries (contrad_linhead_plan, contrad_conv2d_path) over a lattice;
* UNCOVERED is pinned: it can only shrink knowingly.
"""
import ctypes
import importlib
import os

import pytest

import kernel_ledger as KL
import wino_walks as WW
from contrad_amd import _lib, ops

UNCOVERED_PINNED = set()


@pytest.fixture(scope='module')
def built():
    objs = set(KL.shipped_objects()) | set(KL.dev_objects())
    if not os.path.exists(_lib.LIB_PATH) or not all(os.path.exists(o) for o in objs):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def compiled(built):
    return KL.instance_sources()


def test_normalise_keeps_namespaces_and_template_arguments():
    n = KL.normalise
    assert n('void (anonymous namespace)::__device_stub__igemm_lean_kernel<1, 128, 32, true>((anonymous namespace)::IgemmArgs)') \
        == 'igemm_lean_kernel<1, 128, 32, true>'
    assert n('void (anonymous namespace)::wino44n::wino44n_kernel<1, 6>((anonymous namespace)::wino44::Args) [clone .kd]') \
        == 'wino44n::wino44n_kernel<1, 6>'
    assert n('(anonymous namespace)::linhead_loss_kernel(float const*, float const*, long long const*, int, int, int, float, '
             'float*, float*, double*, unsigned long long*, unsigned int*)') == 'linhead_loss_kernel'
    assert n('void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int, '
             'at::native::FillFunctor<float>, std::array<char*, 1ul>)').startswith('at::native::vectorized_elementwise_kernel<4, ')
    long_name = 'ns::kernel<%s>' % ', '.join(str(i) for i in range(60))
    assert n('void %s(int)' % long_name) == long_name and len(long_name) > 200      # nothing is cut short


def test_compiled_instances_are_the_ledger(compiled):
    ledger, uncovered = set(KL.LEDGER), set(KL.UNCOVERED)
    assert not ledger & uncovered
    have = set(compiled)
    assert have - (ledger | uncovered) == set(), 'compiled instances without a ledger line'
    assert (ledger | uncovered) - have == set(), 'ledger lines for kernels the build no longer has'
    assert len(have) >= 211                    # the count at the commit that introduced the ledger


def test_development_objects_hold_the_same_instances(built):
    assert KL.compiled_instances(KL.dev_objects()) == KL.compiled_instances(KL.shipped_objects())
    dev_only = [o for o in KL.dev_objects() if o not in KL.shipped_objects()]
    ship_only = [o for o in KL.shipped_objects() if o not in KL.dev_objects()]
    assert [os.path.basename(o) for o in dev_only] == ['igemm_dev.o'] and [os.path.basename(o) for o in ship_only] == ['igemm.o']
    assert KL.compiled_instances(dev_only) == KL.compiled_instances(ship_only)


def test_ledger_lines_name_parity_modules_inside_their_sources(compiled):
    for m, (sources, why) in KL.PARITY_MODULES.items():
        assert os.path.exists(os.path.join(KL.ROOT, 'tests', m + '.py')), m
        assert why and sources and all(os.path.exists(os.path.join(KL.CSRC, s + '.hip')) for s in sources), m
    for inst, modules in KL.LEDGER.items():
        assert modules and len(set(modules)) == len(modules), inst
        for m in modules:
            assert m in KL.PARITY_MODULES, (inst, m)
            assert compiled[inst] in KL.PARITY_MODULES[m][0], (inst, m, compiled[inst])
    for inst, why in KL.UNCOVERED.items():
        assert why.strip() and '\n' not in why, inst


def test_the_record_agrees_with_the_ledger(compiled):
    rec = KL.read_record()
    assert set(rec) == set(compiled)
    for inst, modules in KL.LEDGER.items():
        for m in modules:
            got = rec[inst].get(m)
            assert got == KL.BY_PLAN_QUERY or (isinstance(got, int) and got > 0), (inst, m, got)
    for inst in rec:
        assert (not rec[inst]) == (inst in KL.UNCOVERED), inst             # NEVER exactly on the uncovered lines
        assert all(m in KL.PARITY_MODULES and compiled[inst] in KL.PARITY_MODULES[m][0] for m in rec[inst]), inst


def test_uncovered_is_pinned():
    assert set(KL.UNCOVERED) == UNCOVERED_PINNED


def _tables():
    paths = importlib.import_module('test_conv_paths_gpu')
    linhead = importlib.import_module('test_linhead_gpu')

    def wino_sel(P, mode, shape):
        return KL.wino_instance(tuple(shape), mode, f44=P in (9, 11))
    return {
        ('test_wino_walks_gpu', 'WALK_CASES'): {WW.case_id(c): [wino_sel(c[0], c[1], c[2:10])] for c in WW.WALK_CASES},
        ('test_conv_paths_gpu', 'PATH_CASES'): {paths.case_id(c): [wino_sel(c[0], c[1], c[3:11])]
                                                for c in paths.PATH_CASES if c[0] >= 7 and c[1] < 2},
        ('test_conv_paths_gpu', 'INSTANCE_CASES'): {c[14]: [wino_sel(c[0], c[1], c[3:11])] for c in paths.INSTANCE_CASES},
        ('test_linhead_gpu', 'CASES'): {'x'.join(str(v) for v in c): list(KL.linhead_instances(*c[:3])) for c, _form in linhead.CASES},
    }, paths, linhead


def test_host_selected_instances_are_selected_by_the_cases_the_ledger_names(compiled):
    tables, paths, linhead = _tables()
    templated = {i for i in compiled if i.startswith(('linhead_logits_kernel<', 'linhead_wgrad_kernel<', 'wino22::wino22_kernel<',
                                                     'wino23::wino23_kernel<', 'wino44::wino44_kernel<', 'wino44n::wino44n_kernel<'))}
    assert len(templated) == 12 + 6 + 3 + 6 + 8
    assert set(KL.HOST_SELECTED) == templated - set(KL.UNCOVERED)
    for inst, (module, table, case) in KL.HOST_SELECTED.items():
        assert module in KL.LEDGER[inst], inst
        assert inst in tables[(module, table)][case], (inst, module, table, case)
    for c in paths.INSTANCE_CASES:                        # the forced cases run the family their path number names
        assert c[14].split('::')[0] == {8: 'wino22', 9: 'wino44', 10: 'wino23', 11: 'wino44n'}[c[0]]
    for c, form in linhead.CASES:
        assert KL.linhead_plan(*c[:3]) == form


def test_the_restated_linhead_plan_agrees_with_the_library(built):
    seen = set()
    for N in (1, 37, 64, 65, 70, 256, 1000, 70000):
        for K in (1, 15, 64, 200, 300, 512, 8192):
            for C in list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 72, 80, 81, 96, 97, 100, 112, 113, 127, 128]:
                assert ops.linhead_plan(N, K, C) == KL.linhead_plan(N, K, C)[:3], (N, K, C)
                seen.update(KL.linhead_instances(N, K, C))
    assert seen == {'linhead_logits_kernel<%d>' % i for i in range(1, 9)} | {'linhead_wgrad_kernel<%d>' % i for i in range(1, 5)}


def test_the_restated_item_width_agrees_with_the_path_query(built):
    """Wino44::n32 (64- or 32-wide items, paths 9 / 11) over a lattice of 3x3 stride-1 layers, both modes: wherever the plan
    takes F(4x4,3x3) the restatement names the family of the path number, and the raw-box width is the map's."""
    path = built.raw('contrad_conv2d_path')
    took = set()
    for H in (4, 8, 16, 32, 64):
        for N in (1, 16, 94, 192, 229, 373, 383, 1493, 1536, 5977):
            for cin in (32, 64):
                for cout in (32, 64, 96, 128, 160, 192, 512):
                    for mode in (0, 1):
                        C, K = (cin, cout) if mode == 0 else (cout, cin)
                        d = ops.make_desc(N, H, H, C, K, 3, 3, 1, 1, C, K, K)
                        P = path(ctypes.byref(d), mode)
                        if P not in (9, 11):
                            continue
                        inst = KL.wino_instance((N, H, H, C, K, 3, 1, 1), mode)
                        bw = {4: 6, 8: 10, 16: 18}.get(H, 34)
                        assert inst == '%s_kernel<%d, %d>' % ('wino44::wino44' if P == 9 else 'wino44n::wino44n', mode, bw), (N, H, C, K, mode)
                        took.add(inst)
    assert took == {i for i in KL.LEDGER if i.startswith(('wino44::wino44_kernel<', 'wino44n::wino44n_kernel<'))}


def test_the_restated_mover_pieces_follow_the_output_grid():
    """nraw of Wino22::launch / Wino23::launch: grids of 16 / 8 / 4 give 5 / 6 / 7 (the non-square 16 x 8 grid: 5)."""
    for G, n in ((16, 5), (8, 6), (4, 7)):
        for mode in (0, 1):
            assert KL.wino_instance((3, 2 * G, 2 * G, 64, 64, 4, 2, 1), mode) == 'wino22::wino22_kernel<%d, %d>' % (mode, n)
        assert KL.wino_instance((3, 2 * G + 1, 2 * G + 1, 64, 64, 3, 2, 0), 0) == 'wino23::wino23_kernel<%d>' % n
    assert KL.wino_instance((3, 32, 16, 64, 64, 4, 2, 1), 0) == 'wino22::wino22_kernel<0, 5>'       # 4 x 9 x 17 x 2 / 256 = 4.8
    assert KL.wino_instance((3, 65, 65, 64, 64, 3, 2, 0), 0) == 'wino23::wino23_kernel<5>'          # patches of 8 x 16 tiles
    assert KL.wino_instance((3, 33, 33, 64, 64, 3, 2, 0), 1) is None                               # (forward only)
