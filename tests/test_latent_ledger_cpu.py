"""The latent ledger (tests/latent_ledger.py) against the built object files of csrc/latent/ and the record
profiles/latent_ledger.txt.  No GPU.

* the kernel instances in csrc/latent/*.o are exactly the ledger's lines;
* every line names test_latent_kernels_gpu, a parity module for the kernel's source;
* the record has a non-zero dispatch count for every (instance, module) pair the ledger claims;
* the latent objects are linked into both libraries and stay out of the instance sets that tests/kernel_ledger.py,
  tests/eval_ledger.py and tests/spectral_ledger.py pin.
"""
import os
import subprocess

import pytest

import eval_ledger as EL
import kernel_ledger as KL
import latent_ledger as LL
import spectral_ledger as SL
from contrad_amd import _lib, build


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_lib.LIB_PATH) or not all(os.path.exists(o) for o in LL.latent_objects() + SL.spectral_objects() + EL.eval_objects()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def compiled(built):
    return LL.instance_sources()


def test_latent_objects_are_the_sources_build_compiles():
    assert [o[:-2] + '.hip' for o in LL.latent_objects()] == build.latent_sources()
    assert [os.path.basename(o) for o in LL.latent_objects()] == ['latent.o']
    assert not set(LL.latent_objects()) & (set(KL.shipped_objects()) | set(EL.eval_objects()) | set(SL.spectral_objects()))
    assert not set(build.latent_sources()) & (set(build.eval_sources()) | set(build.spectral_sources()))


def test_compiled_instances_are_the_ledger(compiled):
    assert not set(LL.LEDGER) & set(LL.UNCOVERED) and LL.UNCOVERED == {}
    have = set(compiled)
    assert have - set(LL.LEDGER) == set(), 'compiled instances without a ledger line'
    assert set(LL.LEDGER) - have == set(), 'ledger lines for kernels the build no longer has'


def test_the_other_three_ledgers_are_untouched(compiled):
    have = set(compiled)
    assert not have & KL.compiled_instances() and not have & EL.compiled_instances() and not have & SL.compiled_instances()
    assert EL.compiled_instances() == set(EL.LEDGER)
    assert SL.compiled_instances() == set(SL.LEDGER)
    assert KL.compiled_instances() == set(KL.LEDGER) | set(KL.UNCOVERED)


def test_ledger_lines_name_the_parity_module(compiled):
    for m, (sources, why) in LL.PARITY_MODULES.items():
        assert os.path.exists(os.path.join(LL.ROOT, 'tests', m + '.py')), m
        assert why and sources and all(os.path.exists(os.path.join(LL.CSRC, s + '.hip')) for s in sources), m
    for inst, modules in LL.LEDGER.items():
        assert modules == ['test_latent_kernels_gpu'], inst
        assert LL.credited(modules[0], compiled[inst]), inst


def test_the_record_agrees_with_the_ledger(compiled):
    rec = LL.read_record()
    assert set(rec) == set(compiled)
    for inst, modules in LL.LEDGER.items():
        for m in modules:
            got = rec[inst].get(m)
            assert isinstance(got, int) and got > 0, (inst, m, got)
    for inst in rec:
        assert all(m in LL.PARITY_MODULES for m in rec[inst]), inst


def test_both_libraries_hold_the_entry_points(built):
    names = [n for n in built.protos if n.startswith('contrad_latent_') or n.startswith('contrad_pair_dist')]
    assert sorted(names) == ['contrad_latent_pair', 'contrad_latent_styles', 'contrad_pair_dist', 'contrad_pair_dist_resident_d']
    assert not [n for n in names if 'workspace' in n]                       # no scratch: no workspace query
    for lib in (build.LIB, build.DEV_LIB):
        out = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(names) <= have, lib
