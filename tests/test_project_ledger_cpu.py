"""The project ledger (tests/project_ledger.py) against the built object files of csrc/project/ and the record
profiles/project_ledger.txt.  No GPU.

* the kernel instances in csrc/project/*.o are exactly the ledger's lines;
* every line names test_project_kernels_gpu, a parity module for the kernel's source;
* the record has a non-zero dispatch count for every (instance, module) pair the ledger claims;
* the project objects are linked into both libraries and stay out of the instance sets that the other four ledgers pin;
* both libraries export the four entry points, and none of them is a workspace query.
"""
import os
import subprocess

import pytest

import eval_ledger as EL
import kernel_ledger as KL
import latent_ledger as LL
import project_ledger as PL
import spectral_ledger as SL
from contrad_amd import _lib, build


@pytest.fixture(scope='module')
def built():
    objs = PL.project_objects() + LL.latent_objects() + SL.spectral_objects() + EL.eval_objects()
    if not os.path.exists(_lib.LIB_PATH) or not all(os.path.exists(o) for o in objs):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def compiled(built):
    return PL.instance_sources()


def test_project_objects_are_the_sources_build_compiles():
    assert [o[:-2] + '.hip' for o in PL.project_objects()] == build.project_sources()
    assert [os.path.basename(o) for o in PL.project_objects()] == ['project.o']
    others = set(KL.shipped_objects()) | set(EL.eval_objects()) | set(SL.spectral_objects()) | set(LL.latent_objects())
    assert not set(PL.project_objects()) & others
    assert not set(build.project_sources()) & (set(build.eval_sources()) | set(build.spectral_sources()) | set(build.latent_sources()))


def test_compiled_instances_are_the_ledger(compiled):
    assert not set(PL.LEDGER) & set(PL.UNCOVERED) and PL.UNCOVERED == {}
    have = set(compiled)
    assert have - set(PL.LEDGER) == set(), 'compiled instances without a ledger line'
    assert set(PL.LEDGER) - have == set(), 'ledger lines for kernels the build no longer has'


def test_the_other_four_ledgers_are_untouched(compiled):
    have = set(compiled)
    for other in (KL, EL, SL, LL):
        assert not have & other.compiled_instances(), other.__name__
    assert EL.compiled_instances() == set(EL.LEDGER)
    assert SL.compiled_instances() == set(SL.LEDGER)
    assert LL.compiled_instances() == set(LL.LEDGER)
    assert KL.compiled_instances() == set(KL.LEDGER) | set(KL.UNCOVERED)


def test_ledger_lines_name_the_parity_module(compiled):
    for m, (sources, why) in PL.PARITY_MODULES.items():
        assert os.path.exists(os.path.join(PL.ROOT, 'tests', m + '.py')), m
        assert why and sources and all(os.path.exists(os.path.join(PL.CSRC, s + '.hip')) for s in sources), m
    for inst, modules in PL.LEDGER.items():
        assert modules == ['test_project_kernels_gpu'], inst
        assert PL.credited(modules[0], compiled[inst]), inst


def test_the_record_agrees_with_the_ledger(compiled):
    rec = PL.read_record()
    assert set(rec) == set(compiled)
    for inst, modules in PL.LEDGER.items():
        for m in modules:
            got = rec[inst].get(m)
            assert isinstance(got, int) and got > 0, (inst, m, got)
    for inst in rec:
        assert all(m in PL.PARITY_MODULES for m in rec[inst]), inst


def test_both_libraries_hold_the_entry_points(built):
    names = [n for n in built.protos if n.startswith('contrad_proj_')]
    assert sorted(names) == ['contrad_proj_image_end', 'contrad_proj_noise_grad', 'contrad_proj_noise_normalize', 'contrad_proj_noise_reg']
    assert not [n for n in names if 'workspace' in n]                       # scratch is an argument: no workspace query
    for lib in (build.LIB, build.DEV_LIB):
        out = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(names) <= have, lib
