"""The eval ledger (tests/eval_ledger.py) against the built object files of csrc/eval/ and the record
profiles/eval_ledger.txt.  No GPU.

* the kernel instances in csrc/eval/*.o are exactly the ledger's lines;
* every line names test_swd_kernels_gpu, a parity module for the kernel's source;
* the record has a non-zero dispatch count for every (instance, module) pair the ledger claims;
* the eval objects are linked into both libraries and stay out of the instance set that tests/kernel_ledger.py pins.
"""
import os
import subprocess

import pytest

import eval_ledger as EL
import kernel_ledger as KL
from contrad_amd import _lib, build


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_lib.LIB_PATH) or not all(os.path.exists(o) for o in EL.eval_objects()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def compiled(built):
    return EL.instance_sources()


def test_eval_objects_are_the_sources_build_compiles():
    assert [o[:-2] + '.hip' for o in EL.eval_objects()] == build.eval_sources()
    assert [os.path.basename(o) for o in EL.eval_objects()] == ['swd.o']
    assert not set(EL.eval_objects()) & set(KL.shipped_objects())


def test_compiled_instances_are_the_ledger(compiled):
    assert not set(EL.LEDGER) & set(EL.UNCOVERED) and EL.UNCOVERED == {}
    have = set(compiled)
    assert have - set(EL.LEDGER) == set(), 'compiled instances without a ledger line'
    assert set(EL.LEDGER) - have == set(), 'ledger lines for kernels the build no longer has'
    assert not have & KL.compiled_instances()                      # the other ledger's set is what it was


def test_ledger_lines_name_the_parity_module(compiled):
    for m, (sources, why) in EL.PARITY_MODULES.items():
        assert os.path.exists(os.path.join(EL.ROOT, 'tests', m + '.py')), m
        assert why and sources and all(os.path.exists(os.path.join(EL.CSRC, s + '.hip')) for s in sources), m
    for inst, modules in EL.LEDGER.items():
        assert modules == ['test_swd_kernels_gpu'], inst
        assert EL.credited(modules[0], compiled[inst]), inst


def test_the_record_agrees_with_the_ledger(compiled):
    rec = EL.read_record()
    assert set(rec) == set(compiled)
    for inst, modules in EL.LEDGER.items():
        for m in modules:
            got = rec[inst].get(m)
            assert isinstance(got, int) and got > 0, (inst, m, got)
    for inst in rec:
        assert all(m in EL.PARITY_MODULES for m in rec[inst]), inst


def test_both_libraries_hold_the_entry_points(built):
    names = [n for n in built.protos if n.startswith('contrad_swd_')]
    assert len(names) == 9
    for lib in (build.LIB, build.DEV_LIB):
        out = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(names) <= have, lib
