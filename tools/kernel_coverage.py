"""Which compiled kernel instance does which parity module launch?  Reads the rocprofv3 (rocpd sqlite) kernel traces of
the parity modules, one directory of databases named ``<module>_<pid>_results.db`` (a module whose cases run in child
processes leaves one database per process), and writes the record kept as profiles/kernel_ledger.txt: one line per compiled
instance (tests/kernel_ledger.py: compiled_instances), tab-separated -- the instance, then ``module=dispatches`` for every
module that launched it (and is a parity module for the kernel's source file), or NEVER.  Kernels in a trace that are not ours (torch's, rocBLAS's) match nothing in the compiled
set and are ignored.  No GPU.

    python tools/kernel_coverage.py TRACE_DIR [--out profiles/kernel_ledger.txt] [--ledger]
    python tools/kernel_coverage.py TRACE_DIR --counts-out DIR [--only MODULE]

The databases run to tens of megabytes per module.  --counts-out writes, where the databases are, one small
``<module>.counts.json`` per module ({kernel name as traced: dispatches}, summed over the module's processes) and stops;
TRACE_DIR may hold such files in place of (or beside) databases, and the record is then made from them where the object files are.

--ledger prints the LEDGER literal of the record (tests/kernel_ledger.py).
--eval does all of the above for the ledger of csrc/eval/*.hip instead (tests/eval_ledger.py, profiles/eval_ledger.txt).
--spectral does it for the ledger of csrc/spectral/*.hip (tests/spectral_ledger.py, profiles/spectral_ledger.txt).
--latent does it for the ledger of csrc/latent/*.hip (tests/latent_ledger.py, profiles/latent_ledger.txt).
--project does it for the ledger of csrc/project/*.hip (tests/project_ledger.py, profiles/project_ledger.txt).

Recording (on the GPU box, one step per parity module, kernel trace only, each under its own time limit):
    rocprofv3 --kernel-trace -f rocpd -d TRACE_DIR -o <module>_%pid% -- python -m pytest tests/<module>.py -q -m gpu
"""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import kernel_ledger as L  # noqa: E402


def raw_counts(path):
    """({kernel name as traced: dispatches}, processes) of one database (the ``kernels`` table tools/rocpd_summary.py reads;
    one process) or counts file."""
    if path.endswith('.json'):
        with open(path) as f:
            d = json.load(f)
        return d['kernels'], d['processes']
    db = sqlite3.connect(path)
    counts = dict(db.execute('select name, count(*) from kernels group by name').fetchall())
    db.close()
    return counts, 1


def module_of(path):
    m = re.match(r'(test_\w+?_gpu)(_\d+_results\.db|\.counts\.json)$', os.path.basename(path))
    return m.group(1) if m else None


def collect(trace_dir, modules, normalise=L.normalise):
    """({module: {kernel: dispatches}}, {module: traced processes}) over every database / counts file under trace_dir that
    belongs to one of ``modules``."""
    per, procs = {}, {}
    paths = glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True) + \
        glob.glob(os.path.join(trace_dir, '**', '*.counts.json'), recursive=True)
    for path in sorted(paths):
        m = module_of(path)
        if m not in modules:
            continue
        acc = per.setdefault(m, {})
        counts, np_ = raw_counts(path)
        procs[m] = procs.get(m, 0) + np_
        for name, n in counts.items():
            k = normalise(name)
            acc[k] = acc.get(k, 0) + n
    return per, procs


def main(argv=None):
    global L
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('trace_dir')
    ap.add_argument('--out', default=None, help='default: the ledger\'s own record')
    ap.add_argument('--ledger', action='store_true')
    ap.add_argument('--counts-out', metavar='DIR')
    ap.add_argument('--only', action='append', default=[], metavar='MODULE')
    ap.add_argument('--eval', action='store_true',
                    help='the ledger of csrc/eval/*.hip (tests/eval_ledger.py, profiles/eval_ledger.txt) in place of csrc/*.hip\'s')
    ap.add_argument('--spectral', action='store_true',
                    help='the ledger of csrc/spectral/*.hip (tests/spectral_ledger.py, profiles/spectral_ledger.txt)')
    ap.add_argument('--latent', action='store_true',
                    help='the ledger of csrc/latent/*.hip (tests/latent_ledger.py, profiles/latent_ledger.txt)')
    ap.add_argument('--project', action='store_true',
                    help='the ledger of csrc/project/*.hip (tests/project_ledger.py, profiles/project_ledger.txt)')
    a = ap.parse_args(argv)
    if a.eval + a.spectral + a.latent + a.project > 1:
        ap.error('--eval, --spectral, --latent and --project name four ledgers: one run writes one record')
    if a.eval:
        import eval_ledger
        L = eval_ledger
    if a.spectral:
        import spectral_ledger
        L = spectral_ledger
    if a.latent:
        import latent_ledger
        L = latent_ledger
    if a.project:
        import project_ledger
        L = project_ledger
    a.out = a.out or L.RECORD
    if a.counts_out:
        per, procs = collect(a.trace_dir, set(a.only or L.PARITY_MODULES), normalise=str)
        for m, counts in sorted(per.items()):
            with open(os.path.join(a.counts_out, m + '.counts.json'), 'w') as f:
                json.dump({'processes': procs[m], 'kernels': counts}, f, indent=0, sort_keys=True)
            print('%s: %d kernel names, %d dispatches, %d process(es)' % (m, len(counts), sum(counts.values()), procs[m]))
        return 0 if per else 1
    sources = L.instance_sources()
    compiled = sorted(sources)
    modules = list(L.PARITY_MODULES)
    per, procs = collect(a.trace_dir, set(modules))
    for m in per:                      # a module counts only for the sources it is a parity module of (kernel_ledger.PARITY_MODULES)
        per[m] = {k: n for k, n in per[m].items() if k in sources and L.credited(m, sources[k])}
    missing = [m for m in modules if m not in per]
    lines, never = [], 0
    for inst in compiled:
        hits = ['%s=%s' % (m, per[m][inst]) for m in modules if inst in per.get(m, {})]
        never += not hits
        lines.append('\t'.join([inst] + (hits or [L.NEVER])))
    with open(a.out, 'w') as f:
        f.write('# kernel ledger record: compiled instance <tab> parity module=dispatches ... | NEVER   (tools/kernel_coverage.py)\n')
        f.write('# %d compiled instances, %d parity modules traced, %d instances launched by none\n' % (len(compiled), len(per), never))
        for m in modules:              # (a module whose cases run in child processes: their dispatches are in the trace)
            if m in per:
                f.write('# %s: %d dispatches of %d instances in %d traced process(es)\n'
                        % (m, sum(per[m].values()), len(per[m]), procs[m]))
            else:
                f.write('# no trace of %s\n' % m)
        f.write('\n'.join(lines) + '\n')
    print('%d instances, %d NEVER, modules without a trace: %s -> %s' % (len(compiled), never, missing or 'none', a.out))
    if a.ledger:
        print('LEDGER = {')
        for inst in compiled:
            ms = [m for m in modules if inst in per.get(m, {})]
            if ms:
                print('    %r: [%s],' % (inst, ', '.join(repr(m) for m in ms)))
        print('}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
