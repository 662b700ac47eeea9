"""Dev tool: do the three existing kinds of the sum kernel (csrc/kid.hip: kid_sums_kernel behind contrad_kid_sums,
contrad_mmd_sums kind 1 and contrad_dot_sums) pay for the Gaussian kind that contrad_gauss_sums added?  This build against
the parent build, both libraries loaded side by side in one process; the protocol of tools/ab_cddls_recover.py.  Behind
profiles/contrast.txt.

    python tools/ab_kid_kinds.py PARENT.so PARENT_AGAIN.so [OUT.txt]

PARENT.so: the parent commit's library; PARENT_AGAIN.so: a copy of it under another name, so that the parent's own run-to-run
spread is on record.  HIP-event time around one call (two launches); per run the median of 20 calls after 3 warm-up calls;
7 runs per build, the builds alternating.  Shapes of tools/bench_kid.py: (1000, 1000) and (4096, 50 000).  Gate per entry
point and shape: this build's median inside (or below) the parent's min - max over its 14 runs, and outputs bitwise equal
to the parent's on the timed inputs.  Exit status 0 when every gate holds.  Last, contrad_gauss_sums of this build alone
at the same shapes (a record: the parent has no such entry point).
"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contrad_amd import _lib as L  # noqa: E402
from contrad_amd import ops  # noqa: E402

LL, VP, CI, CD = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_double
PROTOS = {
    'contrad_kid_sums_workspace_bytes': (LL, [CI, CI]),
    'contrad_kid_sums': (CI, [VP, LL, CI, CI, LL, CD, CD, CI, VP, VP, LL, VP]),
    'contrad_mmd_sums': (CI, [VP, LL, CI, CI, LL, CI, CD, CD, CI, VP, VP, LL, VP]),
    'contrad_dot_sums': (CI, [VP, LL, VP, LL, CI, CI, CI, VP, VP, LL, VP]),
}


def entries(path):
    """The existing entry points of the library at ``path`` (the parent exports none of this tree's newer symbols, so it is
    not loaded through _lib._Lib)."""
    dll, out = ctypes.CDLL(path), {}
    for name, (ret, proto) in PROTOS.items():
        f = getattr(dll, name)
        f.restype, f.argtypes = ret, proto
        out[name] = f
    return out


BUILDS = [('parent commit', os.path.abspath(sys.argv[1])),
          ('this build', L.LIB_PATH),
          ('parent commit again (second file)', os.path.abspath(sys.argv[2]))]
dev = torch.device('cuda', 0)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def one_run(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def show(name, r):
    emit('  %-36s %s  median %8.1f  min %8.1f  max %8.1f' % (name, ' '.join('%8.1f' % x for x in r), statistics.median(r),
                                                          min(r), max(r)))


st, p = ops._stream(), ops._p
libs = [entries(path) for _, path in BUILDS]
emit('times in us; one MI355X, one process; the kinds of kid_sums_kernel that existed before the Gaussian kind')
all_ok = True
g = torch.Generator(device='cpu').manual_seed(0)
for M, n in ((1000, 1000), (4096, 50000)):
    S = torch.randn(M, n, generator=g).clamp_(-1, 1).to(dev)
    T = torch.randn(M, n, generator=g).to(dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    nbytes = libs[0]['contrad_kid_sums_workspace_bytes'](M, n)
    assert nbytes == libs[1]['contrad_kid_sums_workspace_bytes'](M, n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    tail = (0, p(out), p(ws), LL(nbytes), st)
    cases = [
        ('contrad_kid_sums', 'gamma = coef0 = 1, self0 0', lambda f: f(p(S), LL(n), M, n, LL(0), 1.0, 1.0, *tail)),
        ('contrad_mmd_sums', "kind 1 ('rq'), self0 0", lambda f: f(p(S), LL(n), M, n, LL(0), 1, 1.0, 1.0, *tail)),
        ('contrad_dot_sums', 'two operands', lambda f: f(p(S), LL(n), p(T), LL(n), M, n, *tail)),
    ]
    for name, what, call in cases:
        runs = [[] for _ in BUILDS]
        for _ in range(7):
            for b, lib in enumerate(libs):
                runs[b].append(one_run(lambda: call(lib[name])))
        results = []
        for lib in libs:
            out.fill_(-7.0)
            assert call(lib[name]) == 0
            torch.cuda.synchronize()
            results.append(out.clone())
        same = all(torch.equal(results[0].view(torch.uint8), r.view(torch.uint8)) for r in results[1:])
        emit('%s (%d, %d) %s: out %.17g' % (name, M, n, what, float(results[1])))
        for (bname, _), r in zip(BUILDS, runs):
            show(bname, r)
        parent, nm = runs[0] + runs[2], statistics.median(runs[1])
        ok = nm <= max(parent) and same
        all_ok = all_ok and ok
        emit('  parent min - max over its 14 runs %.1f - %.1f us; this build median %.1f us: %s; outputs bitwise equal: %s'
             % (min(parent), max(parent), nm, 'ACCEPT' if nm <= max(parent) else 'MISS by %.1f us' % (nm - max(parent)), same))
    gauss = L.lib().raw('contrad_gauss_sums')
    r = [one_run(lambda: gauss(p(S), LL(n), M, n, LL(0), 2.0, *tail)) for _ in range(7)]
    emit('contrad_gauss_sums (%d, %d) t = 2, self0 0 (this build alone; %d MB read once)' % (M, n, M * n * 4 // 1000000))
    show('this build', r)
    del S, T
emit('ALL ACCEPTED' if all_ok else 'SOME MISSED')
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])) or '.', exist_ok=True)
    with open(sys.argv[3], 'a') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if all_ok else 1)
