"""Dev tool: the similarity-matrix kernels (csrc/simrow.h under knn.hip, prdc.hip, kid.hip) of this tree's library against
another build's, both loaded side by side in one process.  Behind profiles/simrow.txt.

    python tools/ab_simrow.py PARENT.so PARENT_AGAIN.so [OUT.txt]
    python tools/ab_simrow.py PARENT.so PARENT_AGAIN.so OUT.txt kid    # contrad_mmd_sums alone, at tools/bench_kid.py's shapes (profiles/fd.txt)

PARENT.so: the library of the commit to compare with (the three sources of that commit compiled and linked with this tree's
other objects, or a second checkout's library); PARENT_AGAIN.so: a copy of it under another name, so that the parent's own
run-to-run spread is part of the record.  HIP-event time around one call of the entry point; per run the median of 20 calls
after 3 warm-up calls; 7 runs per build, the builds alternating (parent, this build, parent again).  A kernel is accepted when
this build's median is at most the parent's median plus the parent's spread (max - min over its 14 runs); the outputs of all
builds on the timed inputs must be bitwise equal.  Exit status 0 exactly when every kernel is accepted.
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

BUILDS = [('parent commit', os.path.abspath(sys.argv[1])),
          ('this build', os.path.join(ROOT, 'contrad_amd', 'csrc', 'libcontrad_hip.so')),
          ('parent commit again (second file)', os.path.abspath(sys.argv[2]))]
libs = []
for name, path in BUILDS:
    L.LIB_PATH = path
    libs.append(L._Lib())
dev = torch.device('cuda', 0)
LL = ctypes.c_longlong
lines = []
KID_ONLY = len(sys.argv) > 4 and sys.argv[4] == 'kid'


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


def ab(title, make_call, outputs):
    """make_call(lib) -> a function of no arguments that launches once and writes `outputs` (tensors)."""
    if KID_ONLY and not title.startswith('mmd_sums'):
        return True
    calls = [make_call(lb) for lb in libs]
    runs = [[] for _ in libs]
    for _ in range(7):
        for b, fn in enumerate(calls):
            runs[b].append(one_run(fn))
    results = []
    for fn in calls:                                       # bitwise equality of what each build wrote on the timed input
        for t in outputs:
            t.fill_(-7)                                    # (the column counts of prdc_count are added to: the same start)
        fn()
        torch.cuda.synchronize()
        results.append([t.clone() for t in outputs])
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for r in results[1:] for a, b in zip(results[0], r))
    emit(title)
    for (name, _), r in zip(BUILDS, runs):
        emit('  %-36s %s  median %8.1f  min %8.1f  max %8.1f  range %5.1f' % (
            name, ' '.join('%8.1f' % x for x in r), statistics.median(r), min(r), max(r), max(r) - min(r)))
    parent = runs[0] + runs[2]
    pm, spread = statistics.median(parent), max(parent) - min(parent)
    nm = statistics.median(runs[1])
    ok = nm <= pm + spread
    emit('  parent median over its 14 runs %.1f us, spread (max - min) %.1f us; this build %.1f us: %s; outputs bitwise equal: %s'
         % (pm, spread, nm, 'ACCEPT' if ok else 'MISS', same))
    return ok and same


g = torch.Generator(device='cpu').manual_seed(0)
M, n = 512, 50000
S = (torch.randn(M, n, generator=g) * 0.1).to(dev)
S1 = torch.randn(4096 if KID_ONLY else M, n, generator=g).clamp_(-1, 1).to(dev)
Ssm = torch.randn(1000, 1000, generator=g).clamp_(-1, 1).to(dev)
labels = torch.randint(0, 10, (n,), generator=g).to(dev)
st = ops._stream()
all_ok = True
emit('times in us; one MI355X, one process; S = %d x %d unless stated' % (M, n))

# knn_select, k 200, C 10
k, C = 200, 10
idx = torch.empty((M, k), device=dev, dtype=torch.int32)
val = torch.empty((M, k), device=dev)
scores = torch.empty((M, C), device=dev)
pred = torch.empty((M,), device=dev, dtype=torch.int32)
for self0 in (-1, 0):
    def mk(lb, self0=self0):
        f = lb.raw('contrad_knn_select_loo')
        return lambda: f(ops._p(S), LL(n), M, n, LL(self0), ops._p(labels), C, k, 1.0, ops._as_int(idx), ops._p(val), ops._p(scores),
                         ops._as_int(pred), None, LL(0), st)
    all_ok &= ab('knn_select (contrad_knn_select_loo) k 200, C 10, self0 %d' % self0, mk, [idx, val, scores, pred])

# prdc_kth, k 5, self0 0
thr = torch.empty((M,), device=dev)


def mk_kth(lb):
    f = lb.raw('contrad_prdc_kth')
    return lambda: f(ops._p(S), LL(n), M, n, 5, LL(0), ops._p(thr), st)


all_ok &= ab('prdc_kth k 5, self0 0', mk_kth, [thr])

# prdc_count
t_row = ops.prdc_kth(S, n, 5)
t_col = ops.prdc_kth(S.t().contiguous(), M, 5)
rh = torch.empty(M, dtype=torch.int32, device=dev)
cc = torch.zeros(n, dtype=torch.int32, device=dev)
cr = torch.zeros(n, dtype=torch.int32, device=dev)
for title, tr_, tc_ in (('both thresholds', t_row, t_col), ('thr_col only', None, t_col), ('thr_row only', t_row, None)):
    def mk(lb, tr_=tr_, tc_=tc_):
        f = lb.raw('contrad_prdc_count')
        return lambda: f(ops._p(S), LL(n), M, n, ops._p(tr_), ops._p(tc_), ops._as_int(rh if tc_ is not None else None),
                         ops._as_int(cc if tc_ is not None else None), ops._as_int(cr if tr_ is not None else None), st)
    # the column arrays are added to: the equality check below starts each build from the same fill
    all_ok &= ab('prdc_count, %s' % title, mk, [rh, cc, cr])

# mmd_sums
out = torch.empty((1,), device=dev, dtype=torch.float64)
for X, name in ((Ssm, '1000 x 1000'), (S1, '%d x 50 000' % S1.shape[0])):
    m_, n_ = X.shape
    nbytes = libs[0].raw('contrad_kid_sums_workspace_bytes')(m_, n_)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for kind in (0, 1):
        def mk(lb, X=X, m_=m_, n_=n_, kind=kind, ws=ws, nbytes=nbytes):
            f = lb.raw('contrad_mmd_sums')
            return lambda: f(ops._p(X), LL(n_), m_, n_, LL(0), kind, 1.0 / 64, 1.0, 0, ops._p(out), ops._p(ws), LL(nbytes), st)
        all_ok &= ab('mmd_sums %s, kind %d, self0 0' % (name, kind), mk, [out])


# prdc_kth at the 10 000-column shape of tools/bench_prdc.py whole (chunks of 512 rows, a last chunk of 272)
for M, n in ((512, 10000), (272, 10000)):
    S = (torch.randn(M, n, generator=g) * 0.1).to(dev)
    thr = torch.empty((M,), device=dev)
    for self0 in (0, 9728, -1):
        def mk_kth(lb, S=S, M=M, n=n, thr=thr, self0=self0):
            f = lb.raw('contrad_prdc_kth')
            return lambda: f(ops._p(S), LL(n), M, n, 5, LL(self0), ops._p(thr), st)
        all_ok &= ab('prdc_kth %d x %d k 5, self0 %d' % (M, n, self0), mk_kth, [thr])
emit('ALL ACCEPTED' if all_ok else 'SOME MISSED')
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])) or '.', exist_ok=True)
    with open(sys.argv[3], 'a') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if all_ok else 1)
