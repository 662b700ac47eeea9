"""Dev tool: the training form of contrad_bn_relu_apply (bn_relu_apply_kernel, csrc/elementwise.hip) of this tree's library
against another build's, both loaded side by side in one process.  Behind the timing in profiles/bn_eval.txt.

    python tools/ab_bn_apply.py PARENT.so PARENT_AGAIN.so [OUT.txt]

PARENT.so: the library of the commit to compare with; PARENT_AGAIN.so: a copy of it under another name, so that the parent's
own run-to-run spread is part of the record.  Only the one entry point is bound, so a parent that lacks newer symbols loads.
Shapes: the BatchNorm layers of G_SNDCGAN at the benchmark batch of 512 (the largest is 524 288 x 64) and norm_init with its
column permutation.  HIP-event time around one call; per run the median of 20 calls after 3 warm-up calls; 7 runs per build,
the builds alternating (parent, this build, parent again).  A shape is accepted when this build's median is at most the
parent's median plus the parent's spread (max - min over its 14 runs); the outputs of all builds must be bitwise equal.
Exit status 0 exactly when every shape is accepted.
"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contrad_amd import ops  # noqa: E402

BUILDS = [('parent commit', os.path.abspath(sys.argv[1])),
          ('this build', os.path.join(ROOT, 'contrad_amd', 'csrc', 'libcontrad_hip.so')),
          ('parent commit again (second file)', os.path.abspath(sys.argv[2]))]
LL, VP, FL, IN = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float, ctypes.c_int
fns = []
for _, path in BUILDS:
    f = ctypes.CDLL(path).contrad_bn_relu_apply
    f.restype, f.argtypes = IN, [VP, VP, LL, IN, IN, IN, VP, FL, VP, VP, FL, IN, VP]
    fns.append(f)
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


emit('times in us; one MI355X, one process; contrad_bn_relu_apply, training form (count = M)')
all_ok = True
g = torch.Generator().manual_seed(0)
for M, K, perm in ((512 * 32 * 32, 64, 1), (512 * 16 * 16, 128, 1), (512 * 8 * 8, 256, 1), (512, 8192, 16)):
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(dev)
    y = torch.empty_like(x)
    gamma, beta = (torch.rand(K, generator=g) + 0.5).to(dev), (torch.randn(K, generator=g) * 0.3).to(dev)
    stats = ops.colstats(x, with_sq=True)
    st = ops._stream()
    calls = [(lambda f=f: f(ops._p(x), ops._p(y), LL(M), K, K, K, ops._p(stats), float(M), ops._p(gamma), ops._p(beta), 1e-5,
                            perm, st)) for f in fns]
    assert all(c() == 0 for c in calls)
    runs = [[] for _ in fns]
    for _ in range(7):
        for b, c in enumerate(calls):
            runs[b].append(one_run(c))
    results = []
    for c in calls:
        y.fill_(-7)
        c()
        torch.cuda.synchronize()
        results.append(y.clone())
    same = all(torch.equal(results[0].view(torch.int32), r.view(torch.int32)) for r in results[1:])
    emit('M %d, K %d, perm_hw %d' % (M, K, perm))
    for (name, _), r in zip(BUILDS, runs):
        emit('  %-36s %s  median %8.1f  min %8.1f  max %8.1f  range %5.1f' % (
            name, ' '.join('%8.1f' % t for t in r), statistics.median(r), min(r), max(r), max(r) - min(r)))
    parent = runs[0] + runs[2]
    pm, spread, nm = statistics.median(parent), max(parent) - min(parent), statistics.median(runs[1])
    inside = min(parent) <= nm <= max(parent)
    ok = nm <= pm + spread
    emit('  parent median over its 14 runs %.1f us, min %.1f, max %.1f; this build %.1f us: %s (%s the parent\'s min - max); '
         'outputs bitwise equal: %s' % (pm, min(parent), max(parent), nm, 'ACCEPT' if ok else 'MISS',
                                        'inside' if inside else 'outside', same))
    all_ok &= ok and same
emit('ALL ACCEPTED' if all_ok else 'SOME MISSED')
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])) or '.', exist_ok=True)
    with open(sys.argv[3], 'a') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if all_ok else 1)
