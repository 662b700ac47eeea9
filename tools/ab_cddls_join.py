"""Dev tool: the join kernel of csrc/cddls.hip (cddls_feature_seed_kernel and its pooled-seed and join forms) against the
parent build's feature seed, both libraries loaded side by side in one process, and the two new forms against the HBM
stream of cddls_bn_relu_bwd_eval.  Behind profiles/cddls_snresnet18.txt; the protocol of tools/ab_simrow.py.

    python tools/ab_cddls_join.py PARENT.so PARENT_AGAIN.so [OUT.txt]

PARENT.so: the library of the commit to compare with (that commit's cddls.hip compiled and linked with this tree's other
objects); PARENT_AGAIN.so: a copy of it under another name, so that the parent's own run-to-run spread is on record.
HIP-event time around one call; per run the median of 20 calls after 3 warm-up calls; 7 runs per build, the builds
alternating.  Gates: (1) contrad_cddls_feature_seed at (500, 8192): this build's median inside the parent's min - max over
its 14 runs, outputs bitwise equal; (2) the join at 500 x 32 x 32 x 64 streams at least as many bytes per second as
contrad_cddls_bn_relu_bwd_eval at the same shape in its slowest run.  The two are also compared as times, and that line is
reported only: the join moves four tensors (two branch gradients and the activation in, one out) where the BatchNorm
backward moves three, so its time can lie inside the other's range only if it streams a third faster per byte.  Exit
status 0 when both gates hold.
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

LL = ctypes.c_longlong
SEED_PROTO = [ctypes.c_void_p] * 4 + [LL, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]


def seed_entry(path):
    """contrad_cddls_feature_seed of the library at ``path`` (the parent exports none of this tree's newer symbols, so it
    is not loaded through _lib._Lib)."""
    f = ctypes.CDLL(path).contrad_cddls_feature_seed
    f.restype, f.argtypes = ctypes.c_int, SEED_PROTO
    return f


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


def show(name, r, nbytes=None):
    rate = '' if nbytes is None else '  %.2f TB/s' % (nbytes / statistics.median(r) / 1e6)
    emit('  %-36s %s  median %8.1f  min %8.1f  max %8.1f%s' % (name, ' '.join('%8.1f' % x for x in r), statistics.median(r),
                                                           min(r), max(r), rate))


g = torch.Generator().manual_seed(0)
st = ops._stream()
emit('times in us; one MI355X, one process')

# (1) the existing form at the sampler's own shape, three builds alternating
N, F = 500, 8192
gh, act = torch.randn(N, F, generator=g).to(dev), torch.randn(N, F, generator=g).to(dev)
c, out = torch.randn(F, generator=g).to(dev), torch.empty(N, F, device=dev)
entries = [seed_entry(p) for _, p in BUILDS]
calls = [(lambda f=f: f(ops._p(gh), ops._p(c), ops._p(act), ops._p(out), LL(N), F, 0.1, st)) for f in entries]
runs = [[] for _ in BUILDS]
for _ in range(7):
    for b, fn in enumerate(calls):
        runs[b].append(one_run(fn))
results = []
for fn in calls:
    out.fill_(-7)
    assert fn() == 0
    torch.cuda.synchronize()
    results.append(out.clone())
same = all(torch.equal(results[0].view(torch.uint8), r.view(torch.uint8)) for r in results[1:])
emit('contrad_cddls_feature_seed (%d, %d): reads 2 x %.1f MB, writes %.1f MB' % (N, F, N * F * 4e-6, N * F * 4e-6))
for (name, _), r in zip(BUILDS, runs):
    show(name, r, 3 * N * F * 4)
parent = runs[0] + runs[2]
nm = statistics.median(runs[1])
ok_seed = nm <= max(parent)                       # inside the parent's range, or below it
emit('  parent min - max over its 14 runs %.1f - %.1f us; this build median %.1f us: %s; outputs bitwise equal: %s'
     % (min(parent), max(parent), nm, 'ACCEPT' if ok_seed else 'MISS', same))

# (2) the new forms of this build next to the BatchNorm backward stream, alternating
shape = (500, 32, 32, 64)
n_big = 500 * 32 * 32 * 64
a_big, b_big, x_big, o_big = (torch.randn(n_big, generator=g).to(dev) for _ in range(4))
gamma, var = torch.rand(64, generator=g).to(dev) + 0.5, torch.rand(64, generator=g).to(dev) + 0.5
n_small = 500 * 4 * 4 * 512
a_s, b_s, x_s, o_s = (t[:n_small] for t in (a_big, b_big, x_big, o_big))
gp, cp = torch.randn(500, 512, generator=g).to(dev), torch.randn(512, generator=g).to(dev)
cases = [
    ('cddls_bn_relu_bwd_eval 512000 x 64 (largest call of a step)', 3 * n_big * 4,
     lambda: ops.bn_relu_bwd_eval(a_big.view(-1, 64), x_big.view(-1, 64), o_big.view(-1, 64), gamma, var)),
    # the join reads THREE tensors (both branch gradients and the activation) and writes one
    ('cddls_join_bwd 500 x 32 x 32 x 64', 4 * n_big * 4, lambda: ops.cddls_join_bwd(a_big, b_big, x_big, 0.1, out=o_big)),
    ('cddls_join_bwd 500 x 4 x 4 x 512', 4 * n_small * 4, lambda: ops.cddls_join_bwd(a_s, b_s, x_s, 0.1, out=o_s)),
    ('cddls_pooled_seed (500, 16, 512)', 2 * n_small * 4 + 500 * 512 * 4,
     lambda: ops.cddls_pooled_seed(gp, cp, x_s, 0.1, out=o_s)),
]
runs2 = [[] for _ in cases]
for _ in range(7):
    for i, (_, _, fn) in enumerate(cases):
        runs2[i].append(one_run(fn))
emit('this build, the streaming forms (bytes moved / median):')
for (name, nbytes, _), r in zip(cases, runs2):
    show(name, r, nbytes)
jm = statistics.median(runs2[1])
emit('  as times (reported, not part of the exit status): large join median %.1f us against the BatchNorm backward min - max '
     '%.1f - %.1f us: %s' % (jm, min(runs2[0]), max(runs2[0]), 'inside' if jm <= max(runs2[0]) else 'NOT inside'))
# like for like: bytes per second of the join's median against the slowest run of the BatchNorm backward
rate_join, rate_bn = cases[1][1] / jm / 1e6, cases[0][1] / max(runs2[0]) / 1e6
ok_join = rate_join >= rate_bn
emit('  per byte: large join %.2f TB/s against the BatchNorm backward at its slowest run %.2f TB/s: %s'
     % (rate_join, rate_bn, 'ACCEPT' if ok_join else 'MISS'))
all_ok = ok_seed and same and ok_join
emit('ALL ACCEPTED' if all_ok else 'SOME MISSED')
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])) or '.', exist_ok=True)
    with open(sys.argv[3], 'a') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if all_ok else 1)
