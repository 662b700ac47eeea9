"""Dev tool: do the Langevin forms of the three cDDLS kernels that gained a recovery form (csrc/cddls.hip:
cddls_energy_kernel, cddls_image_end_kernel, cddls_latent_update_kernel) pay for it?  This build against the parent
build, both libraries loaded side by side in one process; the protocol of tools/ab_cddls_join.py.  Behind
profiles/recover.txt.

    python tools/ab_cddls_recover.py PARENT.so PARENT_AGAIN.so [OUT.txt]

PARENT.so: the parent commit's cddls.hip compiled and linked with this tree's other objects; PARENT_AGAIN.so: a copy of it
under another name, so that the parent's own run-to-run spread is on record.  HIP-event time around one call; per run the
median of 20 calls after 3 warm-up calls; 7 runs per build, the builds alternating.  Shapes of tools/bench_cddls.py (batch
500, 32 x 32, sndcgan).  Gate per entry point: this build's median inside (or below) the parent's min - max over its 14
runs, and outputs bitwise equal to the parent's on the timed inputs.  Exit status 0 when every gate holds.
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

LL, VP, CI, CF = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
PROTOS = {
    'contrad_cddls_energy': [VP, CI, VP, VP, VP, VP, VP, CI, CI, LL, VP],
    'contrad_cddls_image_end': [VP, VP, VP, VP, LL, CF, CF, VP, LL, VP, VP],
    'contrad_cddls_latent_update': [VP, VP, LL, CF, CF, VP, LL, VP, VP],
}


def entries(path):
    """The three existing entry points of the library at ``path`` (the parent exports none of this tree's newer symbols, so
    it is not loaded through _lib._Lib)."""
    dll, out = ctypes.CDLL(path), {}
    for name, proto in PROTOS.items():
        f = getattr(dll, name)
        f.restype, f.argtypes = ctypes.c_int, proto
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


g = torch.Generator().manual_seed(0)
st = ops._stream()
p = ops._p
N, F, P, NZ = 500, 8192, 3 * 32 * 32, 128
EPS, SIGMA, SEED = 0.01, 0.1, 7
d, feat, c_row = torch.randn(N, 1, generator=g).to(dev), torch.randn(N, F, generator=g).relu().to(dev), torch.randn(F, generator=g).to(dev)
bias, e = torch.randn(1, generator=g).to(dev), torch.empty(N, device=dev)
gx, gout = torch.randn(N * P, generator=g).to(dev), torch.rand(N * P, generator=g).to(dev)
z2_0, z_0, gz = torch.randn(N * P, generator=g).to(dev), (torch.rand(N * NZ, generator=g) * 2 - 1).to(dev), torch.randn(N * NZ, generator=g).to(dev)
z2, z, g_lin = z2_0.clone(), z_0.clone(), torch.empty(N * P, device=dev)
state = torch.zeros(4, dtype=torch.int32, device=dev)


def reset():
    z2.copy_(z2_0); z.copy_(z_0); state.zero_(); e.fill_(-7); g_lin.fill_(-7)


CASES = [
    ('contrad_cddls_energy', '(500, F 8192, P 3072)',
     lambda f: f(p(d), 1, p(feat), p(c_row), p(bias), p(z2_0), p(e), N, F, LL(P), st), lambda: (e,)),
    ('contrad_cddls_image_end', '500 x 3072, generator noise',
     lambda f: f(p(gx), p(gout), p(z2), p(g_lin), LL(N * P), EPS, SIGMA, None, LL(SEED), p(state), st), lambda: (g_lin, z2)),
    ('contrad_cddls_latent_update', '500 x 128, generator noise',
     lambda f: f(p(z), p(gz), LL(N * NZ), EPS, SIGMA, None, LL(SEED), p(state), st), lambda: (z, state)),
]
libs = [entries(path) for _, path in BUILDS]
emit('times in us; one MI355X, one process; the Langevin forms of the kernels that gained a recovery form')
all_ok = True
for name, what, call, outs in CASES:
    runs = [[] for _ in BUILDS]
    for _ in range(7):
        for b, lib in enumerate(libs):
            reset()
            runs[b].append(one_run(lambda: call(lib[name])))
    results = []
    for lib in libs:
        reset()
        assert call(lib[name]) == 0
        torch.cuda.synchronize()
        results.append([t.clone() for t in outs()])
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for r in results[1:] for a, b in zip(results[0], r))
    emit('%s %s' % (name, what))
    for (bname, _), r in zip(BUILDS, runs):
        show(bname, r)
    parent, nm = runs[0] + runs[2], statistics.median(runs[1])
    ok = nm <= max(parent) and same
    all_ok = all_ok and ok
    emit('  parent min - max over its 14 runs %.1f - %.1f us; this build median %.1f us: %s; outputs bitwise equal: %s'
         % (min(parent), max(parent), nm, 'ACCEPT' if nm <= max(parent) else 'MISS', same))
emit('ALL ACCEPTED' if all_ok else 'SOME MISSED')
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])) or '.', exist_ok=True)
    with open(sys.argv[3], 'a') as f:
        f.write('\n'.join(lines) + '\n')
sys.exit(0 if all_ok else 1)
