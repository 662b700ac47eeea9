"""Dev tool: where the time of a kernel-distance evaluation (contrad_amd/kid.py, csrc/kid.hip) goes.

    python tools/bench_kid.py kernels [OUT.txt]   # contrad_kid_sums at (1000, 1000) and (4096, 50 000)
    python tools/bench_kid.py whole   [OUT.txt]   # kid at n_r = n_f = 10 000, d = 8192, 100 subsets of 1000, by stage
    python tools/bench_kid.py kernels|whole OUT.txt rq    # the same under the rational-quadratic kernel (default: poly3)

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time.
Yardstick: kid_sums reads M * n * 4 bytes once, held against 6.3 TB/s (the achievable HBM rate).
The (1000, 1000) block is 4 MB: it sits in the caches, just written by the GEMM in the real pipeline, and two launches
bound its time from below; (4096, 50 000) is 819 MB, beyond the Infinity Cache, so its rate is the one to hold against HBM.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import features, kid, ops  # noqa: E402

dev = torch.device('cuda', 0)
HBM = 6.3e12
KERNEL = sys.argv[3] if len(sys.argv) > 3 else 'poly3'
kid.check_kernel_name(KERNEL)


def sums_of(S, n, **kw):
    """The sum launches of KERNEL: contrad_kid_sums for poly3 (the path kid.py takes), contrad_mmd_sums otherwise."""
    return ops.kid_sums(S, n, **kw) if KERNEL == 'poly3' else ops.mmd_sums(S, n, KERNEL, **kw)


def kernels(emit):
    g = torch.Generator(device='cpu').manual_seed(0)
    for M, n in ((1000, 1000), (4096, 50000)):
        S = torch.randn(M, n, generator=g).clamp_(-1, 1).to(dev)
        out = sums_of(S, n, self0=0)
        if KERNEL == 'poly3':
            term = lambda s: (s + 1.0) ** 3
        else:
            term = lambda s: sum((1.0 + (2.0 - 2.0 * s).clamp_(min=0.0) / (2 * a)) ** -a for a in (0.5, 1.0, 2.0))
        ref = term(S.double()).sum() - term(S.double().diagonal()).sum()
        assert abs(float(out) - float(ref)) <= 1e-9 * float(ref), (float(out), float(ref))
        t = windows(lambda: sums_of(S, n, self0=0, out=out))
        bound_ms = M * n * 4 / HBM * 1e3
        emit(fmt('kid_sums %s(%d, %d), self0 = 0: two launches' % ('' if KERNEL == 'poly3' else KERNEL + ' ', M, n), t,
                 '  %6.0f GB/s of one read of S, %.2f of its read bound (%.4f ms)' % (M * n * 4 / t[0] * 1e-6, bound_ms / t[0], bound_ms)))
        del S


def whole(emit):
    n, d, T, size = 10000, 8192, 100, 1000
    g = torch.Generator(device='cpu').manual_seed(0)
    real = torch.randn(n, d, generator=g).to(dev)
    fake = (torch.randn(n, d, generator=g) + 0.05).to(dev)
    out = kid.kid(real, fake, T, size, kernel=KERNEL)
    emit('kid n_r = n_f = %d, d = %d, %d subsets of %d: %.6f +- %.6f' % (n, d, T, size, out['kid'], out['kid_std']))
    t = windows(lambda: kid.kid(real, fake, T, size, kernel=KERNEL), iters=1, reps=5, warm=1)
    emit(fmt('kid: all (normalise, %d x (gathers, three %d x %d x %d GEMMs, sums), one read)' % (T, size, size, d), t))
    rows_r, rows_f = features.normalize_rows(real), features.normalize_rows(fake)
    bank = features.bank_of(rows_r)
    t = windows(lambda: kid.kid(None, rows_f, T, size, normalize=False, real_bank=(bank, n), kernel=KERNEL), iters=1, reps=5, warm=1)
    emit(fmt('  on normalised rows and the real bank: what --prdc_kid adds to a hooked evaluation', t))
    idx = torch.randperm(n, generator=g)[:size].to(dev)
    R_t, F_t, bank_R, bank_F = kid.gather_subset(rows_r, None, rows_f, idx, idx)
    m_pad = bank_R.shape[1]
    S = torch.empty(min(features.chunk_rows_of(m_pad), size), m_pad, device=dev)
    table = torch.zeros(3, dtype=torch.float64, device=dev)

    def gemms():
        for q, b in ((R_t, bank_R), (F_t, bank_F), (F_t, bank_R)):
            for _ in features.similarity_chunks(q, b, S):
                pass

    def sums():
        for c, s0 in ((0, 0), (1, 0), (2, -1)):
            for i in range(0, size, S.shape[0]):
                r = min(S.shape[0], size - i)
                sums_of(S[:r], size, self0=s0 + i if s0 >= 0 else -1, out=table[c:c + 1], accumulate=i > 0)
    t = windows(gemms, iters=T, reps=5, warm=1)
    emit(fmt('  the three GEMMs of one subset alone (%d-row chunks), per subset' % S.shape[0], t,
             '  x %d = %.1f ms, %5.1f TFLOP/s' % (T, T * t[0], 3 * 2.0 * size * size * d / t[0] * 1e-9)))
    t = windows(sums, iters=T, reps=5, warm=1)
    emit(fmt('  the kid_sums launches of one subset alone (on one resident S), per subset', t, '  x %d = %.1f ms' % (T, T * t[0])))
    t = windows(lambda: kid.gather_subset(rows_r, None, rows_f, idx, idx), iters=T, reps=5, warm=1)
    emit(fmt('  the gathers and banks of one subset alone, per subset', t, '  x %d = %.1f ms' % (T, T * t[0])))
    t = windows(lambda: kid.gather_subset(None, bank, rows_f, idx, idx), iters=T, reps=5, warm=1)
    emit(fmt('  -- with the real rows taken from the transposed bank (the hook)', t, '  x %d = %.1f ms' % (T, T * t[0])))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'kernels': kernels, 'whole': whole}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
