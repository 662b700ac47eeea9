"""Dev tool: what a Frechet-distance evaluation (contrad_amd/fd.py, csrc/kid.hip) costs.

    python tools/bench_fd.py [OUT.txt] [small]    # (n_r, n_f, d) = (10 000, 10 000, 8192) and, without `small`, (50 000, 10 000, 8192)

Times are HIP-event medians of 5 with the min - max spread, one process, one shape at a time: the whole call (normalise,
centre, the cross-similarity GEMM, 60 Newton-Schulz steps, one read), the same on normalised rows and the real state (what
``--prdc_fd`` adds to a hooked evaluation), and one step by its parts.  Yardstick: a step is two GEMMs of 2 p q^2 flops each
(p = max(n_r, n_f), q = min), held against the fp32 MFMA rate the similarity GEMMs of tools/bench_kid.py reach.  No
threshold: the commit before this tool could not compute the quantity.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import fd, features, ops  # noqa: E402

dev = torch.device('cuda', 0)


def shape(emit, n_r, n_f, d, n_iter=fd.N_ITER):
    g = torch.Generator(device='cpu').manual_seed(0)
    real = torch.randn(n_r, d, generator=g).relu_().to(dev)
    fake = (torch.randn(n_f, d, generator=g) + 0.05).relu_().to(dev)
    out = fd.fd(real, fake, n_iter)
    est = out['estimates']
    emit('fd n_r = %d, n_f = %d, d = %d, %d steps: %.6f = %.6f + %.6f + %.6f - 2 * %.6f; tail %.3e of the estimate, step 30 at %.3e below '
         'the last' % (n_r, n_f, d, n_iter, out['fd'], out['mean_term'], out['trace_real'], out['trace_fake'], out['cross_term'],
                       out['tail'] / est[-1], (est[-1] - est[min(29, n_iter - 1)]) / est[-1]))
    p, q = max(n_r, n_f), min(n_r, n_f)
    flops = 4.0 * p * q * q
    t = windows(lambda: fd.fd(real, fake, n_iter), iters=1, reps=5, warm=0)
    emit(fmt('fd: all (normalise, centre, M, %d steps, one read)' % n_iter, t, '  %.1f ms / step' % (t[0] / n_iter)))
    rows_r, rows_f = features.normalize_rows(real), features.normalize_rows(fake)
    state = fd.real_state_of(features.bank_of(rows_r), n_r)
    del real, fake
    t = windows(lambda: fd.fd(None, rows_f, n_iter, normalize=False, real_state=state), iters=1, reps=5, warm=0)
    emit(fmt('  on normalised rows and the real state: what --prdc_fd adds to a hooked evaluation', t))
    t = windows(lambda: fd.real_state_of(features.bank_of(rows_r), n_r), iters=1, reps=5, warm=1)
    emit(fmt('  the real state (bank, centring, trace), once per run', t))
    del state, rows_r, rows_f
    q_pad = ops.round_up(q, 4)
    M = torch.randn(p, q_pad, generator=g).mul_(1.0 / (p * q) ** 0.5).to(dev)
    M[:, q:] = 0
    X, Xn, XT = M.clone(), torch.empty_like(M), torch.empty(q, p, device=dev)
    G, H = torch.empty(q, q_pad, device=dev), torch.zeros(q_pad, q_pad, device=dev)
    cell = torch.zeros(1, dtype=torch.float64, device=dev)
    t = windows(lambda: (fd.newton_schulz_step(X, XT, G, H, Xn, q), ops.dot_sums(Xn, M, q, out=cell)), iters=1, reps=5, warm=1)
    emit(fmt('  one step on a resident X [%d][%d]: transpose, G, H, X H, estimate' % (p, q_pad), t,
             '  %5.1f TFLOP/s over its two GEMMs' % (flops / t[0] * 1e-9)))
    t = windows(lambda: XT.copy_(X[:, :q].t()), iters=1, reps=5, warm=1)
    emit(fmt('    the transposed copy', t))
    t = windows(lambda: fd.gemm_rows(XT, X, G), iters=1, reps=5, warm=1)
    emit(fmt('    G = X^T X (%d x %d x %d)' % (q, q_pad, p), t, '  %5.1f TFLOP/s' % (2.0 * p * q * q / t[0] * 1e-9)))
    t = windows(lambda: fd.gemm_rows(X, H, Xn), iters=1, reps=5, warm=1)
    emit(fmt('    X H (%d x %d x %d)' % (p, q_pad, q_pad), t, '  %5.1f TFLOP/s' % (2.0 * p * q * q / t[0] * 1e-9)))
    t = windows(lambda: ops.dot_sums(Xn, M, q, out=cell), iters=1, reps=5, warm=1)
    emit(fmt('    dot_sums(X, M): two reads of %d MB' % (p * q * 4 // 1000000), t, '  %6.0f GB/s' % (2.0 * p * q * 4 / t[0] * 1e-6)))


if __name__ == '__main__':
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    for n_r, n_f, d in ((10000, 10000, 8192),) + (() if 'small' in sys.argv[2:] else ((50000, 10000, 8192),)):
        shape(emit, n_r, n_f, d)
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])) or '.', exist_ok=True)
        with open(sys.argv[1], 'a') as f:
            f.write('\n'.join(lines) + '\n')
