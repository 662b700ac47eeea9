"""Dev tool: where the time of a precision / recall / density / coverage evaluation (contrad_amd/prdc.py, csrc/prdc.hip) goes.

    python tools/bench_prdc.py kernels [OUT.txt]   # contrad_prdc_kth at (512, 50 000, 5), contrad_prdc_count at (512, 50 000)
    python tools/bench_prdc.py whole   [OUT.txt]   # prdc at n_r = n_f = 10 000, d = 8192, by stage

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time.
Yardsticks: prdc_count reads M * n * 4 bytes once (the HBM streaming bound); prdc_kth reads the row four times (one per
radix digit).  M = 512 is one chunk of prdc (102 MB, inside the 256 MB Infinity Cache, and just written by the GEMM in
the real pipeline); M = 4096 (819 MB) does not fit, so its rate is the one to hold against HBM.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import features, ops, prdc  # noqa: E402

dev = torch.device('cuda', 0)


def kernels(emit):
    n, k = 50000, 5
    g = torch.Generator(device='cpu').manual_seed(0)
    for M in (512, 4096):
        S = (torch.randn(M, n, generator=g) * 0.1).to(dev)
        thr = ops.prdc_kth(S, n, k)
        assert torch.equal(thr, torch.topk(S, k, dim=1)[0][:, k - 1])          # (random floats: no ties, no zeros, no NaN)
        t = windows(lambda: ops.prdc_kth(S, n, k, self0=-1, out=thr))
        emit(fmt('prdc_kth (%d, %d, %d)' % (M, n, k), t,
                 '  %6.0f GB/s of 4 row reads, %.2f us / row' % (4.0 * M * n * 4 / t[0] * 1e-6, t[0] * 1e3 / M)))
        t_col = ops.prdc_kth(S.t().contiguous(), M, k)      # a threshold per column, taken from the data
        t_row = ops.prdc_kth(S, n, k)
        cc = torch.zeros(n, dtype=torch.int32, device=dev)
        cr = torch.zeros(n, dtype=torch.int32, device=dev)
        rh = torch.empty(M, dtype=torch.int32, device=dev)
        for name, a in (('both thresholds', dict(thr_row=t_row, thr_col=t_col, row_hits=rh, col_hits_c=cc, col_hits_r=cr)),
                        ('thr_col only', dict(thr_col=t_col, row_hits=rh, col_hits_c=cc)),
                        ('thr_row only', dict(thr_row=t_row, col_hits_r=cr))):
            t = windows(lambda: ops.prdc_count(S, n, **a))
            emit(fmt('prdc_count (%d, %d), %s' % (M, n, name), t, '  %6.0f GB/s of one read of S' % (M * n * 4 / t[0] * 1e-6)))
        del S


def whole(emit):
    n, d, k = 10000, 8192, 5
    g = torch.Generator(device='cpu').manual_seed(0)
    real = torch.randn(n, d, generator=g).to(dev)
    fake = (torch.randn(n, d, generator=g) + 0.05).to(dev)
    t = windows(lambda: prdc.prdc(real, fake, k), iters=1, reps=5, warm=1)
    emit(fmt('prdc n_r = n_f = %d, d = %d, k = %d: all (three %d x %d x %d GEMMs)' % (n, d, k, n, n, d), t))
    state = prdc.real_state_of(real, k)
    t = windows(lambda: prdc.prdc(None, fake, k, real_state=state), iters=1, reps=5, warm=1)
    emit(fmt('  with the cached real state (two GEMMs): what the training hook pays per evaluation', t))
    rows = features.normalize_rows(fake)
    bankT = features.bank_of(rows)
    chunk = features.chunk_rows_of(bankT.shape[1])
    S = torch.empty(chunk, bankT.shape[1], device=dev)
    chunks = [(i, min(chunk, n - i)) for i in range(0, n, chunk)]
    thr = torch.empty(n, device=dev)
    cc = torch.zeros(n, dtype=torch.int32, device=dev)
    cr = torch.zeros(n, dtype=torch.int32, device=dev)
    rh = torch.empty(n, dtype=torch.int32, device=dev)

    def gemms():
        for _ in features.similarity_chunks(rows, bankT, S):
            pass

    def kths():
        for i, m in chunks:
            ops.prdc_kth(S[:m], n, k, self0=i, out=thr[i:i + m])

    def counts():
        for i, m in chunks:
            ops.prdc_count(S[:m], n, thr_row=thr[i:i + m], thr_col=thr, row_hits=rh[i:i + m], col_hits_c=cc, col_hits_r=cr)
    t = windows(gemms, iters=1, reps=5, warm=1)
    emit(fmt('  one similarity GEMM alone (%d chunks of %d rows)' % (len(chunks), chunk), t, '  %5.1f TFLOP/s' % (2.0 * n * n * d / t[0] * 1e-9)))
    t = windows(kths, iters=1, reps=5, warm=1)
    emit(fmt('  the prdc_kth launches of one set alone (every chunk on one resident S)', t))
    t = windows(counts, iters=1, reps=5, warm=1)
    emit(fmt('  the prdc_count launches alone (every chunk on one resident S)', t))


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
