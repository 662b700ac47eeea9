"""Dev tool: where the time of a kNN evaluation (contrad_amd/knn.py, csrc/knn.hip) goes.

    python tools/bench_knn.py select   [OUT.txt]   # contrad_knn_select alone at (M, 50 000, 200, 10), torch.topk beside it
    python tools/bench_knn.py accuracy [OUT.txt]   # knn_accuracy on synthetic_set 50 000 / 10 000, SNDCGAN features, by stage

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time.
The select kernel reads every row five times (four radix digits and the compaction): its compulsory traffic is
5 * M * n * 4 bytes.  M = 512 is one chunk of the classifier (102 MB, inside the 256 MB Infinity Cache); M = 2048 (410 MB)
does not fit: equal time per row at both sizes means the kernel is not limited by where S lives.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrad_amd import features, knn, lineval, ops
from contrad_amd.evaluate.gan import freeze
from contrad_amd.models.gan import get_architecture

dev = torch.device('cuda', 0)


def windows(fn, iters=20, reps=7, warm=3):
    """Median and (min, max) time per call in milliseconds over ``reps`` event-bracketed windows of ``iters`` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def fmt(name, t, extra=''):
    return '%-72s %9.3f ms  (min %.3f, max %.3f)%s' % (name, t[0], t[1], t[2], extra)


def select(emit):
    n, k, C = 50000, 200, 10
    g = torch.Generator(device='cpu').manual_seed(0)
    labels = torch.randint(0, C, (n,), generator=g).to(dev)
    for M in (512, 2048):
        S = (torch.randn(M, n, generator=g) * 0.1).to(dev)
        nbytes = 5.0 * M * n * 4
        idx, val, _, _ = ops.knn_select(S, n, labels, C, k, 10.0)
        tv, ti = torch.topk(S, k, dim=1)
        assert torch.equal(val, tv)                                # (random floats: no ties, the orders coincide)
        t = windows(lambda: ops.knn_select(S, n, labels, C, k, 10.0))
        emit(fmt('knn_select (%d, %d, %d, %d): select + vote' % (M, n, k, C), t,
                 '  %6.0f GB/s of 5 row reads, %.2f us / row' % (nbytes / t[0] * 1e-6, t[0] * 1e3 / M)))
        t = windows(lambda: torch.topk(S, k, dim=1))
        emit(fmt('torch.topk(S, %d) on the same (%d, %d) S: values + indices only' % (k, M, n), t))
        del S


def accuracy(emit):
    data = lineval.synthetic_set(0, 10, 50000, 10000)
    torch.manual_seed(0)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    D = freeze(D.to(dev))
    data = knn.to_device(data, 10, dev)
    t = windows(lambda: knn.knn_accuracy(D, data, 10, 200, 0.1, 500), iters=1, reps=5, warm=1)
    emit(fmt('knn_accuracy 50 000 / 10 000, sndcgan (d = 8192), k 200, batch 500: all', t))
    bankT = features.new_bank(50000, D.d_penul, dev)
    t = windows(lambda: (features.extract_features(D, data['x_train'], 500, bankT=bankT),
                         features.extract_features(D, data['x_test'], 500)), iters=1, reps=5, warm=1)
    emit(fmt('  features: 60 000 eval-mode trunk forwards, normalise, bank transpose', t))
    q = features.extract_features(D, data['x_test'], 500)
    clf = knn.KNNClassifier(bankT, data['y_train'], 10, k=200, temp=0.1, normalize=False, transposed=True)
    t = windows(lambda: clf.predict(q), iters=1, reps=5, warm=1)
    emit(fmt('  predict: %d chunks of %d rows, GEMM then select per chunk' % (-(-10000 // clf.chunk_rows), clf.chunk_rows), t))
    S = torch.empty(clf.chunk_rows, clf.n_pad, device=dev)
    chunks = [(i, min(clf.chunk_rows, 10000 - i)) for i in range(0, 10000, clf.chunk_rows)]

    def gemms():
        for _ in features.similarity_chunks(q, clf.bankT, S):
            pass

    def selects():
        for i, m in chunks:
            ops.knn_select(S[:m], clf.n, clf.labels, 10, 200, clf.inv_temp)
    t = windows(gemms, iters=1, reps=5, warm=1)
    emit(fmt('  the similarity GEMMs alone (10 000 x 50 000 x 8192)', t, '  %5.1f TFLOP/s' % (2 * 1e4 * 5e4 * 8192 / t[0] * 1e-9)))
    t = windows(selects, iters=1, reps=5, warm=1)
    emit(fmt('  the selects alone (every chunk on one resident S)', t))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'select'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'select': select, 'accuracy': accuracy}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
