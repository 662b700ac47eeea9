"""Float64 statement of the weighted kNN vote in plain numpy (no project kernels): normalise, similarities, the
neighbour order, weights exp(s / T), per-class sums, argmax.  The yardstick of tests/test_knn_gpu.py, tied to a
brute-force loop by tests/test_knn_ref64_cpu.py.

The order of the neighbours is total: value descending, then column ascending; -0.0 and +0.0 compare equal; NaN
compares below every number.  The predicted class is the largest score under the same order, the lowest class on a tie."""
import numpy as np


def normalize64(x):
    """x / max(||x||_2, 1e-12) per row (F.normalize), in float64."""
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def select(S, k):
    """idx[M, k]: per row of S (any float dtype, compared exactly) the first k columns of the neighbour order."""
    S = np.asarray(S)
    M, n = S.shape
    assert 1 <= k <= n
    v = np.where(S == 0, np.zeros((), S.dtype), S)        # -0.0 -> +0.0; NaN stays, and sorts last as -NaN
    cols = np.arange(n)
    return np.stack([np.lexsort((cols, -v[i]))[:k] for i in range(M)]).astype(np.int64)


def vote(val, nb_labels, C, inv_temp):
    """scores[M, C] (float64) of neighbour values val[M, k] with labels nb_labels[M, k]; a label outside [0, C) votes for
    nobody."""
    val = np.asarray(val, np.float64)
    w = np.exp(val * inv_temp)
    scores = np.zeros((val.shape[0], C), np.float64)
    for i in range(val.shape[0]):
        ok = (nb_labels[i] >= 0) & (nb_labels[i] < C)
        np.add.at(scores[i], nb_labels[i][ok], w[i][ok])
    return scores


def predict(scores):
    """The class of the largest score, NaN below every number, the lowest class on an exact tie."""
    return np.argmax(np.where(np.isnan(scores), -np.inf, scores), axis=1).astype(np.int64)


def select_and_vote(S, labels, C, k, inv_temp):
    """The contract of contrad_knn_select on a given S[M, n]: (idx, val, scores64, pred); val keeps S's dtype and bits."""
    S, labels = np.asarray(S), np.asarray(labels)
    idx = select(S, k)
    val = np.take_along_axis(S, idx, 1)
    scores = vote(val, labels[idx], C, float(inv_temp))
    return idx, val, scores, predict(scores)


def knn_ref64(bank, labels, q, C, k, T):
    """The classifier on features: dict of S (float64 cosine similarities [M, n]), k (clamped to n), idx, val, scores, pred."""
    S = normalize64(q) @ normalize64(bank).T
    k = min(int(k), S.shape[1])
    idx, val, scores, pred = select_and_vote(S, labels, C, k, 1.0 / T)
    return {'S': S, 'k': k, 'idx': idx, 'val': val, 'scores': scores, 'pred': pred}


def fragile_rows(S, scores, k, gap_s=1e-5, gap_score=1e-4):
    """Rows whose verdict a float32 evaluation may legitimately change: the k-th and (k+1)-th similarities differ by less
    than ``gap_s``, or the two best class scores by less than ``gap_score`` relative to the best."""
    srt = -np.sort(-np.asarray(S, np.float64), axis=1)
    out = np.zeros(S.shape[0], bool)
    if k < S.shape[1]:
        out |= (srt[:, k - 1] - srt[:, k]) < gap_s
    if scores.shape[1] > 1:
        top = -np.sort(-scores, axis=1)[:, :2]
        out |= (top[:, 0] - top[:, 1]) < gap_score * np.abs(top[:, 0])
    return out
