"""Float64 statement of the memorisation check (contrad_amd/nearest.py) in plain numpy (no project kernels): the neighbour
order with the row's own column left out, the nearest other real of every real, the nearest real of every fake, the
authenticity verdicts, the rows a float32 evaluation may legitimately decide otherwise, the leave-one-out vote and the
choice of the retrieved fakes.  The yardstick of tests/test_nearest_gpu.py, tied to a brute-force loop by
tests/test_nearest_ref64_cpu.py.

The order of the neighbours is contrad_knn_select's: value descending, then column ascending; -0.0 and +0.0 compare equal;
NaN compares below every number.  Row i of S is global row self0 + i and leaves that column out when self0 >= 0 and the
column exists -- by index, whatever it holds."""
import numpy as np


def normalize64(x):
    """x / max(||x||_2, 1e-12) per row, in float64."""
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def select_loo(S, k, self0=-1):
    """idx[M, k] (int64): per row i of S (any float dtype, compared exactly) the first k entries of the list of candidate
    columns -- every column but self0 + i -- sorted by (value descending with -0.0 == +0.0 and NaN last, column ascending)."""
    S = np.asarray(S)
    M, n = S.shape
    out = np.empty((M, k), np.int64)
    for i in range(M):
        e = self0 + i if self0 >= 0 else -1
        cand = np.array([j for j in range(n) if j != e], np.int64)
        assert 1 <= k <= len(cand), (k, len(cand))
        v = S[i, cand]
        nan = np.isnan(v)
        v = np.where(nan, 0, np.where(v == 0, 0, v))                  # -0.0 -> +0.0; a NaN's place is decided by the flag
        order = np.lexsort((cand, -v, nan))                           # last key first: numbers before NaN, value, column
        out[i] = cand[order[:k]]
    return out


def select_and_vote_loo(S, labels, C, k, inv_temp, self0=-1):
    """The contract of contrad_knn_select_loo on a given S[M, n]: (idx, val, scores64, pred); val keeps S's dtype and bits.
    scores[i][c] = sum of exp(val * inv_temp) over the neighbours with label c (a label outside [0, C) votes for nobody);
    pred: the largest score, NaN below every number, the lowest class on a tie."""
    S, labels = np.asarray(S), np.asarray(labels)
    idx = select_loo(S, k, self0)
    val = np.take_along_axis(S, idx, 1)
    w = np.exp(val.astype(np.float64) * float(inv_temp))
    scores = np.zeros((S.shape[0], C), np.float64)
    for i in range(S.shape[0]):
        for r in range(k):
            l = labels[idx[i, r]]
            if 0 <= l < C:
                scores[i, l] += w[i, r]
    pred = np.argmax(np.where(np.isnan(scores), -np.inf, scores), axis=1).astype(np.int64)
    return idx, val, scores, pred


def top_two_gap(S, self0=-1):
    """Per row the difference of its two best candidate values (inf where there is only one candidate)."""
    S = np.array(S, np.float64)
    if self0 >= 0:
        for i in range(S.shape[0]):
            if self0 + i < S.shape[1]:
                S[i, self0 + i] = -np.inf
    if S.shape[1] < 2:
        return np.full(S.shape[0], np.inf)
    top = -np.sort(-S, axis=1)[:, :2]
    return top[:, 0] - top[:, 1]


def authenticity_ref64(real, fake, gap=1e-5):
    """The float64 / exact-compare memorisation check of feature rows: dict of S_RR, S_FR (cosine similarities), nn1 and t1 of
    every real (self left out by index), i_star and s of every fake, the verdicts ``authentic`` (s < t1[i_star], strict),
    ``authenticity``, and the guard-rule masks ``fragile_real`` / ``fragile_fake`` of ``fragile``."""
    R, F = normalize64(real), normalize64(fake)
    S_RR, S_FR = R @ R.T, F @ R.T
    nn1 = select_loo(S_RR, 1, 0)[:, 0]
    t1 = S_RR[np.arange(len(R)), nn1]
    i_star = select_loo(S_FR, 1)[:, 0]
    s = S_FR[np.arange(len(F)), i_star]
    authentic = s < t1[i_star]
    fr, ff = fragile(S_RR, S_FR, t1, i_star, s, gap)
    return {'S_RR': S_RR, 'S_FR': S_FR, 'nn1': nn1, 't1': t1, 'i_star': i_star, 's': s, 'authentic': authentic,
            'authenticity': float(authentic.mean()), 'fragile_real': fr, 'fragile_fake': ff}


def fragile(S_RR, S_FR, t1, i_star, s, gap=1e-5):
    """(reals, fakes) whose result a float32 evaluation may legitimately change: a real whose two best similarities to other
    reals differ by less than ``gap`` (its nn1 may swap); a fake whose two best real similarities differ by less than
    ``gap`` (its i* may swap), or with |s - t1[i*]| < ``gap`` (its verdict may flip).  (A swapped nn1 moves t1 by no more than
    the rounding of a similarity: the largest of perturbed values is the perturbed largest value.)"""
    fr = top_two_gap(S_RR, 0) < gap
    ff = (top_two_gap(S_FR) < gap) | (np.abs(s - t1[i_star]) < gap)
    return fr, ff


def most_similar(s, rows):
    """The ``rows`` indices with the largest s, in that order, the lower index on a tie -- as a plain loop."""
    left, out = list(range(len(s))), []
    for _ in range(rows):
        best = left[0]
        for j in left[1:]:
            if s[j] > s[best]:
                best = j
        out.append(best)
        left.remove(best)
    return np.array(out, np.int64)
