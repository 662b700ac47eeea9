"""Float64 statement of precision / recall / density / coverage in similarity space, in plain numpy (no project
kernels), and the exact integer outputs of the two kernels of csrc/prdc.hip on a given float32 S.  The yardstick of
tests/test_prdc_gpu.py, tied to a brute-force double loop by tests/test_prdc_ref64_cpu.py.

With R the real rows, F the fake rows (both L2-normalised), S_XY = X Y^T:
    t_R[i] = k-th largest of S_RR[i][j], j != i;  t_F[j] = k-th largest of S_FF[j][l], l != j   (self left out by INDEX)
    hit_c[j][i] = S_FR[j][i] >= t_R[i];  hit_r[j][i] = S_FR[j][i] >= t_F[j]                      (inclusive; NaN: no hit)
    precision = mean_j any_i hit_c, density = sum hit_c / (k n_f), coverage = mean_i any_j hit_c, recall = mean_i any_j hit_r
The order behind "k-th largest" is the kNN kernel's: value descending, then column ascending; -0.0 == +0.0; NaN below
every number."""
import numpy as np

METRICS = ('precision', 'recall', 'density', 'coverage')


def normalize64(x):
    """x / max(||x||_2, 1e-12) per row (F.normalize), in float64."""
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


# ---- the kernels' contracts on a given S (any float dtype, compared exactly, bits kept) ----
def kth_exact(S, k, self0=-1):
    """thr[i]: the float of row i of S that holds the k-th place of the neighbour order among the columns other than
    self0 + i (self0 < 0: all columns).  contrad_prdc_kth's contract."""
    S = np.asarray(S)
    M, n = S.shape
    out = np.empty(M, S.dtype)
    for i in range(M):
        cols = np.arange(n)
        if self0 >= 0 and self0 + i < n:
            cols = np.delete(cols, self0 + i)
        row = S[i, cols]
        assert 1 <= k <= len(row)
        v = np.where(row == 0, np.zeros((), S.dtype), row)          # -0.0 -> +0.0; NaN stays and sorts last as -NaN
        out[i] = row[np.lexsort((cols, -v))[k - 1]]
    return out


def count_exact(S, thr_row=None, thr_col=None):
    """(row_hits[M], col_hits_c[n], col_hits_r[n]) of one call of contrad_prdc_count on zeroed column arrays; None for the
    outputs a missing threshold array skips.  Comparisons in S's own dtype; NaN on either side is no hit."""
    S = np.asarray(S)
    row_hits = col_c = col_r = None
    with np.errstate(invalid='ignore'):
        if thr_col is not None:
            hit = S >= np.asarray(thr_col, S.dtype)[None, :]
            row_hits, col_c = hit.sum(1).astype(np.int64), hit.sum(0).astype(np.int64)
        if thr_row is not None:
            col_r = (S >= np.asarray(thr_row, S.dtype)[:, None]).sum(0).astype(np.int64)
    return row_hits, col_c, col_r


def counts_of(row_hits, col_c, col_r):
    return {'fakes_in_real_balls': int((row_hits > 0).sum()), 'hits': int(row_hits.sum()),
            'reals_with_a_fake': int((col_c > 0).sum()), 'reals_in_fake_balls': int((col_r > 0).sum())}


def metrics_of(counts, n_r, n_f, k):
    return {'precision': counts['fakes_in_real_balls'] / n_f, 'recall': counts['reals_in_fake_balls'] / n_r,
            'density': counts['hits'] / (k * n_f), 'coverage': counts['reals_with_a_fake'] / n_r}


def prdc_from_S(S_RR, S_FF, S_FR, k):
    """The integer counts and metrics the device must give for ITS float32 similarity matrices (S_FR: fake rows, real
    columns), exactly."""
    t_R, t_F = kth_exact(S_RR, k, 0), kth_exact(S_FF, k, 0)
    out = counts_of(*count_exact(S_FR, thr_row=t_F, thr_col=t_R))
    out.update(metrics_of(out, S_RR.shape[0], S_FF.shape[0], k))
    return out


# ---- on features, in float64 ----
def kth_excluding_self(S, k):
    """k-th largest of every row of the square float64 S with the diagonal left out, by an index-excluded sort."""
    n = S.shape[0]
    assert S.shape == (n, n) and 1 <= k <= n - 1
    off = S[~np.eye(n, dtype=bool)].reshape(n, n - 1)               # row i without column i
    return -np.sort(-off, axis=1)[:, k - 1]


def prdc_ref64(real, fake, k, gap=0.0):
    """dict: the float64 point values (counts and metrics) and, per count, the interval [lo, hi] of what an evaluation
    whose similarities and thresholds each carry an error below ``gap / 2`` may return: an indicator with
    |s - t| >= gap is decided, the others count for ``hi`` only."""
    R, F = normalize64(real), normalize64(fake)
    n_r, n_f = len(R), len(F)
    t_R, t_F = kth_excluding_self(R @ R.T, k), kth_excluding_self(F @ F.T, k)
    S = F @ R.T
    dc, dr = S - t_R[None, :], S - t_F[:, None]
    point = counts_of((dc >= 0).sum(1), (dc >= 0).sum(0), (dr >= 0).sum(0))
    lo = counts_of((dc >= gap).sum(1), (dc >= gap).sum(0), (dr >= gap).sum(0))
    hi = counts_of((dc > -gap).sum(1), (dc > -gap).sum(0), (dr > -gap).sum(0))
    out = dict(point)
    out.update(metrics_of(point, n_r, n_f, k))
    out['lo'], out['hi'] = lo, hi
    out['width'] = {m: metrics_of(hi, n_r, n_f, k)[m] - metrics_of(lo, n_r, n_f, k)[m] for m in METRICS}
    out.update({'n_real': n_r, 'n_fake': n_f, 'k': k})
    return out


def manifold_sets(seed, d, n_r, n_f, q=8):
    """Real and fake rows on a q-dimensional subspace of R^d plus a little full-rank noise; the fakes' first latent
    coordinate is pushed to one side, so that they cover only part of the reals."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((q, d)) / np.sqrt(d)
    R = normalize64(rng.standard_normal((n_r, q)) @ A + 0.01 * rng.standard_normal((n_r, d)) / np.sqrt(d))
    z = rng.standard_normal((n_f, q))
    z[:, 0] = np.abs(z[:, 0]) * 0.7 + 0.3
    F = normalize64(z @ A + 0.01 * rng.standard_normal((n_f, d)) / np.sqrt(d))
    return R, F
