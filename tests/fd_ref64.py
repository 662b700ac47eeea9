"""The float64 yardstick of the Frechet distance (contrad_amd/fd.py): numpy only, none of this project's kernels.

    mu = column mean        Sigma = np.cov(rows, rowvar=False)  (ddof 1)
    fd = ||mu_r - mu_f||^2 + tr Sigma_r + tr Sigma_f - 2 ||A B^T||_*,   A = (R - mu_r) / sqrt(n_r - 1), B = (F - mu_f) / sqrt(n_f - 1)

with the nuclear norm as the sum of the singular values ``np.linalg.svd`` returns.  ``textbook`` restates the trace term as
sum sqrt(eigvalsh(S_r^(1/2) S_f S_r^(1/2))) on the d x d covariances (full-rank cases); ``emulate_fp32`` restates the DEVICE
algorithm in float32 numpy (float64 only where the device uses it: the means, the sums of products, the host combination),
for the conditions of the GPU cases that can be checked without a GPU.  ``sets`` makes the feature cases of
tests/test_fd_gpu.py."""
import math

import numpy as np


def normalize64(X):
    X = np.asarray(X, np.float64)
    return X / np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), 1e-12)


def moments(rows):
    """(mu [d], Sigma [d][d]) in float64: the column mean and np.cov(rows, rowvar=False)."""
    rows = np.asarray(rows, np.float64)
    return rows.mean(0), np.atleast_2d(np.cov(rows, rowvar=False))


def centred(rows):
    """(rows - mu) / sqrt(n - 1) in float64: A with A^T A = Sigma."""
    rows = np.asarray(rows, np.float64)
    return (rows - rows.mean(0)) / math.sqrt(rows.shape[0] - 1)


def nuclear(A, B):
    return float(np.linalg.svd(A @ B.T, compute_uv=False).sum())


def fd_ref64(real, fake, normalize=True):
    """The distance and its terms from float64 rows; ``normalize``: L2-normalise the rows first (x / max(||x||, 1e-12))."""
    R, F = (normalize64(real), normalize64(fake)) if normalize else (np.asarray(real, np.float64), np.asarray(fake, np.float64))
    A, B = centred(R), centred(F)
    diff = R.mean(0) - F.mean(0)
    out = {'mean_term': float(diff @ diff), 'trace_real': float((A * A).sum()), 'trace_fake': float((B * B).sum()),
           'cross_term': nuclear(A, B)}
    out['fd'] = out['mean_term'] + out['trace_real'] + out['trace_fake'] - 2.0 * out['cross_term']
    out['scale'] = out['mean_term'] + out['trace_real'] + out['trace_fake']
    return out


def textbook(real, fake):
    """The same distance with the trace term from the d x d covariances: sum sqrt(eigvalsh(S_r^(1/2) S_f S_r^(1/2)))."""
    (mu_r, S_r), (mu_f, S_f) = moments(real), moments(fake)
    w, V = np.linalg.eigh(S_r)
    root = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    ev = np.linalg.eigvalsh(root @ S_f @ root)
    diff = mu_r - mu_f
    return float(diff @ diff + np.trace(S_r) + np.trace(S_f) - 2.0 * np.sqrt(np.maximum(ev, 0.0)).sum())


def emulate_fp32(R, F, n_iter):
    """The device algorithm in float32 numpy on already normalised rows: float64 means, rows centred and rounded once to
    fp32, M = Fc Rc^T oriented [p][q] with q the smaller, X_0 = M / ||M||_F, X <- X (1.5 I - 0.5 X^T X), the estimates
    <X_k, M> and the sums of squares as float64 sums of exact products.  Returns the dict of ``fd.combine``'s terms."""
    R32, F32 = np.asarray(R, np.float32), np.asarray(F, np.float32)
    n_r, n_f = R32.shape[0], F32.shape[0]
    mu_r, mu_f = R32.astype(np.float64).mean(0), F32.astype(np.float64).mean(0)
    Rc, Fc = (R32.astype(np.float64) - mu_r).astype(np.float32), (F32.astype(np.float64) - mu_f).astype(np.float32)
    M = Fc @ Rc.T if n_f >= n_r else Rc @ Fc.T
    dot = lambda a, b: float((a.astype(np.float64) * b.astype(np.float64)).sum())
    fro2 = dot(M, M)
    X = M * np.float32(1.0 / math.sqrt(fro2) if fro2 > 0 else 0.0)
    eye = np.eye(M.shape[1], dtype=np.float32)
    est = []
    for _ in range(n_iter):
        X = X @ (np.float32(1.5) * eye - np.float32(0.5) * (X.T @ X))
        est.append(dot(X, M))
    mean_term = float(((mu_r - mu_f) ** 2).sum())
    tr_r, tr_f = dot(Rc, Rc) / (n_r - 1), dot(Fc, Fc) / (n_f - 1)
    cross = est[-1] / math.sqrt(float(n_r - 1) * float(n_f - 1))
    return {'fd': mean_term + tr_r + tr_f - 2.0 * cross, 'mean_term': mean_term, 'trace_real': tr_r, 'trace_fake': tr_f,
            'cross_term': cross, 'estimates': est}


# ---- the feature cases of the GPU tests: (d, n_r, n_f, kind) ----
FEATURE_CASES = [(24, 300, 257, 'moved'), (512, 300, 257, 'moved'), (64, 1000, 37, 'moved'), (16, 2, 2, 'moved'),
                 (8192, 300, 257, 'moved'), (24, 300, 257, 'state'), (24, 300, 300, 'equal')]
TOL_CAP = 1e-5
MIN_FD = 1e-3                                                               # of s: the float64 fd of every case but 'equal'


def sets(case, seed=0):
    """(real, fake) float32 rows of a case, ReLU-like (non-negative, as penultimate features after an activation) and NOT
    normalised: rows on an 8-dimensional subspace plus noise, the fakes moved along the first latent.  'equal': the fake
    set is the real set."""
    d, n_r, n_f, kind = case
    r = np.random.RandomState(1000 + seed)
    basis = r.randn(min(8, d), d)
    real = np.maximum(r.randn(n_r, basis.shape[0]) @ basis + 0.3 * r.randn(n_r, d) + 0.5, 0.0)
    if kind == 'equal':
        return real.astype(np.float32), real.astype(np.float32).copy()
    z = r.randn(n_f, basis.shape[0])
    z[:, 0] += 1.5
    fake = np.maximum(z @ basis + 0.3 * r.randn(n_f, d) + 0.5, 0.0)
    return real.astype(np.float32), fake.astype(np.float32)
