"""Float64 statement of the kernel distance of contrad_amd/kid.py in plain numpy (no project kernels), and the sum
contrad_kid_sums must give on a given float32 S with the bound it must meet.  The yardstick of tests/test_kid_gpu.py,
tied to a brute-force double loop by tests/test_kid_ref64_cpu.py.

With R, F the real and fake rows (L2-normalised in float64), k(a, b) = (gamma a.b + coef0)^3 and, per subset t of m rows
of each set (the index sets of ``kid.subset_indices``):
    A_t = sum_{i != j} k(S_RR),  B_t = sum_{i != j} k(S_FF),  C_t = sum_{i, j} k(S_FR)     (self pairs left out by INDEX)
    MMD2_t = (A_t + B_t) / (m (m - 1)) - 2 C_t / m^2,  kid = mean_t MMD2_t,  kid_std = std_t MMD2_t (ddof 0)
Every sum here is ``math.fsum``: correctly rounded, whatever the order."""
import math

import numpy as np


def normalize64(x):
    """x / max(||x||_2, 1e-12) per row (F.normalize), in float64."""
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def _included(M, n, self0):
    """[M][n] bool: False at column self0 + i of row i (self0 < 0: nowhere)."""
    keep = np.ones((M, n), bool)
    if self0 >= 0:
        for i in range(M):
            if self0 + i < n:
                keep[i, self0 + i] = False
    return keep


# ---- the kernel's contract on a given S ----
def block_sum(S, self0=-1, gamma=1.0, coef0=1.0):
    """fsum over i, j != self0 + i of (gamma * float64(S[i][j]) + coef0)^3: what contrad_kid_sums states."""
    S = np.asarray(S)
    x = gamma * S.astype(np.float64) + coef0
    return math.fsum((x ** 3)[_included(S.shape[0], S.shape[1], self0)].tolist())


def block_bound(S, self0=-1, gamma=1.0, coef0=1.0):
    """(M n + 16) 2^-53 sum (|gamma s| + |coef0|)^3 over the elements that count: any summation order of M n terms, each
    formed with a few roundings (an FMA in place of the multiply-add included), stays inside it."""
    S = np.asarray(S)
    M, n = S.shape
    a = np.abs(gamma * S.astype(np.float64)) + abs(coef0)
    return (M * n + 16) * 2.0 ** -53 * math.fsum((a ** 3)[_included(M, n, self0)].tolist())


def mmd2_of(sums, m):
    """MMD2_t of a [n_subsets][3] table of (A_t, B_t, C_t): the host formula, in float64."""
    s = np.asarray(sums, np.float64).reshape(-1, 3)
    return (s[:, 0] + s[:, 1]) / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)


def kid_of_sums(sums, m):
    """(kid, kid_std) of the table."""
    v = mmd2_of(sums, m)
    return float(v.mean()), float(v.std())


# ---- on features, in float64 ----
def subset_sums64(Rn, Fn, idx_r, idx_f, gamma=1.0, coef0=1.0):
    """(A, B, C) of one subset of the normalised float64 rows, S formed in float64."""
    Rt, Ft = Rn[idx_r], Fn[idx_f]
    return (block_sum(Rt @ Rt.T, 0, gamma, coef0), block_sum(Ft @ Ft.T, 0, gamma, coef0), block_sum(Ft @ Rt.T, -1, gamma, coef0))


def kid_ref64(real, fake, n_subsets=100, subset_size=1000, seed=0, gamma=1.0, coef0=1.0):
    """The float64 kernel distance of raw feature rows; the index sets come from ``kid.subset_indices``."""
    from contrad_amd.kid import subset_indices
    Rn, Fn = normalize64(real), normalize64(fake)
    m = min(subset_size, len(Rn), len(Fn))
    assert m >= 2 and n_subsets >= 1
    idx_r, idx_f = subset_indices(len(Rn), len(Fn), m, n_subsets, seed)
    sums = [subset_sums64(Rn, Fn, idx_r[t], idx_f[t], gamma, coef0) for t in range(n_subsets)]
    kid, std = kid_of_sums(sums, m)
    return {'kid': kid, 'kid_std': std, 'sums': sums, 'subset_size': m, 'n_subsets': n_subsets}


def shifted_sets(seed, d, n_r, n_f, shift, q=8):
    """Real and fake rows on a q-dimensional subspace of R^d plus 1 % full-rank noise; the fakes' first latent coordinate is
    moved by ``shift`` (0: both sets come from one distribution)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((q, d)) / np.sqrt(d)
    R = rng.standard_normal((n_r, q)) @ A + 0.01 * rng.standard_normal((n_r, d)) / np.sqrt(d)
    z = rng.standard_normal((n_f, q))
    z[:, 0] += shift
    F = z @ A + 0.01 * rng.standard_normal((n_f, d)) / np.sqrt(d)
    return R, F
