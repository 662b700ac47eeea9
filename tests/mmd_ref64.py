"""Float64 statement of the rational-quadratic kernel of contrad_amd/kid.py (``kernel='rq'``, contrad_mmd_sums kind 1) in
plain numpy (none of this project's kernels): the sum the kernel must give on a given float32 S with the bound it must
meet, the distance on float64 features, a brute-force double-loop MMD^2 for tiny sets and the intra-class restatement.
The yardstick of tests/test_kid_kernels_gpu.py, tied to the double loop by tests/test_kid_kernels_cpu.py.

The term, for a similarity s of two unit vectors, all in float64:
    u = 2 - 2 s, clamped below at 0 by ``u < 0 ? 0 : u`` (a NaN stays a NaN; an s slightly above 1 gives u = 0)
    term = 1 / sqrt(1 + u) + 1 / (1 + u / 2) + 1 / (1 + u / 4)^2  =  sum over alpha in {1/2, 1, 2} of (1 + u / (2 alpha))^-alpha

Bound, derived not measured: ``(M n + 32) 2^-53 fsum(|terms|)``.  2 - 2 s is exact or one rounding; each of the three
addends is at most 4 correctly rounded operations of condition at most 1, and the two additions make at most 16 roundings
per term, doubled for slack; fused multiply-adds only remove roundings; any summation order costs at most M n roundings.
The lightest single cell is a term of at least 1.03 (u <= 4: 1 / sqrt(5) + 1 / 3 + 1 / 4) in a sum of at most 3 M n: a
relative weight of at least 0.3 / (M n), 3e-7 at 1000 x 1000 against a bound near 1e-10 -- a dropped or doubled cell
cannot hide.  Every sum here is ``math.fsum``: correctly rounded, whatever the order."""
import math

import numpy as np

import kid_ref64 as K

KIND_POLY3, KIND_RQ = 0, 1


def rq_terms(S):
    """The float64 terms of a float32 (or float64) array of similarities, as written above."""
    s = np.asarray(S).astype(np.float64)
    u = 2.0 - 2.0 * s
    u = np.where(u < 0.0, 0.0, u)                                      # (a NaN compares false: it stays)
    q = 1.0 + 0.25 * u
    return 1.0 / np.sqrt(1.0 + u) + 1.0 / (1.0 + 0.5 * u) + 1.0 / (q * q)


def block_sum(S, self0=-1):
    """fsum over i, j != self0 + i of the terms: what contrad_mmd_sums states for kind 1."""
    S = np.asarray(S)
    return math.fsum(rq_terms(S)[K._included(S.shape[0], S.shape[1], self0)].tolist())


def block_bound(S, self0=-1):
    S = np.asarray(S)
    M, n = S.shape
    return (M * n + 32) * 2.0 ** -53 * math.fsum(np.abs(rq_terms(S))[K._included(M, n, self0)].tolist())


# ---- on features, in float64 ----
def subset_sums64(Rn, Fn, idx_r, idx_f):
    """(A, B, C) of one subset of the normalised float64 rows, S formed in float64."""
    Rt, Ft = Rn[idx_r], Fn[idx_f]
    return block_sum(Rt @ Rt.T, 0), block_sum(Ft @ Ft.T, 0), block_sum(Ft @ Rt.T, -1)


def kid_ref64(real, fake, n_subsets=100, subset_size=1000, seed=0):
    """The float64 rational-quadratic distance of raw feature rows; the index sets come from ``kid.subset_indices``."""
    from contrad_amd.kid import subset_indices
    Rn, Fn = K.normalize64(real), K.normalize64(fake)
    m = min(subset_size, len(Rn), len(Fn))
    assert m >= 2 and n_subsets >= 1
    idx_r, idx_f = subset_indices(len(Rn), len(Fn), m, n_subsets, seed)
    sums = [subset_sums64(Rn, Fn, idx_r[t], idx_f[t]) for t in range(n_subsets)]
    kid, std = K.kid_of_sums(sums, m)
    return {'kid': kid, 'kid_std': std, 'sums': sums, 'subset_size': m, 'n_subsets': n_subsets}


def feature_bound(d):
    """|kid_rq on the device - kid_rq in float64| <= 12 e, e = (2 d + 8) 2^-24 (the device similarity against the float64
    one, tests/test_knn_gpu.py): each of the three addends has slope at most 1 in s (d/ds of (1 + u / (2 alpha))^-alpha is
    (1 + u / (2 alpha))^(-alpha - 1) <= 1, and the clamp does not steepen it), so the term is 3-Lipschitz; an MMD^2 is four
    means of terms (weights 1, 1, -2)."""
    return 12.0 * (2 * d + 8) * 2.0 ** -24


# ---- brute force, tiny sets ----
def _unit(rows):
    return [[x / max(sum(v * v for v in r) ** 0.5, 1e-12) for x in r] for r in rows]


def _k(a, b):
    u = max(2.0 - 2.0 * sum(x * y for x, y in zip(a, b)), 0.0)
    return (1.0 + u) ** -0.5 + (1.0 + u / 2.0) ** -1.0 + (1.0 + u / 4.0) ** -2.0


def brute_mmd2(real, fake, idx_r, idx_f):
    """(MMD2, A, B, C) of every subset by double loops over plain Python floats, the kernel written with ``**``."""
    Rn, Fn = _unit(np.asarray(real).tolist()), _unit(np.asarray(fake).tolist())
    out = []
    for ir, jf in zip(np.asarray(idx_r).tolist(), np.asarray(idx_f).tolist()):
        m = len(ir)
        A = sum(_k(Rn[ir[i]], Rn[ir[j]]) for i in range(m) for j in range(m) if i != j)
        B = sum(_k(Fn[jf[i]], Fn[jf[j]]) for i in range(m) for j in range(m) if i != j)
        C = sum(_k(Fn[jf[i]], Rn[ir[j]]) for i in range(m) for j in range(m))
        out.append(((A + B) / (m * (m - 1)) - 2 * C / m ** 2, A, B, C))
    return out


# ---- intra-class ----
def intra_of(values):
    """(kid_intra, kid_intra_std) of the class values: the plain mean and the population deviation, by hand in float64."""
    v = [float(x) for x in values]
    mean = math.fsum(v) / len(v)
    return mean, math.sqrt(math.fsum((x - mean) ** 2 for x in v) / len(v))


def intra_ref64(real, real_labels, fake, fake_labels, n_classes, n_subsets, subset_size, seed, kernel='rq'):
    """Per class c in order, the float64 distance of the rows of class c (the same seed for every class,
    m_c = min(subset_size, n_r_c, n_f_c)) -> (the class values, their mean, their population deviation)."""
    real_labels, fake_labels = np.asarray(real_labels), np.asarray(fake_labels)
    ref = kid_ref64 if kernel == 'rq' else K.kid_ref64
    values = [ref(real[real_labels == c], fake[fake_labels == c], n_subsets, subset_size, seed)['kid'] for c in range(n_classes)]
    return (values,) + intra_of(values)
