"""Float64 statement of the contrastive diagnostics of contrad_amd/contrast.py in plain numpy and ``math`` (none of this
project's kernels): the sum contrad_gauss_sums must give on a given float32 S with the bound it must meet, and alignment,
uniformity, the ranks of the positives and NT-Xent from given rows.  The yardstick of tests/test_contrast_stats_gpu.py, tied
to closed forms by tests/test_contrast_ref64_cpu.py.

The term, for a similarity s of two unit vectors, all in float64:
    u = 2 - 2 s, clamped below at 0 by ``u < 0 ? 0 : u`` (a NaN stays a NaN; an s slightly above 1 gives u = 0)
    term = exp(-(t u))

Bound of the kernel on a given S, derived not measured: ``sum_i term_i (t u_i + 5) 2^-53 + (M n + 16) 2^-53 sum_i term_i``.
  * u is exact in float64: s is a float, 2 s and 2 - 2 s fit 53 bits.
  * t u is one rounding, relative 2^-53; it moves exp(-(t u)) by at most t u 2^-53, relative.
  * the device's exp: OCML's double-precision exp.  The ROCm installation this was written against ships OCML as bitcode
    only (lib/llvm/lib/clang/*/lib/amdgcn/bitcode/ocml.bc) and no accuracy table, so no figure could be cited from it; the
    figure used is 1 ulp, as the accuracy table of OCML's public documentation is remembered for exp in double precision
    (not confirmed from the installation): at most 2^-52, relative.  A case that fails at this bound is a finding to report.
  * the host's ``math.exp`` of this yardstick: at most 1 ulp, 2^-52 relative.
  * together (t u + 4) 2^-53 per term, +1 for the second-order products of these.
  * the summation term is tests/kid_ref64.py's ``block_bound``: (M n + 16) 2^-53 sum |terms| covers any order of M n
    additions.
A dropped or doubled cell weighs at least exp(-4 t) (u <= 4) in a sum of at most M n: at t = 2 a relative weight of at least
3.3e-4 / (M n), 3e-10 at 1000 x 1000 against a relative bound near 1e-10 there and far more at the sizes the tests use.
Every sum here is ``math.fsum``: correctly rounded, whatever the order."""
import math

import numpy as np

import kid_ref64 as K

normalize64 = K.normalize64


# ---- the kernel's contract on a given S ----
def gauss_u(S):
    s = np.asarray(S).astype(np.float64)
    u = 2.0 - 2.0 * s
    return np.where(u < 0.0, 0.0, u)                                   # (a NaN compares false: it stays)


def gauss_terms(S, t):
    """The float64 terms, one ``math.exp`` each."""
    u = gauss_u(S)
    return np.array([math.exp(-(t * v)) if v == v else float('nan') for v in u.reshape(-1).tolist()], np.float64).reshape(u.shape)


def gauss_block_sum(S, self0=-1, t=2.0):
    """fsum over i, j != self0 + i of exp(-t max(2 - 2 s, 0)): what contrad_gauss_sums states."""
    S = np.asarray(S)
    return math.fsum(gauss_terms(S, t)[K._included(S.shape[0], S.shape[1], self0)].tolist())


def gauss_block_bound(S, self0=-1, t=2.0):
    S = np.asarray(S)
    M, n = S.shape
    keep = K._included(M, n, self0)
    terms, u = gauss_terms(S, t)[keep], gauss_u(S)[keep]
    per_term = math.fsum((terms * (t * u + 5.0)).tolist())
    return 2.0 ** -53 * (per_term + (M * n + 16) * math.fsum(np.abs(terms).tolist()))


# ---- from given rows, in float64 ----
def sq_dist(a, b):
    """u(a, b) = max(2 - 2 a.b, 0) for every pair of rows: [len(a)][len(b)]."""
    return np.maximum(2.0 - 2.0 * (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T), 0.0)


def alignment(A, B):
    """mean_i u(A_i, B_i) of unit rows."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return math.fsum(np.maximum(2.0 - 2.0 * (A * B).sum(1), 0.0).tolist()) / len(A)


def uniformity(A, t=2.0):
    """log of the mean over i != j of exp(-t u(A_i, A_j)); the self pair is left out by index."""
    n = len(A)
    U = sq_dist(A, A)
    keep = ~np.eye(n, dtype=bool)
    return math.log(math.fsum(np.exp(-t * U)[keep].tolist()) / (n * (n - 1.0)))


def blocks_of(n, batch):
    b = min(batch, n)
    return [(i, min(b, n - i)) for i in range(0, n, b)]


def block_ranks(Z, b):
    """Z = [A_blk | B_blk] (2b, d) unit rows -> (rank (2b,), margin (2b,)): rank_i = #{j not in {i, pos(i)} : s_ij >= s_i,pos(i)}
    (ties count against the positive, the row itself is left out by index); margin_i = min over those j of |s_ij - s_i,pos(i)|
    (inf without competitors)."""
    Z = np.asarray(Z, np.float64)
    R = 2 * b
    S = Z @ Z.T
    rank, margin = np.zeros(R, np.int64), np.full(R, np.inf)
    for i in range(R):
        p = (i + b) % R
        others = [j for j in range(R) if j != i and j != p]
        if others:
            rank[i] = int((S[i, others] >= S[i, p]).sum())
            margin[i] = float(np.abs(S[i, others] - S[i, p]).min())
    return rank, margin


def ranks(A, B, batch):
    """(rank (2n,), margin (2n,)) over the blocks, each block's rows in the order [A_blk | B_blk]."""
    out = [block_ranks(np.concatenate([A[i:i + m], B[i:i + m]]), m) for i, m in blocks_of(len(A), batch)]
    return np.concatenate([r for r, _ in out]), np.concatenate([m for _, m in out])


def rank_stats(rank):
    rank = np.asarray(rank)
    return {'acc@1': float((rank == 0).mean()), 'acc@5': float((rank < 5).mean()), 'rank_mean': float(rank.mean())}


def block_nt_xent(Z, b, temp):
    """mean_i of -log(exp(s_i,pos(i) / temp) / sum_{j != i} exp(s_ij / temp)) over the 2b rows of a block."""
    Z = np.asarray(Z, np.float64)
    R = 2 * b
    L = (Z @ Z.T) / temp
    total = []
    for i in range(R):
        row = np.delete(L[i], i)
        m = row.max()
        total.append(m + math.log(math.fsum(np.exp(row - m).tolist())) - L[i, (i + b) % R])
    return math.fsum(total) / R


def nt_xent(A, B, batch, temp):
    """The block values averaged with the blocks' row counts as weights."""
    n = len(A)
    return math.fsum(2 * m * block_nt_xent(np.concatenate([A[i:i + m], B[i:i + m]]), m, temp) for i, m in blocks_of(n, batch)) / (2 * n)


def stats64(A, B, batch, temp, t=2.0):
    """Every projection-space quantity of ``contrast_stats`` from unit float64 rows."""
    rank, _ = ranks(A, B, batch)
    out = rank_stats(rank)
    out.update({'nt_xent': nt_xent(A, B, batch, temp), 'align': alignment(A, B), 'uniform': uniformity(A, t),
                'chance': 1.0 / (2 * min(batch, len(A)) - 2)})
    return out


def planted_views(seed, n, d, noise=1.5):
    """Raw rows of view A and view B = A + noise * gaussian (normalised by the caller)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, d))
    return A, A + noise * rng.standard_normal((n, d))
