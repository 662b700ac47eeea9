"""The yardstick of the latent-space tools (contrad_amd/latent.py, csrc/latent/latent.hip): float64 numpy written for these
kernels.  Plain functions, no GPU.

Definitions (include/contrad_hip.h).
  * ``normalize(x) = x / max(|x|, 1e-300)``: a zero row stays zero.
  * ``lerp(a, b, t) = a + t (b - a)``.
  * ``slerp(a, b, t)`` (Karras et al.): a^, b^ normalised, r = b^ - (a^.b^) a^, theta = atan2(|r|, a^.b^) -- never acos, whose
    derivative is unbounded where the dot product is near 1 -- point = normalize(a^ cos(t theta) + (r / |r|) sin(t theta)).
    Where |r| <= (d + 16) 2^-52 the point is a^ for every t: in exact arithmetic that is |r| = 0 (b = a, b = -a); in float64 the
    dot product of two unit rows carries a rounding chain of that size and r's direction below it is noise.
  * ``pair(a, b, t, dt, mode)``: the points at t and at float64(t) + dt, t an fp32 value.
  * ``styles``: out[b, l] = w_avg + psi[l] (src - w_avg), src = w[b] if l < cross[b] else w2[b]; a layer with psi 1 is the source.
  * ``pair_dist``: scale |A^ - B^|^2 with x^ = x / max(|x|, 1e-12), in ``np.longdouble`` where that has more than 53 mantissa bits.
  * ``percentile_mean``: Karras' rule.

Bounds (derived, not measured).
  * ``pair_bound``: 2^-24 |ref| + (d + 16) 2^-52 max(1, |a|_inf, |b|_inf): one fp32 rounding of the result, and the float64 chain
    (sums of d terms, a few quotients, sine and cosine) acting on values no larger than the inputs.
  * ``styles_bound``: 3 2^-24 (|w_avg| + |psi| (|src| + |w_avg|)): the difference, the product and the sum each round once in fp32,
    fused or not.
  * ``pair_dist_bound``: scale [(d + 8) u (4 D + D^2) + 8 ((d + 8) u)^2], u = 2^-53, D^2 = ref / scale: each norm is off by at
    most (d + 8) u relatively, which moves each unit row by that much and the difference vector by twice it, hence the square by
    4 D (d + 8) u to first order; the differences, their squares and their sum add (d + 8) u D^2; the last term is the
    second order.  Doubled where the yardstick itself is only float64.
"""
import numpy as np

TINY = 1e-300
PAIR_TINY = 1e-12
U = 2.0 ** -53
LONG = np.finfo(np.longdouble).nmant > 52


def normalize(x, tiny=TINY):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt(np.sum(x * x, axis=-1, keepdims=True)), tiny)


def degenerate_below(d):
    return (d + 16) * 2.0 ** -52


def slerp_parts(a, b):
    """(a^, c, theta, degenerate) of rows a, b [n, d]; c is zero and theta 0 on degenerate rows."""
    ah, bh = normalize(a), normalize(b)
    dot = np.sum(ah * bh, axis=-1, keepdims=True)
    r = bh - dot * ah
    nr = np.sqrt(np.sum(r * r, axis=-1, keepdims=True))
    deg = ~(nr > degenerate_below(ah.shape[-1]))
    c = np.where(deg, 0.0, r / np.where(deg, 1.0, nr))
    theta = np.where(deg, 0.0, np.arctan2(nr, dot))
    return ah, c, theta, deg


def slerp(a, b, t):
    """Rows a, b [n, d] float64 and t [n] float64 -> the points [n, d] float64."""
    ah, c, theta, deg = slerp_parts(a, b)
    ang = np.asarray(t, np.float64).reshape(-1, 1) * theta
    p = normalize(ah * np.cos(ang) + c * np.sin(ang))
    return np.where(deg, ah, p)


def lerp(a, b, t):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a + np.asarray(t, np.float64).reshape(-1, 1) * (b - a)


def pair(a, b, t, dt, mode):
    """The two points in float64 (not yet rounded to fp32) for fp32 inputs a, b [n, d], t [n]."""
    t0 = np.asarray(t, np.float32).astype(np.float64)
    f = slerp if mode == 1 else lerp
    return f(a, b, t0), f(a, b, t0 + float(dt))


def pair_bound(ref, a, b):
    d = a.shape[-1]
    big = max(1.0, float(np.abs(a).max()), float(np.abs(b).max()))
    return 2.0 ** -24 * np.abs(ref) + (d + 16) * 2.0 ** -52 * big


def styles(w, L, w2=None, cross=None, w_avg=None, psi=None):
    """float64 [B, L, d] and the source rows float32 [B, L, d]."""
    B, d = w.shape
    src = np.repeat(np.asarray(w, np.float32)[:, None, :], L, axis=1)
    if w2 is not None:
        take_w = np.arange(L)[None, :] < np.asarray(cross, np.float64)[:, None]
        src = np.where(take_w[:, :, None], src, np.asarray(w2, np.float32)[:, None, :])
    if psi is None:
        return src.astype(np.float64), src
    m, p = np.asarray(w_avg, np.float64).reshape(1, 1, d), np.asarray(psi, np.float64).reshape(1, L, 1)
    return m + p * (src.astype(np.float64) - m), src


def styles_bound(src, w_avg, psi):
    d = src.shape[-1]
    m, p = np.abs(np.asarray(w_avg, np.float64)).reshape(1, 1, d), np.abs(np.asarray(psi, np.float64)).reshape(1, -1, 1)
    return 3.0 * 2.0 ** -24 * (m + p * (np.abs(src.astype(np.float64)) + m))


def pair_dist(A, B, scale=1.0):
    """scale |A^ - B^|^2 per row, as float64, computed in np.longdouble."""
    A, B = np.asarray(A, np.float32).astype(np.longdouble), np.asarray(B, np.float32).astype(np.longdouble)
    tiny = np.longdouble(PAIR_TINY)
    na = np.maximum(np.sqrt(np.sum(A * A, axis=1, keepdims=True)), tiny)
    nb = np.maximum(np.sqrt(np.sum(B * B, axis=1, keepdims=True)), tiny)
    df = A / na - B / nb
    return (np.longdouble(scale) * np.sum(df * df, axis=1)).astype(np.float64)


def pair_dist_bound(ref, d, scale):
    D2 = np.asarray(ref, np.float64) / scale
    D = np.sqrt(D2)
    e = (d + 8) * U
    bound = scale * (e * (4.0 * D + D2) + 8.0 * e * e)
    return bound if LONG else 2.0 * bound


def percentile_mean(d):
    """Karras' rule -> (mean of the kept values, mean of all, number kept)."""
    d = np.asarray(d, np.float64)
    lo, hi = np.percentile(d, 1, method='lower'), np.percentile(d, 99, method='higher')
    keep = (lo <= d) & (d <= hi)
    return float(d[keep].mean()), float(d.mean()), int(keep.sum())


def ppl(f0, f1, eps):
    """The assembly of ``latent.ppl_of`` from the float feature rows of both ends -> (ppl, ppl_raw, kept, d)."""
    d = pair_dist(f0, f1, 1.0 / (eps * eps))
    return percentile_mean(d) + (d,)
