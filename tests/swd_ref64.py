"""The yardstick of the sliced Wasserstein distance (contrad_amd/swd.py's docstring is the definition): float64 numpy and
``scipy.ndimage.convolve(..., mode='mirror')``, explicit draws, none of this project's code.  Plain data and helpers, no GPU.

Besides the distance it holds the error bounds that tests/test_swd_kernels_gpu.py asserts, derived from the arithmetic and
computed from the yardstick's own absolute sums (u = 2^-24, gamma_k = k u / (1 - k u)):

* pyramid.  A uint8 level is exact in fp32.  ``down`` forms 25 products with weights that are exact in fp32 and adds them in
  fp32, so |fl(down(x^)) - down(x)| <= gamma_25 F*(|x| + E) + F*E where x^ = x + e, |e| <= E elementwise and F* is the same
  stencil on the absolute values.  ``up`` is the same statement on the zero-inserted level with 4 F; the subtraction adds one
  rounding: E(L) = E(G) + E(up) + u (|L| + E(G) + E(up)).
* projection.  With w = dirs / sigma (float64), the device forms fl32(dirs / sigma^) as the GEMM's rows, 148 products added in
  fp32 in some order, and centres with mu^ in float64: |p^ - p| <= gamma_148 max sum_k |w_k| (|b_k| + E) + (u + r)(1 + u) max
  sum_k |w_k| (|b_k - mu| + 2 E) + 2 E max sum_k |w_k| + host, where E bounds the level's error, r = E / (sigma - E) bounds the
  relative error of 1 / sigma^ (the standard deviation is 1-Lipschitz in the root mean square of a perturbation, the mean in
  its maximum) and ``host`` = 400 2^-53 max sum_k |w_k| (|b_k| + |mu|) covers the float64 sums behind mu^, sigma^ and the row
  constants.
* distance.  Sorting is 1-Lipschitz in the sup norm, so a level's value moves by at most the two sets' projection errors
  added, times 1e3.
"""
import math

import numpy as np
from scipy import ndimage

U = 2.0 ** -24
G1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
F = np.outer(G1, G1)
PATCH, HALF, DESC = 7, 3, 147


def gamma(k):
    return k * U / (1.0 - k * U)


def levels_of(size):
    out = []
    while size >= 16:
        out.append(size)
        size //= 2
    return out


def _conv(x, scale=1.0):
    """x [n, H, W, 3] convolved with scale * F over H and W, mirror boundary."""
    return ndimage.convolve(x, (scale * F)[None, :, :, None], mode='mirror')


def down(x):
    return _conv(x)[:, ::2, ::2]


def up(x):
    z = np.zeros((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.shape[3]), np.float64)
    z[:, ::2, ::2] = x
    return _conv(z, 4.0)


def pyramid(x, n_levels):
    """The Laplacian pyramid of x [n, H, W, 3] (any real dtype), finest first; the last level is Gaussian."""
    pyr = [np.asarray(x, np.float64)]
    for i in range(1, n_levels):
        pyr.append(down(pyr[i - 1]))
        pyr[i - 1] = pyr[i - 1] - up(pyr[i])
    return pyr


def pyramid_bounds(x, n_levels):
    """Elementwise bounds [n, res, res, 3] on |fp32 level - float64 level| for every level of ``pyramid(x, n_levels)``
    (module docstring).

    For a uint8 set the first steps are exact and their bound is 0.  A Gaussian level holds values in [0, 255] on the grid
    2^-q (q = 0 for the images).  The weights of ``down`` are multiples of 2^-8 and not negative, so every product and every
    partial sum is a multiple of 2^-(q + 8) inside [0, 255]: it fits the 24 bits of an fp32 significand while q + 16 <= 24,
    and the next level has q + 8.  The weights of ``up`` are multiples of 2^-6: products and partial sums are exact while
    q + 6 + 8 <= 24 (q of the coarse level), and so is the difference with the finer level, of magnitude below 2^9 on the
    coarser of the two grids, while that grid's bits + 9 <= 24.  So G_1, G_2 and L_0 of a uint8 set are exact; L_1 takes the
    roundings of ``up`` and of the subtraction, G_3 those of ``down``."""
    x = np.asarray(x)
    q = [0 if x.dtype == np.uint8 else None]                       # grid bits of the Gaussian levels (None: no grid known)
    gauss = [x.astype(np.float64)]
    e_gauss = [np.zeros_like(gauss[0])]
    bounds = []
    for i in range(1, n_levels):
        g, e = gauss[i - 1], e_gauss[i - 1]
        gauss.append(down(g))
        if q[i - 1] is not None and q[i - 1] + 16 <= 24:
            q.append(q[i - 1] + 8)
            e_gauss.append(np.zeros_like(gauss[i]))
        else:
            q.append(None)
            e_gauss.append(gamma(25) * down(np.abs(g) + e) + down(e))
        lap = g - up(gauss[i])
        if q[i] is not None and q[i] + 14 <= 24 and max(q[i - 1], q[i] + 6) + 9 <= 24:
            bounds.append(np.zeros_like(lap))
            continue
        e_up = gamma(25) * up(np.abs(gauss[i]) + e_gauss[i]) + up(e_gauss[i])
        bounds.append(e + e_up + U * (np.abs(lap) + e + e_up))
    bounds.append(e_gauss[-1])
    return bounds


def descriptors(level, pos, nhoods):
    """[n * nhoods, 147] patches of level [n, res, res, 3] around pos [n * nhoods, 2] (cx, cy), order c * 49 + dy * 7 + dx."""
    pos = np.asarray(pos)
    img = np.arange(len(pos)) // nhoods
    dy, dx = np.meshgrid(np.arange(-HALF, HALF + 1), np.arange(-HALF, HALF + 1), indexing='ij')
    yy = pos[:, 1][:, None, None] + dy[None]
    xx = pos[:, 0][:, None, None] + dx[None]
    patches = level[img[:, None, None], yy, xx]                  # [n_desc, 7, 7, 3]
    return patches.transpose(0, 3, 1, 2).reshape(len(pos), DESC)


def channel_stats(desc):
    d = desc.reshape(len(desc), 3, PATCH * PATCH)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2))


def normalise(desc):
    mu, sigma = channel_stats(desc)
    d = desc.reshape(len(desc), 3, PATCH * PATCH)
    return ((d - mu[None, :, None]) / sigma[None, :, None]).reshape(len(desc), DESC)


def sliced(A, B, dirs):
    """Mean over the repeats of mean |sort(A d) - sort(B d)| for dirs [repeats, 147, m], times 1e3."""
    vals = []
    for d in dirs:
        pa, pb = np.sort(A @ d, axis=0), np.sort(B @ d, axis=0)
        vals.append(np.mean(np.abs(pa - pb)))
    return float(np.mean(vals)) * 1e3


def swd(real, fake, draws, nhoods):
    """([value per level], average) for image sets [n, H, W, 3] and the draws of ``contrad_amd.swd.draws``'s layout."""
    pr, pf = pyramid(real, len(draws)), pyramid(fake, len(draws))
    vals = []
    for lv, a, b in zip(draws, pr, pf):
        A = normalise(descriptors(a, lv['real'], nhoods))
        B = normalise(descriptors(b, lv['fake'], nhoods))
        vals.append(sliced(A, B, np.asarray(lv['dirs'], np.float64)))
    return vals, float(np.mean(vals))


def projection_bound(desc, dirs, e_level):
    """The bound on |fp32 projection - float64 projection| (module docstring) for raw descriptors [n_desc, 147] of a level
    whose elementwise error is at most ``e_level`` and directions [repeats, 147, m]."""
    mu, sigma = channel_stats(desc)
    mu_k, sig_k = np.repeat(mu, PATCH * PATCH), np.repeat(sigma, PATCH * PATCH)
    E = float(e_level)
    assert np.all(sigma > 2 * E)
    r = E / (sigma.min() - E)
    worst = 0.0
    for d in dirs:
        w = np.abs(d / sig_k[:, None])                            # [147, m]
        s_abs = ((np.abs(desc) + E) @ w).max()
        s_cen = ((np.abs(desc - mu_k[None]) + 2 * E) @ w).max()
        s_w = w.sum(axis=0).max()
        host = 400 * 2.0 ** -53 * ((np.abs(desc) + np.abs(mu_k)[None]) @ w).max()
        worst = max(worst, gamma(148) * s_abs + (U + r) * (1 + U) * s_cen + 2 * E * s_w + host)
    return worst


def fsum_bound(n_terms, abs_sum):
    """|a float64 sum in any order - math.fsum| <= n 2^-53 sum |terms| (first order; n terms)."""
    return n_terms * 2.0 ** -53 * abs_sum


def absdiff_terms(A, B, off=None):
    a, b = np.asarray(A, np.float64), np.asarray(B, np.float64)
    t = a - b if off is None else (a - b) + np.asarray(off, np.float64)[:, None]
    return np.abs(t)


def fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


# ---- the synthetic sets of the property tests ----
def smooth_noise(n, size, seed, sigma=1.0):
    """n images [n, size, size, 3] uint8: uniform noise smoothed with a Gaussian of ``sigma`` per image and channel, rescaled
    to 0 ... 255 and floored."""
    r = np.random.RandomState(seed)
    x = ndimage.gaussian_filter(r.uniform(size=(n, size, size, 3)), (0, sigma, sigma, 0), mode='mirror')
    x = (x - x.min()) / (x.max() - x.min()) * 255.0
    return np.floor(x).clip(0, 255).astype(np.uint8)


def blurred(x_u8, sigma=1.5):
    x = ndimage.gaussian_filter(x_u8.astype(np.float64), (0, sigma, sigma, 0), mode='mirror')
    return np.floor(x).clip(0, 255).astype(np.uint8)
