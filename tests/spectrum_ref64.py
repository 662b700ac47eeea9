"""The yardstick of the radial power spectrum (contrad_amd/spectrum.py's docstring is the definition): numpy only, the full
S x S ``fft2`` in float64, bins found per frequency with ``math.isqrt``.  It shares no code with contrad_amd/spectrum.py, not
even the bin table, and it holds the error bound of the device transform -- derived here, never fitted to device output.

The bound.  |F_dev[u, v] - F[u, v]| <= gamma_m sum |Y| with gamma_m = m u / (1 - m u), u = 2^-24: every output is a sum of
S^2 terms Y[y, x] w, each carrying at most m factors (1 + delta), |delta| <= u.  m counts the longest chain of roundings of
csrc/spectral/spectrum.hip at side S = 2^k (the luma is exact and starts no chain):

  * a radix-2 stage of the decimation-in-time FFT costs 5: the twiddle's own rounding (1; the table is fp32 rounded from
    float64), the complex product (3: sqrt(2) gamma_2 <= gamma_3 in modulus, Higham 2002, 3.6) and the add (1).  Stages 0 and
    1 multiply by 1 and -i, which are sign swaps, so they cost the add alone: a pass of k stages costs c = 2 + 5 (k - 2).
  * the row pass packs two real rows into one complex transform and separates them with one more add (the halving is
    exact): r = c + 1.  Separation mixes the two rows: the error of row A's spectrum is bounded by
    gamma_r (sum |A| + sum |B|) / 2 + ..., i.e. by the row pair's sum, not the row's own.  Summed over all rows by the
    column pass each row's |Y| is counted twice, so the row pass weighs 2 r in a bound that is stated against sum |Y|.
  * m = 2 r + c = 15 k - 22: 38, 53, 68, 83, 98, 113 for S = 16 ... 512.

The condition m <= 2 S + 8 (what a plain two-pass matrix DFT needs) holds at every S: 40, 72, 136, 264, 520, 1032.

Propagated to the summary numbers (``tolerances``): |dP| <= (2 |F| e + e^2) / S^4 per entry with e the bound above, through
the bin mean and the mean over images to dA; dR <= (10 / ln 10) (dA_fake / A_fake + dA_real / A_real); the lsd moves by at most
the root mean square of the dR (triangle inequality of the 2-norm), hf by their mean over its band, a Nyquist point by
(10 / ln 10) (dM_fake / M_fake + dM_real / M_real).  The float64 sums on either side are some 1e-13 relative and are covered by
an absolute 1e-9 dB.

The two float64 reductions are compared with ``math.fsum`` of the very terms the device adds (``fsum``): both sides form a term
as the once-rounded x^2 + y^2 of the same fp32 pair (each square is exact in float64; a fused multiply-add rounds the same
value once), times the exact weight 1 or 2, so the terms are identical and only the sums differ.  radial: the owner of a bin
adds N half-spectrum members (N - 1 roundings), multiplies by the rounded reciprocal count (2 more; the 1 / S^4 is a power of
two); the reference rounds once in ``fsum`` and once in its division by the count: (N + 3) 2^-53 sum |terms|.  mean_map: any
order of adding n images, in chunks or not, has at most n - 1 roundings that matter (adding an empty partial is exact), the
reference has one: n 2^-53 sum |terms|.

The generator of the smooth sets (``smooth_noise``) is this file's own: every channel has its own noise, the filter is periodic
and the variance is normalised over the whole set.  The luma then averages three independent channels, so its high band holds
little but quantisation noise, and a given defect shows more strongly than on sets whose channels share one noise field: at
(24, 32) a checkerboard of +6 reads +48.9 dB at the corner and lsd 10.3 dB here, a sigma-1 blur hf -9.3 dB.  Figures quoted
elsewhere for another generator (31 ... 43 dB, 5.4 ... 7.6 dB, -2.1 ... -2.9 dB) are not in conflict with these.
"""
import math

import numpy as np

U32 = 2.0 ** -24
SIDES = (16, 32, 64, 128, 256, 512)
KMAX = {16: 11, 32: 23, 64: 45, 128: 91, 256: 181, 512: 362}
DB = 10.0 / math.log(10.0)

_bins = {}


def rounding_chain(S):
    """m of the module docstring."""
    k = int(S).bit_length() - 1
    assert 1 << k == S and S in SIDES
    return 15 * k - 22


def gamma(m):
    return m * U32 / (1.0 - m * U32)


def luma(x_u8):
    """[n, S, S, 3] uint8 -> float64 [n, S, S], exact."""
    x = np.asarray(x_u8).astype(np.int64)
    return (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2]).astype(np.float64) / 256.0


def fft_bound(x_u8):
    """[n]: the elementwise bound on |F_dev - F| per image."""
    Y = luma(x_u8)
    S = Y.shape[1]
    assert rounding_chain(S) <= 2 * S + 8
    return gamma(rounding_chain(S)) * np.abs(Y).sum(axis=(1, 2))


def rfft2(x_u8):
    """complex128 [n, S, S / 2 + 1] of the exact luma."""
    return np.fft.rfft2(luma(x_u8), axes=(1, 2))


def bins(S):
    """(int64 [S, S] full-grid bin table, K, counts [K])."""
    if S not in _bins:
        t = np.empty((S, S), np.int64)
        for u in range(S):
            fu = u if u <= S // 2 else u - S
            for v in range(S):
                fv = v if v <= S // 2 else v - S
                t[u, v] = (math.isqrt(4 * (fu * fu + fv * fv)) + 1) // 2
        K = int(t[S // 2, S // 2]) + 1
        assert int(t.max()) == K - 1
        _bins[S] = (t, K, np.bincount(t.ravel(), minlength=K))
    return _bins[S]


def bin_means(P):
    """[n, S, S] (full grid) -> [n, K]: the mean over the members of every bin."""
    S = P.shape[1]
    t, K, counts = bins(S)
    return np.stack([np.bincount(t.ravel(), weights=p.ravel(), minlength=K) / counts for p in P])


def spectrum(x_u8):
    """{'S', 'n', 'K', 'profiles' [n, K], 'mean' [K], 'map' [S, S / 2 + 1], and for the tolerances 'dmean', 'dmap'}."""
    Y = luma(x_u8)
    n, S = Y.shape[0], Y.shape[1]
    F = np.fft.fft2(Y, axes=(1, 2))
    P = (F.real ** 2 + F.imag ** 2) / float(S) ** 4
    e = fft_bound(x_u8)[:, None, None]
    dP = (2.0 * np.abs(F) * e + e * e) / float(S) ** 4
    prof = bin_means(P)
    return {'S': S, 'n': n, 'K': bins(S)[1], 'profiles': prof, 'mean': prof.mean(axis=0), 'map': P.mean(axis=0)[:, :S // 2 + 1],
            'dmean': bin_means(dP).mean(axis=0), 'dmap': dP.mean(axis=0)[:, :S // 2 + 1]}


def lsd(R):
    return float(np.sqrt(np.mean(np.square(R[1:]))))


def compare(real, fake):
    """Step 5 on two results of ``spectrum`` (or of anything with 'mean', 'map', 'S')."""
    S = real['S']
    R = 10.0 * np.log10(fake['mean'] / real['mean'])
    pts = ((0, S // 2), (S // 2, 0), (S // 2, S // 2))
    nyq = [float(10.0 * np.log10(fake['map'][p] / real['map'][p])) for p in pts]
    return {'R': R, 'lsd_db': lsd(R), 'hf_db': float(np.mean(R[S // 4 + 1:])), 'nyquist_db': nyq}


def floor_db(profiles):
    even, odd = profiles[0::2].mean(axis=0), profiles[1::2].mean(axis=0)
    return lsd(10.0 * np.log10(odd / even))


def tolerances(real, fake):
    """{'R': [K], 'lsd_db', 'hf_db', 'nyquist_db': [3]}: the propagated bounds of the module docstring, in dB."""
    S = real['S']
    dR = DB * (fake['dmean'] / fake['mean'] + real['dmean'] / real['mean']) + 1e-9
    pts = ((0, S // 2), (S // 2, 0), (S // 2, S // 2))
    nyq = [float(DB * (fake['dmap'][p] / fake['map'][p] + real['dmap'][p] / real['map'][p]) + 1e-9) for p in pts]
    return {'R': dR, 'lsd_db': float(np.sqrt(np.mean(np.square(dR[1:])))), 'hf_db': float(np.mean(dR[S // 4 + 1:])), 'nyquist_db': nyq}


def fsum(values):
    """The exactly rounded sum of float64 values (``math.fsum``)."""
    return math.fsum(np.asarray(values, np.float64).ravel().tolist())


def fsum_bound(terms, abs_sum):
    """terms 2^-53 sum |terms|: what ``terms`` roundings of relative size 2^-53 can move a sum of non-negative values by (to first
    order; the second-order part is below 1e-13 of it at the counts used here)."""
    return terms * 2.0 ** -53 * abs_sum


def half_members(S):
    """(int64 [S, S / 2 + 1] bin of every half-spectrum entry, [K] how many of them each bin has): the values that the owner of
    a bin really adds, about half of the full-grid count."""
    t, K, _counts = bins(S)
    half = np.ascontiguousarray(t[:, :S // 2 + 1])
    return half, np.bincount(half.ravel(), minlength=K)


# ---- inputs ----
def _gauss_wrap(z, sigma):
    """Separable Gaussian filter along axes 1 and 2 with periodic boundary, radius 4 sigma."""
    r = int(math.ceil(4 * sigma))
    g = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    g /= g.sum()
    for axis in (1, 2):
        z = sum(w * np.roll(z, d, axis=axis) for w, d in zip(g, range(-r, r + 1)))
    return z


def _to_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def smooth_noise(n, S, seed):
    """uint8 [n, S, S, 3]: Gaussian-filtered white noise (sigma 1.5, every channel its own), scaled to unit variance over the
    set, as 128 + 50 z, rounded and clipped."""
    z = _gauss_wrap(np.random.RandomState(seed).randn(n, S, S, 3), 1.5)
    return _to_u8(128.0 + 50.0 * z / z.std())


def uniform_noise(n, S, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, S, S, 3)).astype(np.uint8)


def checkerboarded(x_u8, amount=6):
    """+amount on the pixels with x + y even, clipped."""
    S = x_u8.shape[1]
    even = ((np.arange(S)[:, None] + np.arange(S)[None, :]) % 2 == 0)[None, :, :, None]
    return np.clip(x_u8.astype(np.int64) + amount * even, 0, 255).astype(np.uint8)


def blurred(x_u8, sigma=1.0):
    return _to_u8(_gauss_wrap(x_u8.astype(np.float64), sigma))
