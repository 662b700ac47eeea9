"""The kernels of csrc/spectral/spectrum.hip on the GPU, each alone, against the yardstick (tests/spectrum_ref64.py).  Every
output sits in guard storage (NaN outside); the kernels take no scratch, so that is the whole memory contract.

Bounds (derived, not measured; tests/spectrum_ref64.py's docstring).  rfft2: elementwise |F_dev - F| <= gamma_m sum |Y| against
``numpy.fft.rfft2`` of the exact luma in float64, m = 15 log2 S - 22.  radial and mean_map: against float64 numpy on the device's
own fp32 spectrum against ``math.fsum`` of the very terms the device adds, so the only differences are the orders of float64 sums:
terms 2^-53 sum |terms| with terms the number of values the owner really adds -- N + 3 for a radial bin of N half-spectrum
members (3: the rounded reciprocal count, its product, the reference's division), n for an entry of the mean map over n images.
Every figure goes through ``margin`` (conftest.py), which keeps the observed error next to the bound.

Observed on the MI355X (profiles/spectrum.txt): the transform's worst error per size is 0.004 ... 0.019 of its bound on noise
and 0.004 ... 0.024 on smooth inputs; radial stays below 0.36 and mean_map below 0.52 of theirs; the closed forms' zeros are exact."""
import ctypes

import numpy as np
import pytest
import torch

import spectrum_ref64 as R

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float('nan')
EINVAL = -22


def _guarded(shape, dtype=torch.float32):
    """(view, check): a contiguous tensor of ``shape`` inside NaN guard bands; ``check()`` asserts the bands are untouched."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), NAN, device='cuda', dtype=dtype)

    def check():
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + numel:]).all())
    return flat[GUARD:GUARD + numel].view(*shape), check


def _tables(S):
    from contrad_amd import spectrum
    return spectrum.device_tables(S, torch.device('cuda', 0))


def _rfft2(x):
    """The device transform of a host uint8 set as complex128 [n, S, S / 2 + 1], from guarded storage."""
    from contrad_amd import ops
    n, S = x.shape[0], x.shape[1]
    out, check = _guarded((n, S, S // 2 + 1, 2))
    ops.spec_rfft2(torch.from_numpy(x).cuda(), _tables(S)[0], out=out)
    torch.cuda.synchronize()
    check()
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    return got[..., 0] + 1j * got[..., 1]


_inputs = {}


def _input(n, S, kind):
    key = (n, S, kind)
    if key not in _inputs:
        x = R.uniform_noise(n, S, 7 * n + S) if kind == 'noise' else R.smooth_noise(n, S, 7 * n + S)
        x[0, 0, 0] = 255; x[-1, -1, -1] = 0; x[-1, 0, -1] = 255                  # the corners carry weight
        _inputs[key] = (x, R.rfft2(x), R.fft_bound(x))
    return _inputs[key]


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
@pytest.mark.parametrize('n,S', [(1, 16), (5, 16), (3, 32), (7, 32), (2, 64), (1, 128), (3, 128), (2, 256), (1, 512), (3, 512)])
def test_rfft2_against_numpy_within_the_bound(margin, n, S, kind):
    x, want, bound = _input(n, S, kind)
    got = _rfft2(x)
    assert got.shape == want.shape
    err = np.abs(got - want).max(axis=(1, 2))
    ratio = float((err / bound).max())
    print('rfft2 %dx%d %s: worst |F_dev - F| / bound = %.4f (m = %d)' % (n, S, kind, ratio, R.rounding_chain(S)))
    margin('spectrum rfft2 S=%d %s n=%d' % (S, kind, n), ratio, 1.0)
    assert float(np.abs(want).max()) > 100.0 * float(bound.max())               # (the bound sits far below the signal)


@pytest.mark.parametrize('S', [16, 256])
def test_rfft2_closed_forms(margin, S):
    x = np.zeros((5, S, S, 3), np.uint8)
    x[0, 3, 5] = 255                                                         # one pixel of 255 at (y, x) = (3, 5)
    x[1] = 201                                                               # constant
    x[2, :, 1::2] = 255                                                      # columns alternate along x
    x[3, 1::2, :] = 255                                                      # rows alternate along y
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    x[4][(yy + xx) % 2 == 1] = 255                                           # checkerboard
    got, bound = _rfft2(x), R.fft_bound(x)
    h = S // 2
    margin('spectrum one pixel S=%d' % S, np.abs(np.abs(got[0]) - 255.0).max(), bound[0])
    u, v = np.arange(S)[:, None], np.arange(h + 1)[None, :]
    margin('spectrum one pixel phase S=%d' % S, np.abs(got[0] - 255.0 * np.exp(-2j * np.pi * (3 * u + 5 * v) / S)).max(), bound[0])
    for i, peaks in ((1, [(0, 0)]), (2, [(0, 0), (0, h)]), (3, [(0, 0), (h, 0)]), (4, [(0, 0), (h, h)])):
        rest = np.abs(got[i]).copy()
        for p in peaks:
            assert rest[p] > 0.4 * 255.0 * S * S - bound[i], (i, p)
            rest[p] = 0.0
        margin('spectrum closed form %d S=%d: everything off the peaks' % (i, S), rest.max(), bound[i])
    margin('spectrum constant DC S=%d' % S, abs(got[1][0, 0] - 201.0 * S * S), bound[1])


def _half_weights(S):
    w = np.full((S, S // 2 + 1), 2.0)
    w[:, 0] = w[:, S // 2] = 1.0
    return w


def _radial_ref(spec64, S):
    """([n, K] float64, [K] terms of the tolerance) from a complex128 half spectrum: ``math.fsum`` of every bin's weighted
    |F|^2 over its half-spectrum members (the yardstick's bins), divided by the full-grid count and by S^4."""
    _full, K, counts = R.bins(S)
    half, members = R.half_members(S)
    order = np.argsort(half.ravel(), kind='stable')
    ends = np.cumsum(members)
    terms = (spec64.real ** 2 + spec64.imag ** 2) * _half_weights(S)           # (the device's terms, bit for bit)
    prof = np.empty((terms.shape[0], K))
    for i, t in enumerate(terms):
        t = t.ravel()[order]
        for k in range(K):
            prof[i, k] = R.fsum(t[ends[k] - members[k]:ends[k]]) / counts[k] / float(S) ** 4
    return prof, members + 3


def _device_spec(n, S, kind='noise'):
    from contrad_amd import ops
    x = _input(n, S, kind)[0]
    spec = ops.spec_rfft2(torch.from_numpy(x).cuda(), _tables(S)[0])
    host = spec.cpu().numpy().astype(np.float64)
    return spec, host[..., 0] + 1j * host[..., 1]


def _edge_columns_spec(n, S):
    """A spectrum whose only energy is in the columns v = 0 and v = S / 2."""
    r = np.random.RandomState(S)
    host = np.zeros((n, S, S // 2 + 1, 2), np.float32)
    host[:, :, 0] = r.randn(n, S, 2) * 50
    host[:, :, S // 2] = r.randn(n, S, 2) * 50
    h64 = host.astype(np.float64)
    return torch.from_numpy(host).cuda(), h64[..., 0] + 1j * h64[..., 1]


@pytest.mark.parametrize('n,S,source', [(7, 16, 'fft'), (7, 32, 'fft'), (3, 64, 'fft'), (2, 128, 'fft'), (2, 256, 'fft'), (1, 512, 'fft'),
                                        (3, 16, 'edges'), (2, 256, 'edges')])
def test_radial_against_float64_on_the_devices_spec(margin, n, S, source):
    from contrad_amd import ops
    spec, host = _device_spec(n, S) if source == 'fft' else _edge_columns_spec(n, S)
    _tw, bins, rcount = _tables(S)
    want, terms = _radial_ref(host, S)
    K = want.shape[1]
    runs = []
    for _ in range(2):
        out, check = _guarded((n, K), torch.float64)
        ops.spec_radial(spec, bins, rcount, out=out)
        torch.cuda.synchronize()
        check()
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))      # two calls: bitwise equal
    tol = R.fsum_bound(terms[None, :], want)
    assert np.all(np.abs(runs[0] - want)[tol == 0] == 0)
    live = tol > 0
    assert live.sum() >= (n * K if source == 'fft' else n * (S // 2 + 1))
    margin('spectrum radial %dx%d %s' % (n, S, source), float((np.abs(runs[0] - want)[live] / tol[live]).max()), 1.0)
    if source == 'edges':                                                    # weight 1 there: twice the plain sum would show
        P = (host.real ** 2 + host.imag ** 2) / float(S) ** 4
        assert np.allclose(runs[0][:, 0], P[:, 0, 0], rtol=1e-14)
        full, _K, counts = R.bins(S)
        assert np.allclose((runs[0] * counts).sum(axis=1), P.sum(axis=(1, 2)), rtol=1e-12)


@pytest.mark.parametrize('n,S,source', [(7, 16, 'fft'), (7, 32, 'fft'), (7, 64, 'fft'), (7, 128, 'fft'), (7, 256, 'fft'), (7, 512, 'edges'),
                                        (70, 16, 'edges')])
def test_mean_map_against_float64_and_in_chunks(margin, n, S, source):
    from contrad_amd import ops
    spec, host = _device_spec(n, S) if source == 'fft' else _edge_columns_spec(n, S)
    terms = (host.real ** 2 + host.imag ** 2) / float(S) ** 4                  # (S^4 is a power of two: exact)
    E = S * (S // 2 + 1)
    want = np.array([R.fsum(col) for col in terms.reshape(n, E).T]).reshape(S, S // 2 + 1)
    tol = R.fsum_bound(n, want)
    runs = []
    for _ in range(2):
        out, check = _guarded((S, S // 2 + 1), torch.float64)
        ops.spec_mean_map(spec, out=out)
        torch.cuda.synchronize()
        check()
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))      # two calls: bitwise equal
    out, check = _guarded((S, S // 2 + 1), torch.float64)
    ops.spec_mean_map(spec[:3], out=out)                                     # images 0 ... 2, then 3 ... n - 1
    ops.spec_mean_map(spec[3:], out=out, accumulate=True)
    torch.cuda.synchronize()
    check()
    for name, got in (('one call', runs[0]), ('two chunks', out.cpu().numpy())):
        assert np.all(np.abs(got - want)[tol == 0] == 0)
        live = tol > 0
        margin('spectrum mean_map %dx%d %s %s' % (n, S, source, name), float((np.abs(got - want)[live] / tol[live]).max()), 1.0)
    with pytest.raises(RuntimeError):
        ops.spec_mean_map(spec, accumulate=True)


def test_rfft2_twice_is_bitwise_equal():
    from contrad_amd import ops
    for n, S in ((5, 16), (2, 64), (2, 256)):
        x = torch.from_numpy(R.uniform_noise(n, S, 1)).cuda()
        a, b = ops.spec_rfft2(x, _tables(S)[0]), ops.spec_rfft2(x, _tables(S)[0])
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def test_c_entry_points_refuse_before_a_launch():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    S, n = 16, 2
    tw, bins, rcount = _tables(S)
    K = int(rcount.shape[0])
    x = torch.zeros(n, S, S, 3, dtype=torch.uint8, device='cuda')
    spec, cs = _guarded((n, S, S // 2 + 1, 2))
    prof, cp = _guarded((n, K), torch.float64)
    mp, cm = _guarded((S, S // 2 + 1), torch.float64)
    p, ll, st = ops._p, ctypes.c_longlong, ops._stream()
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    rfft2, radial, mean_map = (lib().raw('contrad_spec_' + k) for k in ('rfft2', 'radial', 'mean_map'))
    assert rfft2(p(x), p(tw), p(spec), ll(n), S, st) == 0
    for args in ((None, p(tw), p(spec), ll(n), S), (p(x), None, p(spec), ll(n), S), (p(x), p(tw), None, ll(n), S),
                 (p(x), p(tw), p(spec), ll(0), S), (p(x), p(tw), p(spec), ll(-1), S), (p(x), p(tw), p(spec), ll((1 << 24) + 1), S),
                 (p(x), p(tw), p(spec), ll(n), 8), (p(x), p(tw), p(spec), ll(n), 24), (p(x), p(tw), p(spec), ll(n), 1024),
                 (p(x), p(tw), p(spec), ll(n), 0), (off(x, 1), p(tw), p(spec), ll(1), S), (p(x), off(tw, 4), p(spec), ll(n), S),
                 (p(x), p(tw), off(spec, 4), ll(1), S)):
        assert rfft2(*(args + (st,))) == EINVAL, args
    assert radial(p(spec), ops._as_int(bins), p(rcount), p(prof), ll(n), S, K, st) == 0
    for args in ((None, ops._as_int(bins), p(rcount), p(prof), ll(n), S, K), (p(spec), None, p(rcount), p(prof), ll(n), S, K),
                 (p(spec), ops._as_int(bins), None, p(prof), ll(n), S, K), (p(spec), ops._as_int(bins), p(rcount), None, ll(n), S, K),
                 (p(spec), ops._as_int(bins), p(rcount), p(prof), ll(0), S, K), (p(spec), ops._as_int(bins), p(rcount), p(prof), ll(n), 48, K),
                 (p(spec), ops._as_int(bins), p(rcount), p(prof), ll(n), S, S // 2), (p(spec), ops._as_int(bins), p(rcount), p(prof), ll(n), S, S + 1),
                 (off(spec, 4), ops._as_int(bins), p(rcount), p(prof), ll(1), S, K), (p(spec), ops._as_int(bins), off(rcount, 4), p(prof), ll(n), S, K),
                 (p(spec), ops._as_int(bins), p(rcount), off(prof, 4), ll(1), S, K)):
        assert radial(*(args + (st,))) == EINVAL, args
    assert mean_map(p(spec), p(mp), ll(n), S, 0, st) == 0
    for args in ((None, p(mp), ll(n), S, 0), (p(spec), None, ll(n), S, 0), (p(spec), p(mp), ll(0), S, 0), (p(spec), p(mp), ll(n), 20, 0),
                 (p(spec), p(mp), ll(n), S, 2), (p(spec), p(mp), ll(n), S, -1), (off(spec, 4), p(mp), ll(1), S, 0),
                 (p(spec), off(mp, 4), ll(n), S, 0)):
        assert mean_map(*(args + (st,))) == EINVAL, args
    torch.cuda.synchronize()
    cs(); cp(); cm()


def test_wrappers_refuse_bad_tensors():
    from contrad_amd import ops
    tw, bins, rcount = _tables(16)
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device='cuda')
    spec = ops.spec_rfft2(x, tw)
    assert tuple(spec.shape) == (2, 16, 9, 2) and not bool(spec.any())
    for bad in (lambda: ops.spec_rfft2(x.cpu(), tw), lambda: ops.spec_rfft2(x.float(), tw), lambda: ops.spec_rfft2(x[:, :, :8], tw),
                lambda: ops.spec_rfft2(x[:0], tw), lambda: ops.spec_rfft2(x[..., :2], tw), lambda: ops.spec_rfft2(x, tw[:4]),
                lambda: ops.spec_rfft2(x, tw.double()), lambda: ops.spec_rfft2(x, tw.cpu()), lambda: ops.spec_rfft2(x, _tables(32)[0]),
                lambda: ops.spec_rfft2(torch.zeros(1, 24, 24, 3, dtype=torch.uint8, device='cuda'), tw),
                lambda: ops.spec_rfft2(x, tw, out=spec[:1]), lambda: ops.spec_rfft2(x, tw, out=spec.double()),
                lambda: ops.spec_radial(spec.double(), bins, rcount), lambda: ops.spec_radial(spec[:, :8], bins, rcount),
                lambda: ops.spec_radial(spec, bins.long(), rcount), lambda: ops.spec_radial(spec, bins[:8], rcount),
                lambda: ops.spec_radial(spec, bins, rcount.float()), lambda: ops.spec_radial(spec, bins, rcount[:8]),
                lambda: ops.spec_radial(spec, bins, rcount, out=torch.zeros(2, 12, device='cuda')),
                lambda: ops.spec_mean_map(spec.cpu()), lambda: ops.spec_mean_map(spec[..., 0]),
                lambda: ops.spec_mean_map(spec, out=torch.zeros(16, 9, device='cuda')),
                lambda: ops.spec_mean_map(spec, out=torch.zeros(9, 16, device='cuda', dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            bad()
