"""The kernels of csrc/latent/latent.hip on the GPU, each alone, against the yardstick (tests/latent_ref64.py).  Every output
sits in guard storage (NaN outside); the kernels take no scratch, so that is the whole memory contract.

Bounds (derived, not measured; tests/latent_ref64.py's docstring).  latent_pair: every element within
2^-24 |ref| + (d + 16) 2^-52 max(1, |a|_inf, |b|_inf); with dt = 0 the second point is bitwise the first; rows b = +-a are degenerate
by the yardstick's rule |r| <= (d + 16) 2^-52 (for b = -a the computed r is rounding noise, never exactly 0).  latent_styles: bitwise
the source without psi, within 3 2^-24 (|w_avg| + |psi| (|src| + |w_avg|)) with it.  pair_dist: within
scale [(d + 8) u (4 D + D^2) + 8 ((d + 8) u)^2], u = 2^-53, against np.longdouble.  Every figure goes through ``margin``
(conftest.py), which keeps the observed error next to the bound.

Observed on the MI355X: profiles/ppl.txt."""
import ctypes

import numpy as np
import pytest
import torch

import latent_ref64 as R

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


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- latent_pair ----
_pair_inputs = {}


def _pair_input(n, d):
    """fp32 rows a, b [n + 3, d]: n random rows, then b = a, b = -a and b = a (1 + 1e-6 r); and the four t vectors."""
    if (n, d) not in _pair_inputs:
        g = np.random.RandomState(100 * n + d)
        a, b = g.randn(n + 3, d), g.randn(n + 3, d)
        a[0] *= 30.0                                                  # (norms far from 1)
        b[n] = a[n]
        b[n + 1] = -a[n + 1]
        b[n + 2] = a[n + 2] * (1.0 + 1e-6 * g.randn(d))
        ts = [np.full(n + 3, v, np.float32) for v in (0.0, 1.0, 0.5)] + [g.rand(n + 3).astype(np.float32)]
        _pair_inputs[(n, d)] = (a.astype(np.float32), b.astype(np.float32), ts)
    return _pair_inputs[(n, d)]


def _latent_pair(a, b, t, dt, mode):
    from contrad_amd import ops
    o0, c0 = _guarded(a.shape)
    o1, c1 = _guarded(a.shape)
    ops.latent_pair(_dev(a), _dev(b), _dev(t), dt, mode, out0=o0, out1=o1)
    torch.cuda.synchronize()
    c0()
    c1()
    return o0.cpu().numpy(), o1.cpu().numpy()


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('dt', [0.0, 1e-4])
@pytest.mark.parametrize('n,d', [(1, 2), (3, 128), (2, 130), (5, 512), (70, 512)])
def test_latent_pair_against_the_yardstick(margin, n, d, dt, mode):
    a, b, ts = _pair_input(n, d)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for t, what in zip(ts, ('0', '1', '0.5', 'random')):
        g0, g1 = _latent_pair(a, b, t, dt, mode)
        assert np.all(np.isfinite(g0)) and np.all(np.isfinite(g1))
        w0, w1 = R.pair(a64, b64, t, dt, mode)
        worst, off = 0.0, 0
        for got, want in ((g0, w0), (g1, w1)):
            ratio = np.abs(got.astype(np.float64) - want) / R.pair_bound(want, a64, b64)
            worst = max(worst, float(ratio.max()))
            off += int((got.view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())
        # (the fp32 rounding of the result alone can reach the first term of the bound; `off` counts what the float64 chain moved)
        print('latent_pair %dx%d mode %d dt %g t %s: worst error / bound = %.4f, %d of %d elements are not the rounded yardstick'
              % (n, d, mode, dt, what, worst, off, 2 * g0.size))
        margin('latent_pair n=%d d=%d mode=%d dt=%g t=%s' % (n, d, mode, dt, what), worst, 1.0)
        if dt == 0.0:
            assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
        else:
            assert not np.array_equal(g0[:n], g1[:n])
        if mode == 1:
            # b = +-a: one point for every t, hence the same bits at both ends; every point on the unit sphere
            assert np.array_equal(g0[n:n + 2].view(np.uint32), g1[n:n + 2].view(np.uint32))
            assert np.abs(np.linalg.norm(g0.astype(np.float64), axis=1) - 1.0).max() < d * 2.0 ** -24


def test_latent_pair_steps_by_exactly_eps():
    """The reason for the kernel: the two ends differ by dt in t although fp32(t) + fp32(dt) would not.  In lerp mode the
    difference of the two outputs is dt (b - a) to the fp32 rounding of the outputs themselves."""
    g = np.random.RandomState(5)
    a, b = g.randn(4, 512).astype(np.float32), g.randn(4, 512).astype(np.float32)
    t = np.float32([0.0, 0.3, 0.7, 0.999])
    g0, g1 = _latent_pair(a, b, t, 1e-4, 0)
    step = g1.astype(np.float64) - g0.astype(np.float64)
    want = 1e-4 * (b.astype(np.float64) - a.astype(np.float64))
    assert np.abs(step - want).max() <= 2.0 * 2.0 ** -24 * max(np.abs(a).max(), np.abs(b).max())


def test_latent_pair_refusals():
    from contrad_amd import _lib, ops
    raw = _lib.lib().raw('contrad_latent_pair')
    a = torch.zeros(2, 8, device='cuda')
    t = torch.zeros(2, device='cuda')
    o0, o1 = torch.empty_like(a), torch.empty_like(a)
    p = ops._p
    n2 = ctypes.c_longlong(2)
    assert raw(p(a), p(a), p(t), 0.0, 0, p(o0), p(o1), n2, 8, None) == 0
    assert raw(None, p(a), p(t), 0.0, 0, p(o0), p(o1), n2, 8, None) == EINVAL
    assert raw(p(a), p(a), p(t), 0.0, 2, p(o0), p(o1), n2, 8, None) == EINVAL
    assert raw(p(a), p(a), p(t), 0.0, 0, p(o0), p(o1), ctypes.c_longlong(0), 8, None) == EINVAL
    assert raw(p(a), p(a), p(t), 0.0, 0, p(o0), p(o1), n2, 0, None) == EINVAL
    assert raw(p(a), p(a), p(t), float('nan'), 0, p(o0), p(o1), n2, 8, None) == EINVAL
    assert raw(p(a), p(a), p(t), 0.0, 0, p(o0), p(o0), n2, 8, None) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.latent_pair(a, a[:, :4], t, 0.0, 0)
    with pytest.raises(ValueError):
        ops.latent_pair(a, a, t, 0.0, 3)


# ---- latent_styles ----
def _styles_input(B, L, d):
    g = np.random.RandomState(B * 1000 + L * 10 + d)
    w, w2, w_avg = (g.randn(B, d).astype(np.float32), g.randn(B, d).astype(np.float32), g.randn(d).astype(np.float32))
    psi = g.uniform(-0.5, 1.5, L).astype(np.float32)
    psi[0] = 0.7
    psi[-1] = 1.0 if L > 1 else psi[-1]
    cross = g.randint(0, L + 1, B).astype(np.float32)
    cross[0] = 0.0
    cross[-1] = float(L)
    return w, w2, w_avg, psi, cross


def _latent_styles(w, L, **kw):
    from contrad_amd import ops
    out, check = _guarded((w.shape[0], L, w.shape[1]))
    ops.latent_styles(_dev(w), L, out=out, **{k: _dev(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    check()
    return out.cpu().numpy()


@pytest.mark.parametrize('B,L,d', [(1, 1, 4), (3, 8, 512), (5, 16, 130)])
def test_latent_styles_against_the_yardstick(margin, B, L, d):
    w, w2, w_avg, psi, cross = _styles_input(B, L, d)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)        # noqa: E731
    rows_w, rows_w2 = np.repeat(w[:, None], L, 1), np.repeat(w2[:, None], L, 1)
    assert np.array_equal(bits(_latent_styles(w, L)), bits(rows_w))  # no mixing, no truncation: the rows themselves
    mix = _latent_styles(w, L, w2=w2, cross=cross)
    _, src = R.styles(w, L, w2, cross)
    assert np.array_equal(bits(mix), bits(src))
    assert np.array_equal(bits(_latent_styles(w, L, w2=w2, cross=np.zeros(B, np.float32))), bits(rows_w2))        # cross = 0: w2
    assert np.array_equal(bits(_latent_styles(w, L, w2=w2, cross=np.full(B, L, np.float32))), bits(rows_w))      # cross = L: w
    for kw in (dict(), dict(w2=w2, cross=cross)):
        got = _latent_styles(w, L, w_avg=w_avg, psi=psi, **kw)
        want, src = R.styles(w, L, kw.get('w2'), kw.get('cross'), w_avg, psi)
        ratio = float((np.abs(got.astype(np.float64) - want) / R.styles_bound(src, w_avg, psi)).max())
        print('latent_styles %dx%dx%d mixing %s: worst error / bound = %.4f' % (B, L, d, bool(kw), ratio))
        margin('latent_styles B=%d L=%d d=%d mix=%d' % (B, L, d, bool(kw)), ratio, 1.0)
        if L > 1:
            assert np.array_equal(bits(got[:, -1]), bits(src[:, -1]))              # psi = 1: the source's bits
    zero = _latent_styles(w, L, w_avg=w_avg, psi=np.zeros(L, np.float32))
    assert np.array_equal(bits(zero), bits(np.broadcast_to(w_avg, (B, L, d))))     # psi = 0: w_avg's bits


def test_latent_styles_refusals():
    from contrad_amd import _lib, ops
    raw = _lib.lib().raw('contrad_latent_styles')
    p = ops._p
    w, c, m, s = torch.zeros(2, 8, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(8, device='cuda'), torch.ones(3, device='cuda')
    out = torch.empty(2, 3, 8, device='cuda')
    assert raw(p(w), p(w), p(m), p(s), p(c), p(out), 2, 3, 8, None) == 0
    assert raw(None, None, None, None, None, p(out), 2, 3, 8, None) == EINVAL
    assert raw(p(w), p(w), None, None, None, p(out), 2, 3, 8, None) == EINVAL         # w2 without cross
    assert raw(p(w), None, None, None, p(c), p(out), 2, 3, 8, None) == EINVAL
    assert raw(p(w), None, p(m), None, None, p(out), 2, 3, 8, None) == EINVAL         # w_avg without psi
    assert raw(p(w), None, None, p(s), None, p(out), 2, 3, 8, None) == EINVAL
    assert raw(p(w), None, None, None, None, p(out), 0, 3, 8, None) == EINVAL
    assert raw(p(w), None, None, None, None, p(out), 2, 0, 8, None) == EINVAL
    assert raw(p(w), None, None, None, None, p(out), 2, 3, 0, None) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.latent_styles(w, 3, w2=w)


# ---- pair_dist ----
def _resident_d():
    from contrad_amd import ops
    return ops.pair_dist_resident_d()


def _pair_dist(A, B, scale, ld=None):
    """From guarded output storage; ``ld``: the rows sit in a wider matrix whose other columns are NaN."""
    from contrad_amd import ops
    n, d = A.shape
    out, check = _guarded((n,), torch.float64)
    if ld is None:
        a, b = _dev(A), _dev(B)
    else:
        a = torch.full((n, ld), NAN, device='cuda')
        b = torch.full((n, ld + 3), NAN, device='cuda')
        a[:, :d] = _dev(A)
        b[:, :d] = _dev(B)
        a, b = a[:, :d], b[:, :d]
    ops.pair_dist(a, b, scale, out=out)
    torch.cuda.synchronize()
    check()
    return out.cpu().numpy()


def _dist_shapes():
    return [(1, 1), (3, 130), (5, 512), (2, 8192), (2, _resident_d() + 1)]


@pytest.mark.parametrize('kind', ['random', 'near'])
@pytest.mark.parametrize('shape', range(5))
def test_pair_dist_against_the_yardstick(margin, shape, kind):
    n, d = _dist_shapes()[shape]
    assert _resident_d() >= 8192
    g = np.random.RandomState(17 * n + d)
    A = (g.randn(n, d) * 3.0).astype(np.float32)
    if kind == 'random':
        B, scale = g.randn(n, d).astype(np.float32), 2.5
    else:                                                             # the case the similarity form cannot do
        B, scale = (A.astype(np.float64) * (1.0 + 1e-7 * g.randn(n, d))).astype(np.float32), 1e8
    want = R.pair_dist(A, B, scale)
    bound = R.pair_dist_bound(want, d, scale)
    for ld in (None, d + 5):
        got = _pair_dist(A, B, scale, ld)
        ratio = float((np.abs(got - want) / bound).max())
        print('pair_dist %dx%d %s ld %s: worst error / bound = %.4f (values %.3e ... %.3e)' % (n, d, kind, ld, ratio, want.min(), want.max()))
        margin('pair_dist n=%d d=%d %s ld=%s' % (n, d, kind, ld), ratio, 1.0)
    if kind == 'near' and d > 1:
        assert want.min() > 0.0                                       # (fp32 rows 1e-7 apart do differ)


@pytest.mark.parametrize('shape', range(5))
def test_pair_dist_exact_cases(margin, shape):
    n, d = _dist_shapes()[shape]
    g = np.random.RandomState(d)
    A = g.randn(n, d).astype(np.float32)
    assert np.array_equal(_pair_dist(A, A.copy(), 1e8), np.zeros(n))            # A == B: exactly 0
    from contrad_amd import ops
    a = _dev(A)
    assert np.array_equal(ops.pair_dist(a, a, 1e8).cpu().numpy(), np.zeros(n))  # the same storage
    unit = g.randn(n, d)
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
    got = _pair_dist(np.zeros((n, d), np.float32), unit, 7.0)                   # a zero row against a unit row: scale
    want = R.pair_dist(np.zeros((n, d), np.float32), unit, 7.0)
    margin('pair_dist zero row d=%d' % d, float((np.abs(got - want) / R.pair_dist_bound(want, d, 7.0)).max()), 1.0)
    assert np.all(np.abs(got - 7.0) <= R.pair_dist_bound(np.full(n, 7.0), d, 7.0))


def test_pair_dist_keeps_what_the_similarity_form_cancels():
    """Rows 1e-4 apart relatively: 2 - 2 s from fp32 unit rows is off by orders of magnitude, the difference form is not."""
    g = np.random.RandomState(3)
    A = g.randn(4, 512).astype(np.float32)
    B = (A.astype(np.float64) * (1.0 + 1e-4 * g.randn(4, 512))).astype(np.float32)
    want = R.pair_dist(A, B, 1e8)
    got = _pair_dist(A, B, 1e8)
    assert np.abs(got - want).max() <= R.pair_dist_bound(want, 512, 1e8).max()
    an, bn = torch.nn.functional.normalize(_dev(A)), torch.nn.functional.normalize(_dev(B))
    sim = (2.0 - 2.0 * (an * bn).sum(1)).double().cpu().numpy() * 1e8
    assert np.abs(sim - want).max() > 1e3 * np.abs(got - want).max()


def test_pair_dist_refusals():
    from contrad_amd import _lib, ops
    raw = _lib.lib().raw('contrad_pair_dist')
    p = ops._p
    A = torch.zeros(2, 8, device='cuda')
    out = torch.empty(3, device='cuda', dtype=torch.float64)
    ll = ctypes.c_longlong
    assert raw(p(A), ll(8), p(A), ll(8), ll(2), 8, 1.0, p(out), None) == 0
    assert raw(None, ll(8), p(A), ll(8), ll(2), 8, 1.0, p(out), None) == EINVAL
    assert raw(p(A), ll(7), p(A), ll(8), ll(2), 8, 1.0, p(out), None) == EINVAL
    assert raw(p(A), ll(8), p(A), ll(7), ll(2), 8, 1.0, p(out), None) == EINVAL
    assert raw(p(A), ll(8), p(A), ll(8), ll(0), 8, 1.0, p(out), None) == EINVAL
    assert raw(p(A), ll(8), p(A), ll(8), ll(2), 0, 1.0, p(out), None) == EINVAL
    assert raw(p(A), ll(8), p(A), ll(8), ll(2), 8, float('inf'), p(out), None) == EINVAL
    assert raw(p(A), ll(8), p(A), ll(8), ll(2), 8, 1.0, ctypes.c_void_p(out.data_ptr() + 4), None) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.pair_dist(A, A[:, :4])
    with pytest.raises(RuntimeError):
        ops.pair_dist(A, A.double())
