"""The kernel distance on the GPU against the yardstick (tests/kid_ref64.py): ``contrad_kid_sums`` alone on a given S,
``kid`` on the device's own similarities and against float64 features, ``kid_of`` through a discriminator, the command
line and ``--prdc_kid`` / ``--prdc_best kid`` of the training scripts (which must not move the trajectory by a bit, nor a
byte of ``prdc_<seed>.csv``).

Bounds.  On a given fp32 S the device sum must lie within ``bound = (M n + 16) 2^-53 sum (|gamma s| + |coef0|)^3`` of the
``math.fsum`` of the float64 terms: any summation order and a fused multiply-add are inside it, one dropped or doubled
element is far outside (a typical term is about 1, the bound about 1e-16 M n times the sum).  On features a device
similarity is within e = (2 d + 8) 2^-24 of the float64 one (derived at the head of tests/test_knn_gpu.py) and
|k'| <= 3 (2 + e)^2 on [-1 - e, 1 + e], so every MMD2_t, a combination of means of k with weights 1, 1 and -2, moves by
at most 4 * 3 (2 + e)^2 e, and so does their mean: |kid_dev - kid_ref| <= 12 (2 + e)^2 e = 1.6e-4, 3.0e-3, 4.7e-2 at
d = 24, 512, 8192.  That is a condition, not the expected error: the inputs are chosen so that the float64 KID is at least
ten times the bound (0.47 - 0.89 here).

Observed on the MI355X (the tests print every figure before they assert): kernel on a given S
|out - fsum| <= 4.7e-10 on a sum of 2.55e6 and at most 0.02 of the bound; sums on the device's own S at most 1.3e-4 of the
bound; |kid_dev - kid_ref| 1.3e-8, 7.8e-9 (d = 24), 9.3e-9, 3.1e-11 (d = 512), 6.6e-10, 6.0e-9 (d = 8192)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import kid_ref64 as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
GUARD = 64


# ---- contrad_kid_sums on a given S ----
SUM_SHAPES = [(1, 1, -1), (1, 1, 0), (3, 7, 0), (7, 3, 0), (7, 3, 5), (65, 300, -1), (300, 300, 0), (257, 1025, 5),
              (1000, 1000, 0), (4, 70000, -1), (4, 70000, 123)]
_SUM_REF = {}


def _sum_inputs(shape):
    """{name: (S, fsum, bound)} for a shape, made once."""
    if shape not in _SUM_REF:
        M, n, self0 = shape
        r = np.random.RandomState(0)
        data = {'randn': np.clip(r.randn(M, n), -1, 1).astype(np.float32), 'equal': np.full((M, n), 0.25, np.float32)}
        _SUM_REF[shape] = {name: (S, K.block_sum(S, self0), K.block_bound(S, self0)) for name, S in data.items()}
    return _SUM_REF[shape]


def _device_S(S, pad, off):
    """S on the device with ``pad`` columns of NaN behind every row (a padding column that is read shows) and its base
    ``off`` floats past an allocation: off = 1 is not 16-byte aligned.  Returns (the allocation, the [M][n + pad] view)."""
    M, n = S.shape
    ld = n + pad
    flat = torch.full((off + M * ld + 8,), float('nan'), device='cuda')
    view = flat[off:off + M * ld].view(M, ld)
    view[:, :n] = torch.from_numpy(S).cuda()
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return flat, view


def _raw_sums(view, M, n, self0, gamma=1.0, coef0=1.0, accumulate=False, out=None, row0=0):
    """contrad_kid_sums on rows [row0, row0 + M) of ``view`` with guard bands around ``out`` and around a workspace of
    exactly the size the query names.  Returns (the float64 result, the guarded out buffer)."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    if out is None:
        out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    nbytes = lib().raw('contrad_kid_sums_workspace_bytes')(M, n)
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    rows = view[row0:row0 + M]
    rc = lib().raw('contrad_kid_sums')(ops._p(rows), ctypes.c_longlong(view.stride(0)), M, n, ctypes.c_longlong(self0), gamma,
                                       coef0, 1 if accumulate else 0, ops._p(out[GUARD:]), ops._p(ws[GUARD:]),
                                       ctypes.c_longlong(nbytes), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf in (out, ws):
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all()), 'guard band overwritten'
    return float(out[GUARD]), out


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'base+4B'])
@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', SUM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sums_kernel_on_a_given_S(shape, pad, off):
    M, n, self0 = shape
    for name, (S, ref, bound) in _sum_inputs(shape).items():
        tag = 'kid sums %s %s ld+%d base+%d' % ('x'.join(map(str, shape)), name, pad, off)
        _, view = _device_S(S, pad, off)
        got, _ = _raw_sums(view, M, n, self0)
        print('%s: device %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (tag, got, ref, abs(got - ref), bound))
        assert abs(got - ref) <= bound, tag
        if shape == (1, 1, 0):
            assert got == 0.0                                           # the only element is the one left out
        again, _ = _raw_sums(view, M, n, self0)
        assert _bits(got) == _bits(again), tag + ': two calls differ'
        # the excluded positions are never seen, whatever they hold; a NaN anywhere else is
        inside = [(i, j) for i, j in ((0, 0), (M - 1, n - 1), (M // 2, n // 2)) if self0 < 0 or j != self0 + i]
        for fill in (1e30, float('nan')):
            if self0 >= 0 and any(self0 + i < n for i in range(M)):
                X = S.copy()
                for i in range(M):
                    if self0 + i < n:
                        X[i, self0 + i] = fill
                _, xview = _device_S(X, pad, off)
                same, _ = _raw_sums(xview, M, n, self0)
                assert _bits(same) == _bits(got) and math.isfinite(same), tag + ': the excluded column was read'
        if inside:
            X = S.copy()
            X[inside[-1]] = np.nan
            _, xview = _device_S(X, pad, off)
            assert math.isnan(_raw_sums(xview, M, n, self0)[0]), tag + ': a NaN inside the block was lost'
            assert _bits(_raw_sums(xview, M, n, self0)[0]) == _bits(_raw_sums(xview, M, n, self0)[0])
        if M >= 2:                                                      # two row chunks, the second accumulates
            m1 = (M + 1) // 2 if M < 200 else 129                       # (129: one row past eight 16-row tiles)
            b1, b2 = K.block_bound(S[:m1], self0), K.block_bound(S[m1:], self0 + m1 if self0 >= 0 else -1)
            first, out = _raw_sums(view, m1, n, self0)
            assert abs(first - K.block_sum(S[:m1], self0)) <= b1, tag + ': first chunk'
            both, _ = _raw_sums(view, M - m1, n, self0 + m1 if self0 >= 0 else -1, accumulate=True, out=out, row0=m1)
            print('%s: chunked %.17g  |chunked - one call| %.3g  bounds %.3g + %.3g' % (tag, both, abs(both - got), b1, b2))
            assert abs(both - got) <= b1 + b2 and abs(both - ref) <= b1 + b2, tag + ': chunked'
            out2 = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
            _raw_sums(view, m1, n, self0, out=out2)
            again, _ = _raw_sums(view, M - m1, n, self0 + m1 if self0 >= 0 else -1, accumulate=True, out=out2, row0=m1)
            assert _bits(both) == _bits(again), tag + ': two chunked runs differ'


def test_kernel_parameters_and_accumulate():
    S, ref, bound = _sum_inputs((65, 300, -1))['randn']
    _, view = _device_S(S, 0, 0)
    for gamma, coef0 in ((0.5, 2.0), (-1.0, 0.0), (1.0 / 300, 1.0)):
        got, _ = _raw_sums(view, 65, 300, 7, gamma, coef0)
        assert abs(got - K.block_sum(S, 7, gamma, coef0)) <= K.block_bound(S, 7, gamma, coef0), (gamma, coef0)
    out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    out[GUARD] = 1e6                                                    # accumulate adds to what is there, and only then
    got, _ = _raw_sums(view, 65, 300, -1, accumulate=True, out=out)
    assert abs(got - (1e6 + ref)) <= bound + 2.0 ** -53 * 2e6
    got, _ = _raw_sums(view, 65, 300, -1, accumulate=False, out=out)
    assert abs(got - ref) <= bound
    X = S.copy()
    X[3, 5] = np.inf                                                    # an inf inside the block propagates
    assert _raw_sums(_device_S(X, 0, 0)[1], 65, 300, -1)[0] == np.inf


def test_wrapper_equals_the_entry_point_and_checks_its_arguments():
    from contrad_amd import ops
    S, ref, bound = _sum_inputs((65, 300, -1))['randn']
    S_dev = torch.from_numpy(S).cuda()
    wide = torch.full((65, 304), float('nan'), device='cuda')
    wide[:, :300] = S_dev
    raw, _ = _raw_sums(S_dev, 65, 300, -1)
    for X in (S_dev, wide):                                             # a row view of a wider matrix: only n columns are read
        out = ops.kid_sums(X, 300)
        assert out.dtype == torch.float64 and tuple(out.shape) == (1,) and _bits(float(out)) == _bits(raw)
        got = float(ops.kid_sums(X, 300, self0=10, gamma=0.5, coef0=2.0))
        assert abs(got - K.block_sum(S, 10, 0.5, 2.0)) <= K.block_bound(S, 10, 0.5, 2.0)
    table = torch.zeros(2, 3, dtype=torch.float64, device='cuda')
    assert ops.kid_sums(S_dev[:33], 300, self0=0, out=table[1, 1:2]).data_ptr() == table[1, 1:2].data_ptr()
    ops.kid_sums(S_dev[33:], 300, self0=33, out=table[1, 1:2], accumulate=True)
    assert abs(float(table[1, 1]) - K.block_sum(S, 0)) <= K.block_bound(S, 0) and float(table.abs().sum()) == abs(float(table[1, 1]))
    for bad in (dict(n=301), dict(n=0), dict(gamma=float('nan')), dict(coef0=float('inf')), dict(accumulate=True),
                dict(out=torch.zeros(1, device='cuda')), dict(out=torch.zeros(2, dtype=torch.float64, device='cuda')),
                dict(out=torch.zeros(1, dtype=torch.float64))):
        a = dict(n=300); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.kid_sums(S_dev, **a)
    with pytest.raises(RuntimeError):
        ops.kid_sums(S_dev.double(), 300)


def test_entry_point_returns_einval_on_device_pointers():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    f, query = lib().raw('contrad_kid_sums'), lib().raw('contrad_kid_sums_workspace_bytes')
    S = torch.zeros(2, 8, device='cuda')
    out = torch.full((1,), -7.0, dtype=torch.float64, device='cuda')
    need = query(2, 8)
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device='cuda')
    for a in (dict(S=None), dict(out=None), dict(M=0), dict(n=0), dict(ldS=7), dict(gamma=float('nan')), dict(coef0=float('inf')),
              dict(ws=None), dict(ws_bytes=need - 1)):
        b = dict(S=S, ldS=8, M=2, n=8, gamma=1.0, coef0=1.0, out=out, ws=ws, ws_bytes=need); b.update(a)
        assert f(ops._p(b['S']), ctypes.c_longlong(b['ldS']), b['M'], b['n'], ctypes.c_longlong(0), b['gamma'], b['coef0'], 0,
                 ops._p(b['out']), ops._p(b['ws']), ctypes.c_longlong(b['ws_bytes']), ops._stream()) == -22, a
    torch.cuda.synchronize()
    assert float(out) == -7.0 and bool((ws == -7.0).all())


# ---- kid on the device's own similarities ----
OWN_S_CASES = [(24, 300, 257, 100, 8), (512, 1000, 900, 1000, 3)]
FEATURE_CASES = OWN_S_CASES + [(8192, 300, 257, 257, 2)]
SHIFT = 1.5
_SETS = {}


def _sets(case, seed, shift=SHIFT):
    key = (case, seed, shift)
    if key not in _SETS:
        d, n_r, n_f, _, _ = case
        real, fake = K.shifted_sets(seed, d, n_r, n_f, shift)
        _SETS[key] = (real, fake, torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda())
    return _SETS[key]


def _device_blocks(real_rows, fake_rows, idx_r, idx_f):
    """The three fp32 similarity blocks the device forms for one subset of normalised device rows, read back."""
    from contrad_amd import features, kid
    dev = fake_rows.device
    R_t, F_t, bank_R, bank_F = kid.gather_subset(real_rows, None, fake_rows, torch.from_numpy(idx_r).to(dev), torch.from_numpy(idx_f).to(dev))
    m = len(idx_r)
    read = lambda q, bank: np.concatenate([S[:, :m].cpu().numpy() for _, S in features.similarity_chunks(q, bank)])
    return read(R_t, bank_R), read(F_t, bank_F), read(F_t, bank_R)


def _check_sums_on_own_S(got, real_rows, fake_rows, tag):
    """Every sum of ``got`` (a dict of ``kid``) within ``bound`` of the yardstick's fsum on the device's own floats; kid and
    kid_std the host formula on the returned table, exactly.  Returns the largest |device - fsum| / bound."""
    from contrad_amd import kid
    m, T = got['subset_size'], got['n_subsets']
    idx_r, idx_f = kid.subset_indices(got['n_real'], got['n_fake'], m, T, got['seed'])
    worst = 0.0
    for t in range(T):
        for c, (S, self0) in enumerate(zip(_device_blocks(real_rows, fake_rows, idx_r[t], idx_f[t]), (0, 0, -1))):
            assert S.shape == (m, m) and S.dtype == np.float32
            ref, bound = K.block_sum(S, self0, got['gamma'], got['coef0']), K.block_bound(S, self0, got['gamma'], got['coef0'])
            err = abs(got['sums'][t][c] - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (tag, t, 'ABC'[c], got['sums'][t][c], ref, bound)
    assert (got['kid'], got['kid_std']) == K.kid_of_sums(got['sums'], m), tag
    return worst


@pytest.mark.parametrize('case', OWN_S_CASES, ids=lambda c: 'd%d-%dx%d-m%d-t%d' % c)
def test_kid_sums_on_the_devices_own_similarities(case):
    from contrad_amd import features, kid
    d, n_r, n_f, size, T = case
    _, _, Rd, Fd = _sets(case, 0)
    got = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3)
    m = min(size, n_r, n_f)
    assert (got['n_subsets'], got['subset_size'], got['n_real'], got['n_fake'], got['gamma'], got['coef0'], got['degree'], got['seed']) == \
        (T, m, n_r, n_f, 1.0, 1.0, 3, 3)
    Rn, Fn = features.normalize_rows(Rd), features.normalize_rows(Fd)
    tag = 'kid own S d%d %dx%d m%d t%d' % case
    worst = _check_sums_on_own_S(got, Rn, Fn, tag)
    print('%s: kid %.6f +- %.6f; largest |device sum - fsum| / bound %.3g' % (tag, got['kid'], got['kid_std'], worst))
    assert kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3) == got                       # two calls: the same dict
    assert kid.kid(Rn, Fn, n_subsets=T, subset_size=size, seed=3, normalize=False) == got
    banked = kid.kid(None, Fn, n_subsets=T, subset_size=size, seed=3, normalize=False, real_bank=(features.bank_of(Rn), n_r))
    assert banked == got                                                # the hook's form of the real set: the same floats
    other = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=4)
    assert other['sums'] != got['sums']                                 # another seed: other subsets
    one = kid.kid(Rd, Fd, n_subsets=1, subset_size=size, seed=3)
    assert one['kid_std'] == 0.0 and one['sums'][0] == got['sums'][0]   # the first subset of the same draw


# ---- kid against float64 features ----
_REF64 = {}


def _ref64(case, seed):
    if (case, seed) not in _REF64:
        d, n_r, n_f, size, T = case
        real, fake, _, _ = _sets(case, seed)
        _REF64[case, seed] = K.kid_ref64(real, fake, T, size, seed)
    return _REF64[case, seed]


def _feature_bound(d):
    e = (2 * d + 8) * EPS
    return 12 * (2 + e) ** 2 * e


@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('case', FEATURE_CASES, ids=lambda c: 'd%d-%dx%d-m%d-t%d' % c)
def test_kid_on_features_against_float64(case, seed):
    from contrad_amd import kid
    d, n_r, n_f, size, T = case
    ref, bound = _ref64(case, seed), _feature_bound(d)
    _, _, Rd, Fd = _sets(case, seed)
    got = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=seed)
    _, _, R0, F0 = _sets(case, seed, 0.0)
    same = kid.kid(R0, F0, n_subsets=T, subset_size=size, seed=seed)
    print('kid features d%d %dx%d m%d t%d seed %d: device %.9f  float64 %.9f  |diff| %.3g  bound %.3g  (std device %.6f float64 %.6f; '
          'unshifted sets: %.6f)' % (d, n_r, n_f, size, T, seed, got['kid'], ref['kid'], abs(got['kid'] - ref['kid']), bound,
                                     got['kid_std'], ref['kid_std'], same['kid']))
    assert ref['kid'] >= 10 * bound                                     # the check is not empty
    assert got['subset_size'] == ref['subset_size'] and abs(got['kid'] - ref['kid']) <= bound
    assert abs(got['kid_std'] - ref['kid_std']) <= bound                # (std is a seminorm: |std(x + e) - std(x)| <= std(e) <= max |e_t|)
    assert abs(same['kid']) < 0.1 and got['kid'] > same['kid'] + 0.3


def test_row_chunks_of_a_subset_stay_within_the_float64_bound(monkeypatch):
    from contrad_amd import features, kid
    case = FEATURE_CASES[0]
    d, n_r, n_f, size, T = case
    ref = _ref64(case, 1)
    _, _, Rd, Fd = _sets(case, 1)
    monkeypatch.setattr(features, 'MAX_CHUNK_ROWS', 32)                 # 100 rows of a subset: 32 + 32 + 32 + 4
    assert features.chunk_rows_of(100) == 32                            # the patch reaches the rule (a subset's bank: 100 columns)
    got = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=1)
    assert abs(got['kid'] - ref['kid']) <= _feature_bound(d)
    _check_sums_on_own_S(got, features.normalize_rows(Rd), features.normalize_rows(Fd), 'kid in chunks of 32 rows')


def test_host_refusals_on_device_tensors():
    from contrad_amd import kid
    _, _, Rd, Fd = _sets(FEATURE_CASES[0], 0)
    for bad in (dict(n_subsets=0), dict(subset_size=1), dict(gamma=float('inf'))):
        with pytest.raises(ValueError):
            kid.kid(Rd, Fd, **bad)
    with pytest.raises(ValueError):
        kid.kid(Rd[:1], Fd)                                             # m < 2
    with pytest.raises(ValueError):
        kid.kid(Rd, Fd[:0])
    with pytest.raises(RuntimeError):
        kid.kid(Rd, Fd[:, :8].contiguous())                             # widths differ
    assert kid.kid(Rd[:2], Fd[:2], n_subsets=2)['subset_size'] == 2


# ---- through a discriminator ----
def test_kid_of_through_sndcgan_equals_the_yardstick_on_the_device_S():
    from contrad_amd import kid, lineval
    from contrad_amd.features import extract_features
    import test_prdc_gpu as TP
    data = lineval.synthetic_set(3, 4, 256, 192)
    _, D = TP._encoder()
    D = D.cuda().eval()
    for p in D.parameters():
        p.requires_grad_(False)
    real_u8, fake_u8 = torch.from_numpy(data['x_train']).cuda(), torch.from_numpy(data['x_test']).cuda()
    got = kid.kid_of(D, real_u8, fake_u8, n_subsets=10, seed=5, batch=100)
    assert (got['n_real'], got['n_fake'], got['subset_size'], got['n_subsets'], got['seed']) == (256, 192, 192, 10, 5)
    fr, ff = extract_features(D, real_u8, 100), extract_features(D, fake_u8, 100)
    _check_sums_on_own_S(got, fr, ff, 'kid_of sndcgan')
    # the host formula on the YARDSTICK's sums of the device's own S: the device sums are within their bounds, so
    # MMD2_t is within (b_A + b_B) / (m (m - 1)) + 2 b_C / m^2 and kid within the mean of that (plus the formula's own
    # roundings on numbers below 16: 2^-48 covers them)
    m, T = 192, 10
    idx_r, idx_f = kid.subset_indices(256, 192, m, T, 5)
    yard, slack = [], []
    for t in range(T):
        blocks = _device_blocks(fr, ff, idx_r[t], idx_f[t])
        yard.append([K.block_sum(S, s0) for S, s0 in zip(blocks, (0, 0, -1))])
        b = [K.block_bound(S, s0) for S, s0 in zip(blocks, (0, 0, -1))]
        slack.append((b[0] + b[1]) / (m * (m - 1)) + 2 * b[2] / (m * m))
    ref_kid, ref_std = K.kid_of_sums(yard, m)
    tol = float(np.mean(slack)) + 2.0 ** -48
    print('kid_of sndcgan: device %.12f +- %.12f  yardstick on the device S %.12f +- %.12f  |diff| %.3g  tolerance %.3g'
          % (got['kid'], got['kid_std'], ref_kid, ref_std, abs(got['kid'] - ref_kid), tol))
    assert abs(got['kid'] - ref_kid) <= tol and abs(got['kid_std'] - ref_std) <= max(slack) + 2.0 ** -48
    with pytest.raises(ValueError):
        kid.kid_of(D, real_u8, fake_u8[:, :16, :16].contiguous())
    with pytest.raises(ValueError):
        kid.kid_of(D, real_u8[:0], fake_u8)
    with pytest.raises(ValueError):
        kid.kid_of(D, real_u8, fake_u8[:1])
    with pytest.raises(RuntimeError):
        kid.kid_of(D.train(), real_u8, fake_u8)


# ---- scripts (the encoder, the real set and the runs without --prdc_kid are those of tests/test_prdc_gpu.py) ----
_RUNS = {}


def _run(factory, graph):
    """train_gan for 4 steps with ``--prdc_data ... --prdc_kid --prdc_best kid``, evaluations at 2 and 4 (kept as *_2.pt / *_4.pt)."""
    import test_prdc_gpu as TP
    if graph not in _RUNS:
        from contrad_amd.train_gan import main
        logdir = str(factory.mktemp('kid_run'))
        gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
              '--save_every', '2', '--seed', str(TP.SEED), '--logdir', logdir] + (['--graph'] if graph else []) +
             TP._hook_flags(factory, None) + ['--prdc_kid', '--prdc_best', 'kid'])
        _RUNS[graph] = logdir
    return _RUNS[graph]


def _kid_rows(logdir, seed):
    with open(os.path.join(logdir, 'kid_%d.csv' % seed)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,kid,kid_std'
    return [(int(v[0]), float(v[1]), float(v[2])) for v in (ln.split(',') for ln in lines[1:])]


def _cli_row(path):
    with open(path) as f:
        out = json.load(f)
    return out, (float('%.6f' % out['kid']), float('%.6f' % out['kid_std']))


def test_command_line_writes_the_json(tmp_path_factory, tmp_path):
    import shutil
    import test_kid
    import test_prdc_gpu as TP
    d = TP._files(tmp_path_factory)
    gen = str(tmp_path / 'gen.pt')
    shutil.copy(os.path.join(TP._run(tmp_path_factory, False, False), 'gen.pt'), gen)
    os.makedirs(str(tmp_path / 'samples'))
    TP._sampled_reals([gen], 'sndcgan', 192, str(tmp_path / 'x.npz'), seed=777)
    with np.load(str(tmp_path / 'x.npz')) as z:
        np.savez(str(tmp_path / 'samples' / 'samples.npz'), images=z['x_train'])
    common = [str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz')]
    path = test_kid.main(common + ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--seed', '3', '--n_fake', '100',
                                   '--n_subsets', '7', '--subset_size', '64'])
    assert path == str(tmp_path / 'samples' / 'kid_3.json')
    out, _ = _cli_row(path)
    assert (out['n_real'], out['n_fake'], out['n_subsets'], out['subset_size'], out['gamma'], out['coef0'], out['degree'], out['seed']) == \
        (256, 100, 7, 64, 1.0, 1.0, 3, 3)
    assert (out['kid'], out['kid_std']) == K.kid_of_sums(out['sums'], 64) and 'gamma = 1' in out['kernel']
    path = test_kid.main(common + ['--gen', gen, '--seed', '3', '--n_fake', '64', '--n_real', '200'])
    assert path == str(tmp_path / 'kid_3.json')
    out, _ = _cli_row(path)
    assert (out['n_real'], out['n_fake'], out['n_subsets'], out['subset_size']) == (200, 64, 100, 64)
    np.savez(str(tmp_path / 'small.npz'), images=np.zeros((8, 16, 16, 3), np.uint8))
    for bad in (['--fake', str(tmp_path / 'small.npz')],                                   # 16 x 16 fakes, 32 x 32 reals
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_fake', '1'],       # m < 2
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_real', '0'],       # an empty set
                ['--gen', gen, '--n_subsets', '0'], ['--gen', gen, '--subset_size', '1']):
        with pytest.raises(ValueError):
            test_kid.main(common + bad)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_hook_leaves_checkpoints_and_the_prdc_csv_alone(graph, tmp_path_factory):
    import test_kid
    import test_prdc_gpu as TP
    plain, prdc_only, hooked = TP._run(tmp_path_factory, graph, False), TP._run(tmp_path_factory, graph, ''), _run(tmp_path_factory, graph)
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    csv = 'prdc_%d.csv' % TP.EVAL_SEED
    with open(os.path.join(prdc_only, csv), 'rb') as a, open(os.path.join(hooked, csv), 'rb') as b:
        assert a.read() == b.read()                                     # byte for byte the rows of --prdc_data alone
    rows = _kid_rows(hooked, TP.EVAL_SEED)
    print('kid rows (%s): %s' % ('graph' if graph else 'eager', rows))
    assert [r[0] for r in rows] == [2, 4] and all(math.isfinite(r[1]) and r[2] >= 0.0 for r in rows)
    for other in (plain, prdc_only):                                    # without the flag nothing new is written
        assert not [f for f in os.listdir(other) if f.startswith('kid_') or '_best' in f]
    with open(os.path.join(hooked, 'log.txt')) as f:
        log = f.read()
    assert '[kid %.6f +- %.6f]' % rows[0][1:] in log and '[kid %.6f +- %.6f]' % rows[1][1:] in log
    # the logged figures are the checkpoint's: the command line on the saved generator, with the eval seed, gives the last row
    d = TP._files(tmp_path_factory)
    path = test_kid.main([str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz'), '--gen', os.path.join(hooked, 'gen.pt'),
                          '--seed', str(TP.EVAL_SEED), '--n_fake', str(TP.N_FAKE)])
    assert _cli_row(path)[1] == rows[-1][1:]


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_best_checkpoints_are_those_of_the_smaller_kid(graph, tmp_path_factory):
    import test_prdc_gpu as TP
    hooked = _run(tmp_path_factory, graph)
    rows = _kid_rows(hooked, TP.EVAL_SEED)
    best_step = 4 if rows[1][1] < rows[0][1] else 2                     # the minimum; the first evaluation wins on a tie
    print('kid at step 2: %.6f, at step 4: %.6f -> best step %d' % (rows[0][1], rows[1][1], best_step))
    for name in ('gen', 'dis'):
        TP._same_files(os.path.join(hooked, '%s_best.pt' % name), os.path.join(hooked, '%s_%d.pt' % (name, best_step)))
    assert not os.path.exists(os.path.join(hooked, 'gen_ema_best.pt'))


def test_stylegan2_loop_with_the_hook_evaluates_gen_ema(tmp_path, tmp_path_factory):
    import test_kid
    import test_prdc_gpu as TP
    from contrad_amd import config
    from contrad_amd.train_stylegan2 import main
    d = TP._files(tmp_path_factory)
    args = [os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
            '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
            '--seed', str(TP.SEED)]
    plain, logdir, real = str(tmp_path / 'plain'), str(tmp_path / 'run'), str(tmp_path / 'real.npz')
    main(args + ['--logdir', plain])
    TP._sampled_reals([os.path.join(plain, 'gen_ema.pt')], 'stylegan2', 128, real)
    main(args + ['--logdir', logdir, '--prdc_data', real, '--prdc_encoder', str(d / 'enc.pt'), '--prdc_encoder_arch', 'sndcgan',
                 '--prdc_n', '64', '--prdc_kid', '--prdc_best', 'kid'])
    rows = _kid_rows(logdir, TP.EVAL_SEED)
    assert [r[0] for r in rows] == [2]
    for name in ('gen', 'dis', 'gen_ema'):                              # the first evaluation is the best so far
        TP._same_files(os.path.join(logdir, '%s_best.pt' % name), os.path.join(logdir, '%s.pt' % name))
        TP._same_files(os.path.join(logdir, '%s.pt' % name), os.path.join(plain, '%s.pt' % name))
    cli = [str(d / 'enc.pt'), 'sndcgan', '--real', real, '--gen_arch', 'stylegan2', '--seed', str(TP.EVAL_SEED), '--n_fake', '64']
    assert _cli_row(test_kid.main(cli + ['--gen', os.path.join(logdir, 'gen_ema.pt')]))[1] == rows[-1][1:]      # gen_ema is evaluated
    other = _cli_row(test_kid.main(cli + ['--gen', os.path.join(logdir, 'gen.pt')]))[1]
    print('stylegan2 hook row %s; the command line on gen.pt gives %s' % (rows[-1][1:], other))
    assert other != rows[-1][1:]                                        # ... and gen is not


def test_resumed_monitor_reads_the_smallest_kid_up_to_its_checkpoint(tmp_path_factory, tmp_path):
    """The monitor over the csv files of the --graph run (rows for steps 2 and 4), as a run resumed from step 4, from step 2
    and as a fresh run in the same directory; then one evaluation against each."""
    import shutil
    import test_prdc_gpu as TP
    from contrad_amd import features, prdc
    from contrad_amd.models.gan import get_architecture
    d, hooked = TP._files(tmp_path_factory), _run(tmp_path_factory, True)
    rows = _kid_rows(hooked, TP.EVAL_SEED)
    dev = torch.device('cuda', 0)
    G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, 'gen_4.pt'), dev)

    def monitor(resumed_step, sub):
        logdir = tmp_path / sub
        os.makedirs(str(logdir))
        for name in ('prdc_%d.csv' % TP.EVAL_SEED, 'kid_%d.csv' % TP.EVAL_SEED):
            shutil.copy(os.path.join(hooked, name), str(logdir / name))
        return prdc.PRDCMonitor(str(logdir), 'sndcgan', (32, 32, 3), dev, TP.SEED, str(d / 'real.npz'), str(d / 'enc.pt'),
                                n_fake=TP.N_FAKE, best='kid', resumed_step=resumed_step, kid=True), str(logdir)
    m4, dir4 = monitor(4, 'from4')
    m2, _ = monitor(2, 'from2')
    m0, _ = monitor(0, 'fresh')
    assert (m4.best, m2.best, m0.best) == (min(rows[0][1], rows[1][1]), rows[0][1], None)
    out = m4.update(6, G)                                               # step 4's generator again: the same figures, no improvement
    assert (float('%.6f' % out['kid']), float('%.6f' % out['kid_std'])) == rows[1][1:] and not out['improved']
    assert [r[0] for r in _kid_rows(dir4, TP.EVAL_SEED)] == [2, 4, 6]     # a resumed run appends to its file
    assert [r[0] for r in TP._csv_rows(dir4)] == [2, 4, 6]
    assert m2.update(4, G)['improved'] == (rows[1][1] < rows[0][1]) and m2.best == min(rows[0][1], rows[1][1])
    assert m0.update(2, G)['improved'] and m0.best == rows[1][1]
    with pytest.raises(ValueError, match='needs --prdc_kid'):
        prdc.PRDCMonitor(str(tmp_path), 'sndcgan', (32, 32, 3), dev, TP.SEED, str(d / 'real.npz'), str(d / 'enc.pt'),
                         n_fake=TP.N_FAKE, best='kid')
