"""Precision / recall / density / coverage on the GPU against the yardstick (tests/prdc_ref64.py): the two kernels of
csrc/prdc.hip alone on a given S (exact), ``prdc`` on features against float64, ``prdc_of`` through a discriminator
(exact on the device's own S), the command line and the ``--prdc_data`` hook of the training scripts (which must not move
the trajectory by a bit) with its best checkpoints.

On features a device similarity differs from the float64 one by at most (2 d + 8) * 2^-24 (derived at the head of
tests/test_knn_gpu.py); a value and a threshold both carry it, so an indicator [s >= t] is DECIDED only if
|s - t| >= g = 2 (2 d + 8) 2^-24.  Every device count must lie between the count of decided hits and the count of
decided plus undecided hits; the interval widths are asserted too, so that the inputs cannot silently make the check
empty.

Observed on the MI355X (the distance of the device metrics from the float64 point values, largest over the six cases):
precision 0, recall 0, density 0, coverage 0 -- every count equals the float64 count; the intervals are 0 to 0.010 wide
for precision / recall / coverage and up to 0.039 for density (d = 8192)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import prdc_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
GUARD = 64


def _guarded(numel, dtype, fill, zero=False):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    if zero:
        buf[GUARD:GUARD + numel] = 0
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(pairs, fill=-7):
    for buf, _ in pairs:
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), 'guard band overwritten'


def _ip(t):
    from contrad_amd import ops
    return ctypes.cast(ops._p(t), ctypes.POINTER(ctypes.c_int))


def _padded(S, pad):
    """S on the device with ``pad`` columns of +inf behind every row: a padding column that is read shows."""
    full = np.full((S.shape[0], S.shape[1] + pad), np.inf, np.float32)
    full[:, :S.shape[1]] = S
    return torch.from_numpy(full).cuda()


# ---- prdc_kth on a given S ----
KTH_SHAPES = [(1, 2, 1, 0), (3, 7, 6, 0), (5, 300, 5, 0), (5, 300, 5, 295), (2, 1025, 1, -1), (2, 1025, 1025, -1),
              (4, 70000, 5, 123)]


def _raw_kth(S_dev, ldS, M, n, k, self0):
    from contrad_amd import ops
    from contrad_amd._lib import lib
    out = _guarded(M, torch.float32, -7.0)
    rc = lib().raw('contrad_prdc_kth')(ops._p(S_dev), ctypes.c_longlong(ldS), M, n, k, ctypes.c_longlong(self0), ops._p(out[1]),
                                       ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _guards_intact([out])
    return out[1].cpu().numpy()


def _kth_inputs(shape):
    M, n, k, self0 = shape
    r = np.random.RandomState(0)
    S = r.randn(M, n).astype(np.float32)
    out = {'randn': S, 'ties': (np.round(S * 8) / 8).astype(np.float32), 'equal': np.full((M, n), 0.25, np.float32)}
    zeros = np.zeros((M, n), np.float32)
    zeros[:, ::2] = -0.0
    for i in range(M):
        zeros[i, (7 * i + 1) % n] = np.nan
    out['zeros+nan'] = zeros
    for name, v in (('self=inf', np.inf), ('self=nan', np.nan)):       # exclusion is by index: the value there is never seen
        x = S.copy()
        for i in range(M):
            if 0 <= self0 + i < n:
                x[i, self0 + i] = v
        out[name] = x
    return out


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', KTH_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kth_kernel_on_a_given_S(shape, pad):
    M, n, k, self0 = shape
    for name, S in _kth_inputs(shape).items():
        S_dev = _padded(S, pad)
        got = _raw_kth(S_dev, n + pad, M, n, k, self0)
        tag = 'prdc kth %s %s ld+%d' % ('x'.join(map(str, shape)), name, pad)
        assert np.array_equal(got.view(np.uint32), R.kth_exact(S, k, self0).view(np.uint32)), tag    # bit for bit
        again = _raw_kth(S_dev, n + pad, M, n, k, self0)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), tag + ': two calls differ'
    if self0 >= 0:                                                   # with the excluded column +inf, k = 1 finds it unless excluded
        S = _kth_inputs(shape)['self=inf']
        assert np.isinf(_raw_kth(_padded(S, pad), n + pad, M, n, 1, -1)).all()
        assert np.isfinite(_raw_kth(_padded(S, pad), n + pad, M, n, 1, self0)).all()


# ---- the two selects (csrc/simrow.h under prdc.hip and knn.hip) on the same S ----
AGREE_SHAPES = [(3, 7, 6, 0), (5, 300, 5, 295), (2, 1025, 1, -1), (2, 1025, 1024, -1)]         # k <= 1024: knn_select's limit
NANS = np.array([0x7fc00000, 0xffc00001, 0x7fc00123], np.uint32).view(np.float32)              # the very float must come back


def _agree_inputs(shape):
    """Rows on which the k-th place is decided by the tie rule.  `zeros-*`: Z columns of alternating -0.0 / +0.0 with fewer
    than k columns above them and at least k down to their end, the own column (a -0.0 that must not count) right before the
    run, in its middle or right behind it in column order -- where the row leaves no room on that side (a row without an own
    column, an own column at either end), the run lies at the end, the middle or the start of the row.  `nans`: fewer than k
    columns hold a number, so the k-th place is a NaN."""
    M, n, k, self0 = shape
    r = np.random.RandomState(2)
    S = r.randn(M, n).astype(np.float32)
    out = {'randn': S, 'equal': np.full((M, n), 0.25, np.float32)}
    for where in ('before', 'inside', 'behind'):
        x = np.empty((M, n), np.float32)
        for i in range(M):
            c = self0 + i if 0 <= self0 and self0 + i < n else None
            cols = [j for j in range(n) if j != c]
            at = len(cols) // 2 if c is None else sum(j < c for j in cols)       # cols[at] is the first column behind the own one
            Z = min(max(len(cols) // 2, 2), 8)
            above = min(max(k - Z // 2 - 1, 0), len(cols) - Z)                  # above < k <= above + Z
            assert above < k <= above + Z
            start = {'before': at, 'inside': at - Z // 2, 'behind': at - Z}[where]
            if c is None:
                start = {'before': len(cols) - Z, 'inside': at - Z // 2, 'behind': 0}[where]
            start = min(max(start, 0), len(cols) - Z)
            run = cols[start:start + Z]
            rest = [cols[j] for j in r.permutation(len(cols)) if cols[j] not in run]
            x[i, rest[:above]] = r.uniform(0.5, 1.5, above)
            x[i, rest[above:]] = r.uniform(-1.5, -0.5, len(rest) - above)
            x[i, run] = np.where(np.arange(Z) % 2 == i % 2, -0.0, 0.0)           # the k-th place is a -0.0 or a +0.0 by the row
            if c is not None:
                x[i, c] = -0.0
        out['zeros-own-' + where] = x
    x = S.copy()
    for i in range(M):
        c = self0 + i if 0 <= self0 and self0 + i < n else None
        cols = np.array([j for j in range(n) if j != c])
        holes = r.permutation(cols)[max(k - 2, 0):]                             # k - 2 numbers (none for k = 1): k reaches into the NaNs
        x[i, holes] = NANS[np.arange(len(holes)) % 3]
        if c is not None:
            x[i, c] = NANS[0]
    out['nans'] = x
    return out


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', AGREE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_prdc_kth_equals_the_kth_value_of_knn_select_bit_for_bit(shape, pad):
    """prdc_kth and knn_select share the key order and the radix select of csrc/simrow.h and each add a tie rule of their own
    (prdc.hip's second ordered pass, knn.hip's compaction and sort): on the same S they must name the same float."""
    from contrad_amd import ops
    M, n, k, self0 = shape
    labels = torch.zeros(n, dtype=torch.int64, device='cuda')
    for name, S in _agree_inputs(shape).items():
        S_dev = _padded(S, pad)
        kth = ops.prdc_kth(S_dev, n, k, self0).cpu().numpy()
        val = ops.knn_select(S_dev, n, labels, 1, k, 1.0, self0)[1][:, k - 1].cpu().numpy()
        tag = 'kth against knn_select %s %s ld+%d' % ('x'.join(map(str, shape)), name, pad)
        assert np.array_equal(kth.view(np.int32), val.view(np.int32)), (tag, kth, val)
        assert np.array_equal(kth.view(np.int32), R.kth_exact(S, k, self0).view(np.int32)), tag      # ... and it is the right one


# ---- prdc_count on a given S ----
COUNT_SHAPES = [(1, 1), (3, 7), (65, 300), (257, 1025), (4, 70000)]


def _raw_count(S_dev, ldS, M, n, thr_row, thr_col, row0=0, rows=None, cols=None):
    """contrad_prdc_count on rows [row0, row0 + rows) of S with guarded outputs; ``cols``: the guarded column arrays of an
    earlier call to add into (else zeroed ones).  Returns (row_hits, col_c, col_r, cols)."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    rows = M if rows is None else rows
    rh = _guarded(rows, torch.int32, -7)
    cols = cols or (_guarded(n, torch.int32, -7, zero=True), _guarded(n, torch.int32, -7, zero=True))
    tr = thr_row[row0:row0 + rows] if thr_row is not None else None
    rc = lib().raw('contrad_prdc_count')(ops._p(S_dev[row0:]), ctypes.c_longlong(ldS), rows, n, ops._p(tr), ops._p(thr_col),
                                         _ip(rh[1] if thr_col is not None else None), _ip(cols[0][1] if thr_col is not None else None),
                                         _ip(cols[1][1] if thr_row is not None else None), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _guards_intact([rh, cols[0], cols[1]])
    return rh[1].cpu().numpy(), cols[0][1].cpu().numpy(), cols[1][1].cpu().numpy(), cols


def _count_inputs(shape):
    M, n = shape
    r = np.random.RandomState(1)
    S = (np.round(r.randn(M, n) * 8) / 8).astype(np.float32)          # eighths: equal values abound
    if n >= 7:
        S[0, 3] = np.nan
        S[M - 1, n - 2] = -0.0
    from_col = S[(3 * np.arange(n)) % M, np.arange(n)].copy()         # thresholds taken from the data: equality occurs
    from_row = S[np.arange(M), (5 * np.arange(M)) % n].copy()
    some_nan_c, some_nan_r = from_col.copy(), from_row.copy()
    some_nan_c[::3] = np.nan
    some_nan_r[::2] = np.nan
    f = lambda v, m: np.full(m, v, np.float32)
    return S, {'data': (from_row, from_col), '-inf': (f(-np.inf, M), f(-np.inf, n)), '+inf': (f(np.inf, M), f(np.inf, n)),
               'some-nan': (some_nan_r, some_nan_c), 'row-only': (from_row, None), 'col-only': (None, from_col)}


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', COUNT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_count_kernel_on_a_given_S(shape, pad):
    M, n = shape
    S, variants = _count_inputs(shape)
    S_dev = _padded(S, pad)
    for name, (thr_row, thr_col) in variants.items():
        tag = 'prdc count %dx%d %s ld+%d' % (M, n, name, pad)
        tr = torch.from_numpy(thr_row).cuda() if thr_row is not None else None
        tc = torch.from_numpy(thr_col).cuda() if thr_col is not None else None
        r_rh, r_cc, r_cr = R.count_exact(S, thr_row, thr_col)
        rh, cc, cr, _ = _raw_count(S_dev, n + pad, M, n, tr, tc)
        if thr_col is not None:
            assert np.array_equal(rh, r_rh) and np.array_equal(cc, r_cc), tag
            assert int(rh.sum()) == int(cc.sum()), tag
        else:
            assert (rh == -7).all() and (cc == 0).all(), tag          # a NULL threshold array skips its outputs
        if thr_row is not None:
            assert np.array_equal(cr, r_cr), tag
        else:
            assert (cr == 0).all(), tag
        if name == '-inf':                                            # everything but the NaN hits
            assert int(cc.sum()) == int(np.isfinite(S).sum()) + int(np.isinf(S).sum())
        if name == '+inf':
            assert not rh.any() and not cc.any() and not cr.any()
        again = _raw_count(S_dev, n + pad, M, n, tr, tc)
        for a, b in zip((rh, cc, cr), again[:3]):
            assert np.array_equal(a, b), tag + ': two calls differ'
        if M >= 2:                                                    # two row chunks ADD into the column arrays
            m1 = (M + 1) // 2 if M < 200 else 129                     # (129: one row past a 128-row tile)
            rh1, _, _, cols = _raw_count(S_dev, n + pad, M, n, tr, tc, 0, m1)
            rh2, cc2, cr2, _ = _raw_count(S_dev, n + pad, M, n, tr, tc, m1, M - m1, cols)
            assert np.array_equal(cc2, cc) and np.array_equal(cr2, cr), tag + ': chunked'
            if thr_col is not None:
                assert np.array_equal(np.concatenate([rh1, rh2]), rh), tag + ': chunked'


def test_wrappers_equal_the_entry_points_and_check_their_arguments():
    from contrad_amd import ops
    S, variants = _count_inputs((65, 300))
    thr_row, thr_col = variants['data']
    S_dev, tr, tc = torch.from_numpy(S).cuda(), torch.from_numpy(thr_row).cuda(), torch.from_numpy(thr_col).cuda()
    wide = torch.full((65, 304), float('inf'), device='cuda')
    wide[:, :300] = S_dev
    for X in (S_dev, wide):                                           # a row view of a wider matrix: only n columns are read
        thr = ops.prdc_kth(X, 300, 5, self0=10)
        assert np.array_equal(thr.cpu().numpy().view(np.uint32), R.kth_exact(S, 5, 10).view(np.uint32))
        cc, cr = torch.zeros(300, dtype=torch.int32, device='cuda'), torch.zeros(300, dtype=torch.int32, device='cuda')
        rh = ops.prdc_count(X, 300, thr_row=tr, thr_col=tc, col_hits_c=cc, col_hits_r=cr)
        r_rh, r_cc, r_cr = R.count_exact(S, thr_row, thr_col)
        assert np.array_equal(rh.cpu().numpy(), r_rh) and np.array_equal(cc.cpu().numpy(), r_cc) and np.array_equal(cr.cpu().numpy(), r_cr)
    out = torch.empty(65, device='cuda')
    assert ops.prdc_kth(S_dev, 300, 5, out=out) is out
    cc = torch.zeros(300, dtype=torch.int32, device='cuda')
    for bad in (dict(n=301), dict(n=0), dict(k=0), dict(k=300, self0=0), dict(k=301)):
        a = dict(n=300, k=5, self0=-1); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.prdc_kth(S_dev, a['n'], a['k'], self0=a['self0'])
    with pytest.raises(RuntimeError):
        ops.prdc_kth(S_dev, 300, 5, out=torch.empty(64, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.prdc_count(S_dev, 300)                                    # no threshold at all
    with pytest.raises(RuntimeError):
        ops.prdc_count(S_dev, 300, thr_col=tc)                        # nowhere to add
    with pytest.raises(RuntimeError):
        ops.prdc_count(S_dev, 300, thr_col=tc[:299], col_hits_c=cc)
    with pytest.raises(RuntimeError):
        ops.prdc_count(S_dev, 300, thr_col=tc, col_hits_c=cc.float())
    with pytest.raises(RuntimeError):
        ops.prdc_count(S_dev, 300, thr_row=tr, col_hits_r=cc[:299])


def test_entry_points_return_einval_on_device_pointers():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    S = torch.zeros(2, 8, device='cuda')
    thr = torch.full((2,), -7.0, device='cuda')
    tc, tr = torch.zeros(8, device='cuda'), torch.zeros(2, device='cuda')
    rh = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    cc, cr = torch.full((8,), -7, dtype=torch.int32, device='cuda'), torch.full((8,), -7, dtype=torch.int32, device='cuda')
    kth, count = lib().raw('contrad_prdc_kth'), lib().raw('contrad_prdc_count')
    for a in (dict(k=0), dict(k=8), dict(k=9, self0=-1), dict(ldS=7), dict(M=0), dict(n=0)):
        b = dict(ldS=8, M=2, n=8, k=3, self0=0); b.update(a)
        assert kth(ops._p(S), ctypes.c_longlong(b['ldS']), b['M'], b['n'], b['k'], ctypes.c_longlong(b['self0']), ops._p(thr),
                   ops._stream()) == -22, a
    assert kth(ops._p(None), ctypes.c_longlong(8), 2, 8, 3, ctypes.c_longlong(0), ops._p(thr), ops._stream()) == -22
    assert kth(ops._p(S), ctypes.c_longlong(8), 2, 8, 3, ctypes.c_longlong(0), ops._p(None), ops._stream()) == -22
    for a in (dict(S=None), dict(tr=None, tc=None), dict(rh=None), dict(cc=None), dict(cr=None), dict(ldS=7), dict(M=0), dict(n=0)):
        b = dict(S=S, ldS=8, M=2, n=8, tr=tr, tc=tc, rh=rh, cc=cc, cr=cr); b.update(a)
        assert count(ops._p(b['S']), ctypes.c_longlong(b['ldS']), b['M'], b['n'], ops._p(b['tr']), ops._p(b['tc']), _ip(b['rh']),
                     _ip(b['cc']), _ip(b['cr']), ops._stream()) == -22, a
    torch.cuda.synchronize()
    assert bool((thr == -7).all()) and bool((rh == -7).all()) and bool((cc == -7).all()) and bool((cr == -7).all())


# ---- features against float64 ----
FEATURE_CASES = [(24, 300, 257, 5), (8192, 300, 257, 5), (512, 1000, 900, 5)]
WIDTH_LIMIT = {'precision': 0.02, 'recall': 0.02, 'coverage': 0.02, 'density': 0.05}
COUNT_OF = {'precision': 'fakes_in_real_balls', 'recall': 'reals_in_fake_balls', 'density': 'hits', 'coverage': 'reals_with_a_fake'}
_REF = {}


def _feature_ref(case, seed):
    if (case, seed) not in _REF:
        d, n_r, n_f, k = case
        real, fake = R.manifold_sets(seed, d, n_r, n_f)
        _REF[case, seed] = (real, fake, R.prdc_ref64(real, fake, k, gap=2 * (2 * d + 8) * EPS))
    return _REF[case, seed]


@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('case', FEATURE_CASES, ids=lambda c: 'd%d-%dx%d-k%d' % c)
def test_prdc_on_features_against_float64(case, seed):
    from contrad_amd import prdc
    d, n_r, n_f, k = case
    real, fake, ref = _feature_ref(case, seed)
    got = prdc.prdc(torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda(), k)
    assert (got['n_real'], got['n_fake'], got['k']) == (n_r, n_f, k)
    for m in R.METRICS:
        c = COUNT_OF[m]
        print('prdc features d%d %dx%d k%d seed %d %-9s device %.6f  float64 %.6f  |diff| %.6f  count %d in [%d, %d]  width %.4f'
              % (d, n_r, n_f, k, seed, m, got[m], ref[m], abs(got[m] - ref[m]), got[c], ref['lo'][c], ref['hi'][c], ref['width'][m]))
    for m in R.METRICS:
        c = COUNT_OF[m]
        assert ref['width'][m] <= WIDTH_LIMIT[m], (m, ref['width'][m])          # the check is not empty
        assert ref['lo'][c] <= got[c] <= ref['hi'][c], (m, got[c], ref['lo'][c], ref['hi'][c])
    assert got['precision'] == got['fakes_in_real_balls'] / n_f and got['recall'] == got['reals_in_fake_balls'] / n_r
    assert got['density'] == got['hits'] / (k * n_f) and got['coverage'] == got['reals_with_a_fake'] / n_r


def test_a_set_against_itself_and_the_cached_real_state():
    from contrad_amd import prdc
    real, fake, _ = _feature_ref(FEATURE_CASES[0], 0)
    Rd, Fd = torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda()
    same = prdc.prdc(Rd, Rd, 5)
    assert same['precision'] == same['recall'] == same['coverage'] == 1.0         # exactly: every row finds itself
    state = prdc.real_state_of(Rd, 5)
    assert prdc.prdc(None, Fd, 5, real_state=state) == prdc.prdc(Rd, Fd, 5)
    with pytest.raises(ValueError):
        prdc.prdc(Rd, Fd[:5], 5)                                     # k >= n_fake
    with pytest.raises(ValueError):
        prdc.prdc(Rd[:0], Fd, 5)                                     # an empty set


def test_chunked_rows_equal_one_chunk(monkeypatch):
    from contrad_amd import features, prdc
    real, fake, _ = _feature_ref(FEATURE_CASES[0], 1)
    Rd, Fd = torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda()
    whole = prdc.prdc(Rd, Fd, 5)
    monkeypatch.setattr(features, 'MAX_CHUNK_ROWS', 100)             # 300 real rows: 3 chunks; 257 fake rows: 100 + 100 + 57
    assert features.chunk_rows_of(300) == 100 and features.chunk_rows_of(260) == 100      # the patch reaches the rule
    assert prdc.prdc(Rd, Fd, 5) == whole


# ---- through a discriminator ----
def _encoder(seed=3):
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(seed)
    G, D = get_architecture('sndcgan', (32, 32, 3))
    return G, D


def test_prdc_of_through_sndcgan_equals_the_yardstick_on_the_device_S():
    from contrad_amd import lineval, prdc
    from contrad_amd.features import bank_of, extract_features, similarities
    data = lineval.synthetic_set(3, 4, 256, 192)
    _, D = _encoder()
    D = D.cuda().eval()
    for p in D.parameters():
        p.requires_grad_(False)
    real_u8, fake_u8 = torch.from_numpy(data['x_train']).cuda(), torch.from_numpy(data['x_test']).cuda()
    got = prdc.prdc_of(D, real_u8, fake_u8, k=5, batch=100)
    fr, ff = extract_features(D, real_u8, 100), extract_features(D, fake_u8, 100)
    assert tuple(fr.shape) == (256, D.d_penul) and tuple(ff.shape) == (192, D.d_penul)
    br, bf = bank_of(fr), bank_of(ff)
    S_RR = similarities(fr, br, torch.empty(256, 256, device='cuda')).cpu().numpy()
    S_FF = similarities(ff, bf, torch.empty(192, 192, device='cuda')).cpu().numpy()
    S_FR = similarities(ff, br, torch.empty(192, 256, device='cuda')).cpu().numpy()
    ref = R.prdc_from_S(S_RR, S_FF, S_FR, 5)
    for name, v in ref.items():
        assert got[name] == v, (name, got[name], v)                  # exact: integers, and ratios of them in float64
    assert (got['n_real'], got['n_fake'], got['k']) == (256, 192, 5)
    with pytest.raises(ValueError):
        prdc.prdc_of(D, real_u8, fake_u8[:, :16, :16].contiguous(), k=5)
    with pytest.raises(RuntimeError):
        prdc.prdc_of(D.train(), real_u8, fake_u8, k=5)


# ---- scripts ----
SEED = 5
EVAL_SEED = int(np.random.RandomState(SEED).randint(10000))
N_FAKE = 192
_RUNS = {}


def _sampled_reals(gen_paths, arch, n, path, seed=12345):
    """A real set that the fakes can hit: ``n`` images of each generator checkpoint in ``gen_paths`` at latents of their own."""
    from contrad_amd import features
    from contrad_amd.models.gan import get_architecture
    sets = []
    for gen_path in gen_paths:
        G = features.load_frozen(get_architecture(arch, (32, 32, 3))[0], gen_path, torch.device('cuda', 0))
        sets.append(features.sample_u8(G, n, 500, seed).cpu().numpy())
    np.savez(path, x_train=np.concatenate(sets))


def _files(factory):
    """One directory with the frozen encoder and the real set: samples of the generators the plain run has after steps 2
    and 4 (the hooked runs walk the same trajectory, so each of their evaluations finds reals near its fakes and the
    metrics are not trivially zero)."""
    if 'files' not in _RUNS:
        d = factory.mktemp('prdc_files')
        torch.save(_encoder(4)[1].state_dict(), str(d / 'enc.pt'))
        plain = _run(factory, False, False)
        _sampled_reals([os.path.join(plain, 'gen_2.pt'), os.path.join(plain, 'gen_4.pt')], 'sndcgan', 128, str(d / 'real.npz'))
        _RUNS['files'] = d
    return _RUNS['files']


def _hook_flags(factory, best):
    d = _files(factory)
    return ['--prdc_data', str(d / 'real.npz'), '--prdc_encoder', str(d / 'enc.pt'), '--prdc_n', str(N_FAKE)] + \
        (['--prdc_best', best] if best else [])


def _run(factory, graph, hook):
    """train_gan for 4 steps, evaluations at 2 and 4 (both kept as *_2.pt / *_4.pt).  ``hook``: False, '' (the hook without
    --prdc_best) or the metric whose best checkpoints are kept."""
    key = (graph, hook)
    if key not in _RUNS:
        from contrad_amd.train_gan import main
        logdir = str(factory.mktemp('prdc_run'))
        gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
              '--save_every', '2', '--seed', str(SEED), '--logdir', logdir] + (['--graph'] if graph else []) +
             (_hook_flags(factory, hook) if hook is not False else []))
        _RUNS[key] = logdir
    return _RUNS[key]


def _same(a, b):
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif torch.is_tensor(a):
        assert torch.equal(a, b)
    else:
        assert a == b


def _same_files(a, b):
    _same(torch.load(a, map_location='cpu'), torch.load(b, map_location='cpu'))


def _csv_rows(logdir):
    with open(os.path.join(logdir, 'prdc_%d.csv' % EVAL_SEED)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,precision,recall,density,coverage'
    return [(int(v[0]),) + tuple(float(x) for x in v[1:]) for v in (ln.split(',') for ln in lines[1:])]


def test_command_line_writes_the_json(tmp_path_factory, tmp_path):
    import shutil
    import test_prdc
    d = _files(tmp_path_factory)
    gen = str(tmp_path / 'gen.pt')
    shutil.copy(os.path.join(_run(tmp_path_factory, False, False), 'gen.pt'), gen)
    os.makedirs(str(tmp_path / 'samples'))
    _sampled_reals([gen], 'sndcgan', 192, str(tmp_path / 'x.npz'), seed=777)
    with np.load(str(tmp_path / 'x.npz')) as z:
        np.savez(str(tmp_path / 'samples' / 'samples.npz'), images=z['x_train'])
    common = [str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz')]
    path = test_prdc.main(common + ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--seed', '3', '--n_fake', '100'])
    assert path == str(tmp_path / 'samples' / 'prdc_3.json')
    with open(path) as f:
        out = json.load(f)
    assert (out['n_real'], out['n_fake'], out['k']) == (256, 100, 5)
    assert all(0.0 <= out[m] <= 1.0 for m in ('precision', 'recall', 'coverage'))
    assert out['precision'] > 0.0 and out['coverage'] > 0.0 and out['density'] > 0.0                     # not trivially zero
    assert out['precision'] == out['fakes_in_real_balls'] / 100 and out['density'] == out['hits'] / 500
    path = test_prdc.main(common + ['--gen', gen, '--seed', '3', '--n_fake', '64', '--n_real', '200', '--k', '3'])
    assert path == str(tmp_path / 'prdc_3.json')
    with open(path) as f:
        out = json.load(f)
    assert (out['n_real'], out['n_fake'], out['k']) == (200, 64, 3) and out['precision'] > 0.0
    np.savez(str(tmp_path / 'small.npz'), images=np.zeros((8, 16, 16, 3), np.uint8))
    for bad in (['--fake', str(tmp_path / 'small.npz')],                                   # 16 x 16 fakes, 32 x 32 reals
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_fake', '5'],       # k >= n_fake
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_real', '0'],       # an empty set
                ['--gen', gen, '--n_real', '4']):                                             # k >= n_real
        with pytest.raises(ValueError):
            test_prdc.main(common + bad)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_hook_leaves_the_checkpoints_bitwise_alone(graph, tmp_path_factory):
    import test_prdc
    plain, hooked = _run(tmp_path_factory, graph, False), _run(tmp_path_factory, graph, 'density' if graph else 'coverage')
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        _same_files(os.path.join(plain, name), os.path.join(hooked, name))
    rows = _csv_rows(hooked)
    assert [r[0] for r in rows] == [2, 4]
    assert all(0.0 <= v <= 1.0 for r in rows for v in (r[1], r[2], r[4]))
    assert all(r[1] > 0.0 and r[3] > 0.0 and r[4] > 0.0 for r in rows)                 # not trivially zero
    assert not [f for f in os.listdir(plain) if f.startswith('prdc_') or '_best' in f]
    # the logged figures are the checkpoint's: the command line on the saved generator, with the eval seed, gives the last row
    d = _files(tmp_path_factory)
    path = test_prdc.main([str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz'), '--gen', os.path.join(hooked, 'gen.pt'),
                           '--seed', str(EVAL_SEED), '--n_fake', str(N_FAKE)])
    with open(path) as f:
        out = json.load(f)
    assert tuple(float('%.6f' % out[m]) for m in R.METRICS) == rows[-1][1:]


@pytest.mark.parametrize('graph,metric', [(False, 'coverage'), (True, 'density')], ids=['eager-coverage', 'graph-density'])
def test_best_checkpoints_are_those_of_the_best_evaluation(graph, metric, tmp_path_factory):
    hooked = _run(tmp_path_factory, graph, metric)
    col = 1 + R.METRICS.index(metric)
    rows = _csv_rows(hooked)
    best_step = 4 if rows[1][col] > rows[0][col] else 2              # the first evaluation wins on a tie
    print('%s at step 2: %.6f, at step 4: %.6f -> best step %d' % (metric, rows[0][col], rows[1][col], best_step))
    for name in ('gen', 'dis'):
        _same_files(os.path.join(hooked, '%s_best.pt' % name), os.path.join(hooked, '%s_%d.pt' % (name, best_step)))
    assert not os.path.exists(os.path.join(hooked, 'gen_ema_best.pt'))


def test_without_prdc_best_nothing_new_is_written(tmp_path_factory):
    hooked, tracked = _run(tmp_path_factory, False, ''), _run(tmp_path_factory, False, 'coverage')
    assert _csv_rows(hooked) == _csv_rows(tracked)
    assert not [f for f in os.listdir(hooked) if '_best' in f]


def test_stylegan2_loop_with_the_hook_evaluates_gen_ema(tmp_path, tmp_path_factory):
    import test_prdc
    from contrad_amd import config
    from contrad_amd.train_stylegan2 import main
    d = _files(tmp_path_factory)
    args = [os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
            '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
            '--seed', str(SEED)]
    plain, logdir, real = str(tmp_path / 'plain'), str(tmp_path / 'run'), str(tmp_path / 'real.npz')
    main(args + ['--logdir', plain])
    _sampled_reals([os.path.join(plain, 'gen_ema.pt')], 'stylegan2', 128, real)      # reals near what gen_ema makes, not what gen makes
    main(args + ['--logdir', logdir, '--prdc_data', real, '--prdc_encoder', str(d / 'enc.pt'), '--prdc_encoder_arch', 'sndcgan',
                 '--prdc_n', '64', '--prdc_best', 'density'])
    rows = _csv_rows(logdir)
    assert [r[0] for r in rows] == [2] and rows[0][1] > 0.0
    for name in ('gen', 'dis', 'gen_ema'):                            # the first evaluation is the best so far
        _same_files(os.path.join(logdir, '%s_best.pt' % name), os.path.join(logdir, '%s.pt' % name))
        _same_files(os.path.join(logdir, '%s.pt' % name), os.path.join(plain, '%s.pt' % name))
    cli = [str(d / 'enc.pt'), 'sndcgan', '--real', real, '--gen_arch', 'stylegan2', '--seed', str(EVAL_SEED), '--n_fake', '64']
    with open(test_prdc.main(cli + ['--gen', os.path.join(logdir, 'gen_ema.pt')])) as f:
        out = json.load(f)
    assert tuple(float('%.6f' % out[m]) for m in R.METRICS) == rows[-1][1:]          # gen_ema is the generator evaluated
    with open(test_prdc.main(cli + ['--gen', os.path.join(logdir, 'gen.pt')])) as f:
        other = json.load(f)
    print('stylegan2 hook row %s; the command line on gen.pt gives %s' % (rows[-1][1:], tuple(other[m] for m in R.METRICS)))
    assert tuple(float('%.6f' % other[m]) for m in R.METRICS) != rows[-1][1:]        # ... and gen is not


def test_resumed_monitor_reads_the_best_value_up_to_its_checkpoint(tmp_path_factory, tmp_path):
    """The monitor over the csv of the --graph run that tracks density (rows for steps 2 and 4), as a run resumed from step 4, from step 2
    and as a fresh run in the same directory; then one evaluation against each."""
    import shutil
    from contrad_amd import features, prdc
    from contrad_amd.models.gan import get_architecture
    d, hooked = _files(tmp_path_factory), _run(tmp_path_factory, True, 'density')
    rows = _csv_rows(hooked)
    name = 'prdc_%d.csv' % EVAL_SEED
    dev = torch.device('cuda', 0)
    G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, 'gen_4.pt'), dev)

    def monitor(resumed_step, sub):
        logdir = tmp_path / sub
        os.makedirs(str(logdir))
        shutil.copy(os.path.join(hooked, name), str(logdir / name))
        return prdc.PRDCMonitor(str(logdir), 'sndcgan', (32, 32, 3), dev, SEED, str(d / 'real.npz'), str(d / 'enc.pt'), n_fake=N_FAKE,
                                best='density', resumed_step=resumed_step), str(logdir)
    assert rows[1][3] > rows[0][3]                                    # (density rises from step 2 to step 4 in this run)
    m4, dir4 = monitor(4, 'from4')
    m2, _ = monitor(2, 'from2')
    m0, _ = monitor(0, 'fresh')
    assert (m4.best, m2.best, m0.best) == (rows[1][3], rows[0][3], None)
    out = m4.update(6, G)                                             # step 4's generator again: the same figures, a tie
    assert tuple(float('%.6f' % out[m]) for m in R.METRICS) == rows[1][1:] and not out['improved']
    assert [r[0] for r in _csv_rows(dir4)] == [2, 4, 6]               # a resumed run appends to its file
    assert m2.update(4, G)['improved'] and m2.best == rows[1][3]      # the row of step 4 did not count: its evaluation wins again
    assert m0.update(2, G)['improved']


def test_prdc_data_without_an_encoder_is_refused_before_the_first_cuda_call(tmp_path):
    """In a process of its own: after the refusal CUDA is still uninitialised there, whatever call would have started it."""
    import subprocess
    import sys
    np.savez(str(tmp_path / 'real.npz'), x_train=np.zeros((8, 32, 32, 3), np.uint8))
    code = ("import sys, torch\n"
            "sys.path.insert(0, %r)\n"
            "from contrad_amd.train_gan import main\n"
            "try:\n"
            "    main([%r, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', %r,\n"
            "          '--prdc_data', %r])\n"
            "except ValueError as e:\n"
            "    assert '--prdc_encoder' in str(e), e\n"
            "    print('refused; cuda initialised: %%s' %% torch.cuda.is_initialized())\n"
            % (ROOT, os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin'), str(tmp_path / 'run'), str(tmp_path / 'real.npz')))
    done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip().splitlines()[-1] == 'refused; cuda initialised: False', (done.stdout, done.stderr)
    assert not os.path.exists(str(tmp_path / 'run'))                  # ... and before the log directory is made
