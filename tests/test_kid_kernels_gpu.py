"""The rational-quadratic kernel of the kernel distance and the intra-class distance on the GPU against the yardstick
(tests/mmd_ref64.py): ``contrad_mmd_sums`` alone on a given S (kind 1 within the derived bound, kind 0 bit for bit
``contrad_kid_sums``), ``kid(kernel='rq')`` on the device's own similarities and against float64 features,
``intra_class_kid``, the command line (``--kernel rq``, ``--intra``) and ``--prdc_kid_kernel rq`` of the training scripts.

Bounds (derived, not measured; tests/mmd_ref64.py).  On a given fp32 S the device sum must lie within ``(M n + 32) 2^-53
fsum(|terms|)`` of the ``math.fsum`` of the float64 terms; the lightest cell weighs at least 0.3 / (M n) of the sum, 3e-7 at
1000 x 1000 against a bound near 1e-10.  On features a device similarity is within e = (2 d + 8) 2^-24 of the float64 one
and the term is 3-Lipschitz in s, so |kid_rq - ref64| <= 12 e (4.0e-5 at d = 24); the float64 distance of the shifted sets
is checked to exceed 4 times that.  Every figure is printed before it is asserted.

Observed on the MI355X: kernel on a given S |out - fsum| <= 4.7e-10 on a sum of 1.03e6 and at most
0.036 of the bound; sums on the device's own S at most 1.9e-4 of the bound; |kid_rq - ref64| 3.0e-9 and 1.6e-9."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import kid_ref64 as K
import mmd_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NAN = float('nan')

SUM_SHAPES = [(1, 1, -1), (1, 1, 0), (3, 7, 0), (7, 3, 0), (7, 3, 5), (65, 300, -1), (300, 300, 0), (257, 1025, 5),
              (1000, 1000, 0), (4, 70000, -1), (4, 70000, 123)]
_SUM_REF = {}


def _bits(x):
    return np.float64(x).view(np.uint64)


def _excluded(M, n, self0):
    return [(i, self0 + i) for i in range(M) if 0 <= self0 + i < n] if self0 >= 0 else []


def _live_cell(M, n, self0):
    """One cell that counts (None: there is none), the last one where it can be."""
    for i, j in ((M - 1, n - 1), (M // 2, n // 2), (0, 0), (0, n - 1)):
        if self0 < 0 or j != self0 + i:
            return i, j
    return None


def _sum_inputs(shape):
    """{name: (S, fsum, bound)} for a shape, made once.  The excluded cells hold NaN in every S: they must never be seen."""
    if shape not in _SUM_REF:
        M, n, self0 = shape
        r = np.random.RandomState(0)
        data = {'random': r.uniform(-1, 1, (M, n)).astype(np.float32), 'ones': np.ones((M, n), np.float32),
                'clamp': np.full((M, n), 1 + 2.0 ** -20, np.float32), 'minus': np.full((M, n), -1.0, np.float32)}
        cell = _live_cell(M, n, self0)
        if cell is not None:
            data['nan'] = data['random'].copy()
            data['nan'][cell] = NAN
        for S in data.values():
            for c in _excluded(M, n, self0):
                S[c] = NAN
        _SUM_REF[shape] = {name: (S, R.block_sum(S, self0), R.block_bound(S, self0)) for name, S in data.items()}
    return _SUM_REF[shape]


def _device_S(S, pad):
    """S on the device with ``pad`` columns of NaN behind every row: a padding column that is read shows."""
    M, n = S.shape
    view = torch.full((M, n + pad), NAN, device='cuda')
    view[:, :n] = torch.from_numpy(S).cuda()
    return view


def _raw(view, M, n, self0, kind=1, gamma=1.0, coef0=1.0, accumulate=False, out=None, row0=0, entry='contrad_mmd_sums'):
    """The entry point on rows [row0, row0 + M) of ``view`` with guard bands around ``out`` and around a workspace of exactly
    the size the query names.  Returns (the float64 result, the guarded out buffer)."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    if out is None:
        out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    nbytes = lib().raw('contrad_kid_sums_workspace_bytes')(M, n)
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    rows = view[row0:row0 + M]
    head = (ops._p(rows), ctypes.c_longlong(view.stride(0)), M, n, ctypes.c_longlong(self0))
    tail = (gamma, coef0, 1 if accumulate else 0, ops._p(out[GUARD:]), ops._p(ws[GUARD:]), ctypes.c_longlong(nbytes), ops._stream())
    rc = lib().raw(entry)(*(head + ((kind,) if entry == 'contrad_mmd_sums' else ()) + tail))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf in (out, ws):
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all()), 'guard band overwritten'
    return float(out[GUARD]), out


# ---- contrad_mmd_sums on a given S ----
@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', SUM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rq_sums_kernel_on_a_given_S(shape, pad):
    M, n, self0 = shape
    cells = M * n - len(_excluded(M, n, self0))
    for name, (S, ref, bound) in _sum_inputs(shape).items():
        tag = 'mmd sums rq %s %s ld+%d' % ('x'.join(map(str, shape)), name, pad)
        view = _device_S(S, pad)
        got, _ = _raw(view, M, n, self0)
        print('%s: device %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (tag, got, ref, abs(got - ref), bound))
        if name == 'nan':
            assert math.isnan(got) and math.isnan(ref), tag + ': a NaN inside a live cell was lost'
            continue
        assert abs(got - ref) <= bound, tag
        if name in ('ones', 'clamp'):
            assert ref == 3.0 * cells and got == ref, tag               # every term is 3: the sum is exact
        if shape == (1, 1, 0):
            assert got == 0.0, tag                                      # the only cell is the one left out
        again, _ = _raw(view, M, n, self0)
        assert _bits(got) == _bits(again), tag + ': two calls differ'


@pytest.mark.parametrize('shape', [(7, 3, 5), (300, 300, 0), (257, 1025, 5), (4, 70000, 123)], ids=lambda s: 'x'.join(map(str, s)))
def test_accumulate_over_two_row_chunks(shape):
    M, n, self0 = shape
    S, ref, bound = _sum_inputs(shape)['random']
    m1 = (M + 1) // 2 if M < 200 else 129                               # (129: one row past eight 16-row tiles)
    b1 = R.block_bound(S[:m1], self0)
    for pad in (0, 3):
        view = _device_S(S, pad)
        first, out = _raw(view, m1, n, self0)
        assert abs(first - R.block_sum(S[:m1], self0)) <= b1
        both, _ = _raw(view, M - m1, n, self0 + m1, accumulate=True, out=out, row0=m1)
        print('mmd sums rq %s ld+%d in chunks of %d + %d rows: %.17g  fsum %.17g  |diff| %.3g  bound %.3g'
              % ('x'.join(map(str, shape)), pad, m1, M - m1, both, ref, abs(both - ref), bound))
        assert abs(both - ref) <= bound                                 # the whole-block reference, the whole-block bound
        out2 = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
        _raw(view, m1, n, self0, out=out2)
        again, _ = _raw(view, M - m1, n, self0 + m1, accumulate=True, out=out2, row0=m1)
        assert _bits(both) == _bits(again)
    view = _device_S(S, 0)
    out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    out[GUARD] = 1e6                                                    # accumulate adds to what is there, and only then
    got, _ = _raw(view, M, n, self0, accumulate=True, out=out)
    assert abs(got - (1e6 + ref)) <= bound + 2.0 ** -53 * (1e6 + ref)
    got, _ = _raw(view, M, n, self0, accumulate=False, out=out)
    assert abs(got - ref) <= bound


@pytest.mark.parametrize('shape', [(7, 3, 5), (257, 1025, 5), (1000, 1000, 0)], ids=lambda s: 'x'.join(map(str, s)))
def test_kind_0_is_contrad_kid_sums_bit_for_bit(shape):
    from contrad_amd import ops
    M, n, self0 = shape
    S = _sum_inputs(shape)['random'][0]
    for pad in (0, 3):
        view = _device_S(S, pad)
        for gamma, coef0 in ((1.0, 1.0), (0.5, 2.0), (1.0 / 300, 1.0)):
            old, _ = _raw(view, M, n, self0, gamma=gamma, coef0=coef0, entry='contrad_kid_sums')
            new, _ = _raw(view, M, n, self0, kind=0, gamma=gamma, coef0=coef0)
            assert math.isfinite(old) and _bits(old) == _bits(new), (shape, pad, gamma, coef0, old, new)
            assert abs(old - K.block_sum(S, self0, gamma, coef0)) <= K.block_bound(S, self0, gamma, coef0)
    view = _device_S(S, 0)
    for kind, name in ((0, 'poly3'), (1, 'rq')):                        # the wrapper is the entry point
        want, _ = _raw(view, M, n, self0, kind=kind)
        for k in (kind, name):
            out = ops.mmd_sums(view, n, k, self0=self0)
            assert out.dtype == torch.float64 and tuple(out.shape) == (1,) and _bits(float(out)) == _bits(want)
    assert _bits(float(ops.kid_sums(view, n, self0=self0))) == _bits(_raw(view, M, n, self0, kind=0)[0])
    for bad in (dict(kind='gauss'), dict(kind=2), dict(gamma=NAN), dict(accumulate=True), dict(out=torch.zeros(1, device='cuda'))):
        a = dict(kind='rq'); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.mmd_sums(view, n, **a)


def test_entry_point_returns_einval_on_device_pointers():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    f, query = lib().raw('contrad_mmd_sums'), lib().raw('contrad_kid_sums_workspace_bytes')
    S = torch.zeros(2, 8, device='cuda')
    out = torch.full((1,), -7.0, dtype=torch.float64, device='cuda')
    need = query(2, 8)
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device='cuda')
    for a in (dict(kind=2), dict(kind=-1), dict(S=None), dict(out=None), dict(M=0), dict(n=0), dict(ldS=7), dict(gamma=NAN),
              dict(coef0=float('inf')), dict(ws=None), dict(ws_bytes=need - 1)):
        for kind in ((1, 0) if 'kind' not in a else (a['kind'],)):
            b = dict(S=S, ldS=8, M=2, n=8, gamma=1.0, coef0=1.0, out=out, ws=ws, ws_bytes=need); b.update(a)
            assert f(ops._p(b['S']), ctypes.c_longlong(b['ldS']), b['M'], b['n'], ctypes.c_longlong(0), kind, b['gamma'], b['coef0'], 0,
                     ops._p(b['out']), ops._p(b['ws']), ctypes.c_longlong(b['ws_bytes']), ops._stream()) == -22, (a, kind)
    torch.cuda.synchronize()
    assert float(out) == -7.0 and bool((ws == -7.0).all())


# ---- kid(kernel='rq') on the device's own similarities ----
OWN_S_CASES = [(24, 300, 257, 100, 8), (512, 1000, 900, 1000, 3)]
SHIFT = 1.5
_SETS = {}


def _sets(case, seed):
    if (case, seed) not in _SETS:
        d, n_r, n_f, _, _ = case
        real, fake = K.shifted_sets(seed, d, n_r, n_f, SHIFT)
        _SETS[case, seed] = (real, fake, torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda())
    return _SETS[case, seed]


def _device_blocks(real_rows, fake_rows, idx_r, idx_f):
    """The three fp32 similarity blocks the device forms for one subset of normalised device rows, read back."""
    from contrad_amd import features, kid
    dev = fake_rows.device
    R_t, F_t, bank_R, bank_F = kid.gather_subset(real_rows, None, fake_rows, torch.from_numpy(idx_r).to(dev), torch.from_numpy(idx_f).to(dev))
    m = len(idx_r)
    read = lambda q, bank: np.concatenate([S[:, :m].cpu().numpy() for _, S in features.similarity_chunks(q, bank)])
    return read(R_t, bank_R), read(F_t, bank_F), read(F_t, bank_R)


@pytest.mark.parametrize('case', OWN_S_CASES, ids=lambda c: 'd%d-%dx%d-m%d-t%d' % c)
def test_rq_kid_sums_on_the_devices_own_similarities(case):
    from contrad_amd import features, kid
    d, n_r, n_f, size, T = case
    _, _, Rd, Fd = _sets(case, 0)
    got = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3, kernel='rq')
    m = min(size, n_r, n_f)
    assert (got['n_subsets'], got['subset_size'], got['n_real'], got['n_fake'], got['seed'], got['kernel_name']) == (T, m, n_r, n_f, 3, 'rq')
    assert got['kernel'] == kid.KERNEL_NOTES['rq'] and 'gamma' not in got and 'degree' not in got
    Rn, Fn = features.normalize_rows(Rd), features.normalize_rows(Fd)
    idx_r, idx_f = kid.subset_indices(n_r, n_f, m, T, 3)
    worst = 0.0
    for t in range(T):
        for c, (S, self0) in enumerate(zip(_device_blocks(Rn, Fn, idx_r[t], idx_f[t]), (0, 0, -1))):
            assert S.shape == (m, m) and S.dtype == np.float32
            ref, bound = R.block_sum(S, self0), R.block_bound(S, self0)
            err = abs(got['sums'][t][c] - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (t, 'ABC'[c], got['sums'][t][c], ref, bound)
    print('kid rq own S d%d %dx%d m%d t%d: kid %.6f +- %.6f; largest |device sum - fsum| / bound %.3g' % (case + (got['kid'], got['kid_std'], worst)))
    assert (got['kid'], got['kid_std']) == K.kid_of_sums(got['sums'], m)                      # the host formula on the table, exactly
    assert kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3, kernel='rq') == got            # two calls: the same dict
    assert kid.kid(Rn, Fn, n_subsets=T, subset_size=size, seed=3, normalize=False, kernel='rq') == got
    banked = kid.kid(None, Fn, n_subsets=T, subset_size=size, seed=3, normalize=False, real_bank=(features.bank_of(Rn), n_r), kernel='rq')
    assert banked == got                                                # the hook's form of the real set: the same floats
    poly = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3)
    assert poly['kernel_name'] == 'poly3' and poly['kernel'] == kid.KERNEL_NOTE and poly['sums'] != got['sums']
    assert kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=3, kernel='poly3') == poly       # the default, named


# ---- against float64 features ----
@pytest.mark.parametrize('seed', [0, 1])
def test_rq_kid_on_features_against_float64(seed):
    from contrad_amd import kid
    case = OWN_S_CASES[0]
    d, n_r, n_f, size, T = case
    real, fake, Rd, Fd = _sets(case, seed)
    ref, bound = R.kid_ref64(real, fake, T, size, seed), R.feature_bound(d)
    got = kid.kid(Rd, Fd, n_subsets=T, subset_size=size, seed=seed, kernel='rq')
    print('kid rq features d%d %dx%d m%d t%d seed %d: device %.9f  float64 %.9f  |diff| %.3g  bound %.3g  (std device %.6f float64 %.6f)'
          % (case + (seed, got['kid'], ref['kid'], abs(got['kid'] - ref['kid']), bound, got['kid_std'], ref['kid_std'])))
    assert ref['kid'] > 4 * bound                                       # a wrong divisor or a swapped block shows
    assert got['subset_size'] == ref['subset_size'] and abs(got['kid'] - ref['kid']) <= bound
    assert abs(got['kid_std'] - ref['kid_std']) <= bound                # (std is a seminorm: it moves by at most max |e_t|)


# ---- intra-class ----
def test_intra_class_kid_is_kid_per_class():
    from contrad_amd import kid
    case = OWN_S_CASES[0]
    d, n_r, n_f, _, _ = case
    real, fake, Rd, Fd = _sets(case, 0)
    rng = np.random.default_rng(5)
    y_r = rng.permutation(np.repeat([0, 1, 2], [150, 148, 2]))           # 3 classes of unequal size, the smallest with 2 rows
    y_f = rng.permutation(np.repeat([0, 1, 2], [200, 55, 2]))
    T, size = 4, 100
    for kernel, bound, ref_mod in (('rq', R.feature_bound(d), R), ('poly3', 12 * (2 + 56 * 2.0 ** -24) ** 2 * 56 * 2.0 ** -24, K)):
        got = kid.intra_class_kid(Rd, y_r, Fd, torch.from_numpy(y_f), 3, n_subsets=T, subset_size=size, seed=9, kernel=kernel)
        assert (got['n_classes'], got['seed'], got['kernel_name'], got['kernel']) == (3, 9, kernel, kid.KERNEL_NOTES[kernel])
        assert [c['subset_size'] for c in got['classes']] == [100, 55, 2] and [c['n_real'] for c in got['classes']] == [150, 148, 2]
        for c in range(3):
            rows_r, rows_f = torch.from_numpy(np.flatnonzero(y_r == c)).cuda(), torch.from_numpy(np.flatnonzero(y_f == c)).cuda()
            alone = kid.kid(Rd[rows_r], Fd[rows_f], n_subsets=T, subset_size=size, seed=9, kernel=kernel)
            assert got['classes'][c] == alone, (kernel, c)
        values = [c['kid'] for c in got['classes']]
        assert (got['kid_intra'], got['kid_intra_std']) == (float(np.mean(np.asarray(values, np.float64))), float(np.std(np.asarray(values, np.float64))))
        mean, std = R.intra_of(values)                                  # ... and by hand, to a rounding of the mean
        assert abs(got['kid_intra'] - mean) <= 4 * 2.0 ** -53 * abs(mean) + 2.0 ** -60 and abs(got['kid_intra_std'] - std) <= 2.0 ** -45
        ref_values, ref_mean, _ = R.intra_ref64(real, y_r, fake, y_f, 3, T, size, 9, kernel)
        print('intra-class %s: device %s mean %.9f; float64 %s mean %.9f; bound %.3g' % (kernel, values, got['kid_intra'], ref_values, ref_mean, bound))
        assert all(abs(a - b) <= bound for a, b in zip(values, ref_values)) and abs(got['kid_intra'] - ref_mean) <= bound
    for yr, yf, n_classes in ((y_r, y_f, 2), (np.where(y_r == 2, 1, y_r), y_f, 3), (y_r[:-1], y_f, 3)):
        with pytest.raises(ValueError):
            kid.intra_class_kid(Rd, yr, Fd, yf, n_classes)


# ---- scripts ----
def _labelled_files(tmp_path):
    """A frozen encoder file, a real npz with y_train and a samples.npz with labels (4 classes, 256 and 192 images)."""
    import test_prdc_gpu as TP
    from contrad_amd import lineval
    data = lineval.synthetic_set(3, 4, 256, 192)
    enc, real, fake = str(tmp_path / 'enc.pt'), str(tmp_path / 'real.npz'), str(tmp_path / 'samples' / 'samples.npz')
    os.makedirs(str(tmp_path / 'samples'))
    torch.save(TP._encoder(4)[1].state_dict(), enc)
    np.savez(real, x_train=data['x_train'], y_train=data['y_train'])
    np.savez(fake, images=data['x_test'], labels=data['y_test'])
    return enc, real, fake, data


def test_command_line_with_kernel_rq_and_with_intra(tmp_path):
    import test_kid
    from contrad_amd import kid
    enc, real, fake, data = _labelled_files(tmp_path)
    common = [enc, 'sndcgan', '--real', real, '--fake', fake, '--seed', '3', '--n_subsets', '5', '--subset_size', '64']
    load = lambda path: json.load(open(path))
    path = test_kid.main(common + ['--kernel', 'rq'])
    assert path == str(tmp_path / 'samples' / 'kid_rq_3.json')
    rq = load(path)
    assert (rq['kernel_name'], rq['n_real'], rq['n_fake'], rq['n_subsets'], rq['subset_size'], rq['seed']) == ('rq', 256, 192, 5, 64, 3)
    assert (rq['kid'], rq['kid_std']) == K.kid_of_sums(rq['sums'], 64) and 'alpha' in rq['kernel'] and 'gamma' not in rq
    path = test_kid.main(common)
    assert path == str(tmp_path / 'samples' / 'kid_3.json')
    poly = load(path)
    assert poly['kernel_name'] == 'poly3' and poly['kernel'] == kid.KERNEL_NOTE and (poly['gamma'], poly['coef0'], poly['degree']) == (1.0, 1.0, 3)
    assert poly['sums'] != rq['sums']
    for kernel, name in (('poly3', 'kid_intra_3.json'), ('rq', 'kid_intra_rq_3.json')):
        path = test_kid.main(common + ['--intra', '--kernel', kernel])
        assert path == str(tmp_path / 'samples' / name)
        out = load(path)
        assert out['n_classes'] == 4 and len(out['classes']) == 4 and out['kernel_name'] == kernel
        for c, per in enumerate(out['classes']):                        # every class's value is listed
            n_r, n_f = int((data['y_train'] == c).sum()), int((data['y_test'] == c).sum())
            assert (per['n_real'], per['n_fake'], per['subset_size'], per['seed']) == (n_r, n_f, min(64, n_r, n_f), 3)
            assert (per['kid'], per['kid_std']) == K.kid_of_sums(per['sums'], per['subset_size'])
        assert (out['kid_intra'], out['kid_intra_std']) == kid.intra_of(out['classes'])
        # what the marginal distance cannot see: every fake under the wrong class
        wrong = str(tmp_path / 'samples' / 'wrong.npz')
        np.savez(wrong, images=data['x_test'], labels=(data['y_test'] + 1) % 4)
        args = [a if a != fake else wrong for a in common]
        moved = load(test_kid.main(args + ['--intra', '--kernel', kernel, '--n_classes', '4']))
        marginal = load(test_kid.main(args + ['--kernel', kernel]))
        print('%s: kid_intra %.6f, with every fake under the next class %.6f; marginal kid %.6f both ways'
              % (kernel, out['kid_intra'], moved['kid_intra'], marginal['kid']))
        assert marginal['kid'] == (poly if kernel == 'poly3' else rq)['kid'] and moved['kid_intra'] > out['kid_intra']
    for bad in (['--intra', '--n_classes', '3'],                        # a label outside [0, 3)
                ['--intra', '--n_fake', '1']):                          # classes without two fakes
        with pytest.raises(ValueError):
            test_kid.main(common + bad)


def test_hook_with_the_rq_kernel_writes_its_own_csv(tmp_path_factory, tmp_path):
    import shutil
    import test_prdc_gpu as TP
    from contrad_amd import features, prdc
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_gan import main
    plain, prdc_only = TP._run(tmp_path_factory, False, False), TP._run(tmp_path_factory, False, '')
    logdir = str(tmp_path / 'run')
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', logdir] + TP._hook_flags(tmp_path_factory, None) +
         ['--prdc_kid', '--prdc_kid_kernel', 'rq', '--prdc_best', 'kid'])
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(logdir, name))
    csv, rq_csv = 'prdc_%d.csv' % TP.EVAL_SEED, 'kid_rq_%d.csv' % TP.EVAL_SEED
    with open(os.path.join(prdc_only, csv), 'rb') as a, open(os.path.join(logdir, csv), 'rb') as b:
        assert a.read() == b.read()                                     # byte for byte the rows of --prdc_data alone
    assert [f for f in os.listdir(logdir) if f.startswith('kid_')] == [rq_csv]                  # no kid_<seed>.csv
    with open(os.path.join(logdir, rq_csv)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,kid,kid_std'
    rows = [(int(v[0]), float(v[1]), float(v[2])) for v in (ln.split(',') for ln in lines[1:])]
    print('kid_rq rows: %s' % (rows,))
    assert [r[0] for r in rows] == [2, 4] and all(math.isfinite(r[1]) and r[2] >= 0.0 for r in rows)
    with open(os.path.join(logdir, 'log.txt')) as f:
        log = f.read()
    assert all('[kid_rq %.6f +- %.6f]' % r[1:] in log for r in rows) and '[kid ' not in log
    best_step = 4 if rows[1][1] < rows[0][1] else 2                     # --prdc_best kid tracks this file's minimum
    for name in ('gen', 'dis'):
        TP._same_files(os.path.join(logdir, '%s_best.pt' % name), os.path.join(logdir, '%s_%d.pt' % (name, best_step)))
    # the read-back on --resume comes from kid_rq_<seed>.csv; the row is what the command line gives on the saved generator
    d, dev = TP._files(tmp_path_factory), torch.device('cuda', 0)
    os.makedirs(str(tmp_path / 'resumed'))
    for name in (csv, rq_csv):
        shutil.copy(os.path.join(logdir, name), str(tmp_path / 'resumed' / name))
    m = prdc.PRDCMonitor(str(tmp_path / 'resumed'), 'sndcgan', (32, 32, 3), dev, TP.SEED, str(d / 'real.npz'), str(d / 'enc.pt'),
                         n_fake=TP.N_FAKE, best='kid', resumed_step=2, kid=True, kid_kernel='rq')
    assert m.best == rows[0][1]
    G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(logdir, 'gen_4.pt'), dev)
    out = m.update(4, G)
    assert (float('%.6f' % out['kid']), float('%.6f' % out['kid_std'])) == rows[1][1:] and out['improved'] == (rows[1][1] < rows[0][1])
    assert sorted(f for f in os.listdir(str(tmp_path / 'resumed')) if f.startswith('kid_')) == [rq_csv]
    with pytest.raises(ValueError, match='--prdc_kid_kernel needs --prdc_kid'):
        prdc.PRDCMonitor(str(tmp_path), 'sndcgan', (32, 32, 3), dev, TP.SEED, str(d / 'real.npz'), str(d / 'enc.pt'), n_fake=TP.N_FAKE, kid_kernel='rq')
