"""The float64 yardstick of the rational-quadratic kernel distance (tests/mmd_ref64.py) against a brute-force double loop,
the ``-EINVAL`` cases of ``contrad_mmd_sums`` on host pointers, every host refusal of ``kernel=``, of the intra-class distance,
of ``--intra`` and of ``--prdc_kid_kernel`` (raised before any GPU work), and the defaults that must not move."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import kid_ref64 as K
import mmd_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('shape', [(7, 6, 3, 4, 3), (9, 11, 4, 5, 2), (5, 5, 2, 5, 1)])
def test_yardstick_equals_brute_force(shape):
    from contrad_amd import kid
    n_r, n_f, d, size, n_subsets = shape
    r = np.random.RandomState(0)
    real, fake = r.randn(n_r, d), 0.5 * r.randn(n_f, d) + 0.3
    ref = R.kid_ref64(real, fake, n_subsets, size, seed=3)
    m = min(size, n_r, n_f)
    idx_r, idx_f = kid.subset_indices(n_r, n_f, m, n_subsets, 3)
    brute = R.brute_mmd2(real, fake, idx_r, idx_f)
    assert ref['subset_size'] == m and len(ref['sums']) == n_subsets
    for t, (mmd2, A, B, C) in enumerate(brute):
        for got, want in zip(ref['sums'][t], (A, B, C)):
            assert abs(got - want) <= 1e-12 * abs(want), (t, got, want)
        assert abs(K.mmd2_of(ref['sums'], m)[t] - mmd2) <= 1e-12
    mean = sum(b[0] for b in brute) / n_subsets
    assert abs(ref['kid'] - mean) <= 1e-12
    assert abs(ref['kid_std'] - (sum((b[0] - mean) ** 2 for b in brute) / n_subsets) ** 0.5) <= 1e-12


def test_the_term_its_clamp_and_the_excluded_cell():
    one = np.ones((3, 4), np.float32)
    assert R.block_sum(one) == 36.0 and R.block_sum(one, 0) == 27.0                 # s = 1: u = 0, every term is exactly 3
    assert R.block_sum(np.full((3, 4), 1 + 2.0 ** -20, np.float32)) == 36.0          # the clamp: u < 0 becomes 0
    minus = R.rq_terms(np.float32(-1.0))                                             # u = 4: 1 / sqrt(5) + 1 / 3 + 1 / 4
    assert abs(float(minus) - (5 ** -0.5 + 1 / 3.0 + 0.25)) <= 4 * 2.0 ** -53 and float(minus) >= 1.03
    s = np.linspace(-1, 1, 1001)
    t = R.rq_terms(s)
    assert np.all(np.diff(t) > 0) and np.all(np.diff(t) <= 3 * np.diff(s) * (1 + 1e-9))       # increasing, 3-Lipschitz
    X = one.copy()
    X[1, 1] = np.nan
    assert R.block_sum(X, 0) == 27.0 and math.isfinite(R.block_bound(X, 0))          # left out by index: never seen
    assert math.isnan(R.block_sum(X, -1)) and math.isnan(float(R.rq_terms(np.float32('nan'))))
    assert R.block_sum(np.zeros((1, 1), np.float32), 0) == 0.0 and R.block_bound(np.zeros((1, 1), np.float32), 0) == 0.0
    S = np.clip(np.random.RandomState(1).randn(300, 300), -1, 1).astype(np.float32)
    assert R.block_bound(S, 0) < 1e-3 * 1.03                                          # far below one dropped cell


def test_a_characteristic_kernel_separates_what_the_cubic_cannot():
    """Two sets on the unit circle with the same moments up to order 3 (the corners of a square against those of the square
    turned by 45 degrees: equal Fourier coefficients below order 4): the cubic kernel puts them at 0, rq does not."""
    a = np.arange(4) * np.pi / 2
    P = np.stack([np.cos(a), np.sin(a)], 1)
    Q = np.stack([np.cos(a + np.pi / 4), np.sin(a + np.pi / 4)], 1)
    biased = lambda k: (k(P @ P.T).mean() + k(Q @ Q.T).mean() - 2 * k(Q @ P.T).mean())      # V-statistic: exact population MMD^2
    assert abs(biased(lambda S: (S + 1.0) ** 3)) <= 1e-14
    assert biased(R.rq_terms) > 1e-3


@pytest.mark.parametrize('seed', [0, 1])
def test_the_float64_distance_of_the_gpu_tests_sets_is_far_above_their_bound(seed):
    """tests/test_kid_kernels_gpu.py holds the device within 12 e of this number (d = 24, 8 subsets of 100 of 300 x 257 rows
    moved by 1.5): it must exceed 4 times that, so that a wrong divisor or a swapped block shows."""
    real, fake = K.shifted_sets(seed, 24, 300, 257, 1.5)
    ref, same = R.kid_ref64(real, fake, 8, 100, seed), R.kid_ref64(*K.shifted_sets(seed, 24, 300, 257, 0.0), 8, 100, seed)
    print('float64 kid_rq of the shifted sets %.6f (unshifted %.6f), bound %.3g' % (ref['kid'], same['kid'], R.feature_bound(24)))
    assert R.feature_bound(24) == 12 * 56 * 2.0 ** -24 and ref['kid'] > 4 * R.feature_bound(24)
    assert abs(same['kid']) < 0.25 * ref['kid']


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def test_entry_point_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    query, f = lib().raw('contrad_kid_sums_workspace_bytes'), lib().raw('contrad_mmd_sums')
    M, n = 2, 8
    need = query(M, n)
    S, out, ws = (ctypes.c_float * (M * n))(), (ctypes.c_double * 1)(-7.0), (ctypes.c_double * (need // 8 + 1))()

    def call(S=S, ldS=n, M=M, n=n, self0=0, kind=1, gamma=1.0, coef0=1.0, accumulate=0, out=out, ws=ws, ws_bytes=need):
        return f(_vp(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), kind, gamma, coef0, accumulate, _vp(out), _vp(ws),
                 ctypes.c_longlong(ws_bytes), ctypes.c_void_p(0))

    for bad in (dict(kind=2), dict(kind=-1), dict(kind=3), dict(S=None), dict(out=None), dict(M=0), dict(n=0), dict(M=-1),
                dict(ldS=n - 1), dict(gamma=float('nan')), dict(gamma=float('inf')), dict(coef0=float('nan')),
                dict(coef0=-float('inf')), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(accumulate=1, out=None)):
        assert call(**bad) == -22, bad
        bad0 = dict(bad)
        bad0.setdefault('kind', 0)
        assert call(**bad0) == -22, bad0
    assert out[0] == -7.0 and all(v == 0.0 for v in ws)


def test_python_layer_refusals():
    from contrad_amd import kid, ops
    assert kid.KERNELS == ('poly3', 'rq') and set(kid.KERNEL_NOTES) == set(kid.KERNELS)
    assert kid.KERNEL_NOTES['poly3'] is kid.KERNEL_NOTE and 'alpha' in kid.KERNEL_NOTES['rq'] and '0.2, 0.5, 1, 2, 5' in kid.KERNEL_NOTES['rq']
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.mmd_sums(torch.zeros(2, 8), 8, 'rq')                       # host S
    f = torch.zeros(8, 4)
    for call in (lambda: kid.kid(f, f, kernel='gauss'), lambda: kid.kid(f, f, kernel=None), lambda: kid.kid(f, f, kernel=1),
                 lambda: kid.kid_of(None, None, None, kernel='RQ'),
                 lambda: kid.intra_class_kid(f, [0] * 8, f, [0] * 8, 1, kernel='gauss')):
        with pytest.raises(ValueError, match='unknown kernel'):
            call()
    for bad in (dict(n_subsets=0), dict(subset_size=1)):               # the size refusals hold for rq too, on the host
        with pytest.raises(ValueError, match='kid: '):
            kid.kid(f, f, kernel='rq', **bad)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        kid.kid(f, f, kernel='rq')                                     # ... and host tensors get no further


def test_intra_class_refusals_come_before_any_gpu_work():
    from contrad_amd import kid
    was_initialised = torch.cuda.is_initialized()
    f = torch.zeros(8, 4)
    good = np.array([0, 0, 1, 1, 2, 2, 2, 0])
    for yr, yf, n_classes, match in (
            (np.array([0, 0, 1, 1, 2, 2, 2, 3]), good, 3, 'outside'),               # a label past n_classes
            (good, np.array([0, 0, 1, 1, 2, 2, 2, -1]), 3, 'outside'),              # a negative label
            (np.array([0, 0, 1, 2, 2, 2, 2, 0]), good, 3, 'class 1 has 1 real'),    # a class of one row
            (good, np.array([0, 0, 0, 1, 1, 1, 1, 1]), 3, 'class 2 has 3 real and 0 fake'),
            (good[:7], good, 3, 'one integer per row'),                            # lengths differ
            (good, good[:5], 3, 'one integer per row'),
            (good.astype(np.float64), good, 3, 'one integer per row'),
            (good, good, 0, 'n_classes')):
        with pytest.raises(ValueError, match=match):
            kid.intra_class_kid(f, yr, f, yf, n_classes)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        kid.intra_class_kid(f, good, f, torch.from_numpy(good), 3)     # valid labels (arrays or tensors): as far as the device check
    rows = kid.class_rows(good, good[::-1].copy(), 8, 8, 3)
    assert [r.tolist() for r, _ in rows] == [[0, 1, 7], [2, 3], [4, 5, 6]] and [f_.tolist() for _, f_ in rows] == [[0, 6, 7], [4, 5], [1, 2, 3]]
    assert kid.intra_of([dict(kid=1.0), dict(kid=2.0), dict(kid=6.0)]) == R.intra_of([1.0, 2.0, 6.0]) == (3.0, math.sqrt(14.0 / 3))
    assert torch.cuda.is_initialized() == was_initialised


def test_command_line_defaults_and_intra_refusals(tmp_path):
    from contrad_amd import kid
    P = kid.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--gen', 'run/gen.pt'])
    assert (P.n_subsets, P.subset_size, P.n_real, P.n_fake, P.batch_size, P.seed, P.gen_arch, P.fake) == \
        (100, 1000, None, None, 500, None, None, None)                 # as they were
    assert (P.kernel, P.intra, P.n_classes) == ('poly3', False, None)
    with pytest.raises(SystemExit):
        kid.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--gen', 'g.pt', '--kernel', 'gauss'])
    assert (kid.json_name('poly3'), kid.json_name('rq'), kid.json_name('poly3', True), kid.json_name('rq', True)) == \
        ('kid_%d.json', 'kid_rq_%d.json', 'kid_intra_%d.json', 'kid_intra_rq_%d.json')
    was_initialised = torch.cuda.is_initialized()
    x = np.zeros((6, 32, 32, 3), np.uint8)
    y = np.array([0, 0, 0, 1, 1, 1])
    real, real_nolabels = str(tmp_path / 'real.npz'), str(tmp_path / 'real_nolabels.npz')
    fake, fake_nolabels = str(tmp_path / 'fake.npz'), str(tmp_path / 'fake_nolabels.npz')
    np.savez(real, x_train=x, y_train=y)
    np.savez(real_nolabels, x_train=x)
    np.savez(fake, images=x, labels=y)
    np.savez(fake_nolabels, images=x)
    common = ['enc/dis.pt', 'sndcgan', '--intra']
    with pytest.raises(ValueError, match='--intra needs --fake'):
        kid.main(common + ['--real', real, '--gen', str(tmp_path / 'gen.pt')])
    with pytest.raises(ValueError, match='holds no y_train'):
        kid.main(common + ['--real', real_nolabels, '--fake', fake])
    with pytest.raises(ValueError, match='holds no labels'):
        kid.main(common + ['--real', real, '--fake', fake_nolabels])
    with pytest.raises(ValueError, match='--n_classes does nothing without --intra'):
        kid.main(['enc/dis.pt', 'sndcgan', '--real', real, '--fake', fake, '--n_classes', '2'])
    assert torch.cuda.is_initialized() == was_initialised


def test_hook_flag_parses_and_is_refused_before_any_cuda_call(tmp_path):
    from contrad_amd import prdc, train_gan, train_stylegan2
    was_initialised = torch.cuda.is_initialized()
    on = ['--prdc_data', 'c10.npz', '--prdc_encoder', 'e.pt']
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'])
        assert not hasattr(Q, 'prdc_kid_kernel') and prdc.check_hook_arguments(Q).prdc_kid_kernel == 'poly3'     # off, and no attribute
        with_flag = vars(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid', '--prdc_kid_kernel', 'rq']))
        assert {k: v for k, v in with_flag.items() if not k.startswith('prdc_')} == vars(Q)       # the default dict is what it was
        H = prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid', '--prdc_kid_kernel', 'rq', '--prdc_best', 'kid']))
        assert (H.prdc_kid, H.prdc_kid_kernel, H.prdc_best) == (True, 'rq', 'kid')
        assert prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid'])).prdc_kid_kernel == 'poly3'
        with pytest.raises(ValueError, match='--prdc_kid_kernel needs --prdc_kid'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid_kernel', 'rq']))
        with pytest.raises(ValueError, match='--prdc_kid_kernel needs --prdc_kid'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid_kernel', 'poly3']))
        with pytest.raises(ValueError, match='nothing without --prdc_data'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_kid_kernel', 'rq']))
        with pytest.raises(SystemExit):
            mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid', '--prdc_kid_kernel', 'gauss'])
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    common = [gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', str(tmp_path / 'run')]
    with pytest.raises(ValueError, match='--prdc_kid_kernel needs --prdc_kid'):
        train_gan.main(common + ['--prdc_data', str(tmp_path / 'real.npz'), '--prdc_encoder', str(tmp_path / 'e.pt'), '--prdc_kid_kernel', 'rq'])
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(str(tmp_path / 'run'))
    assert (prdc.kid_csv_name('poly3'), prdc.kid_csv_name('rq')) == ('kid_%d.csv', 'kid_rq_%d.csv')
    assert prdc.BEST_CHOICES == prdc.METRICS + ('kid',)
