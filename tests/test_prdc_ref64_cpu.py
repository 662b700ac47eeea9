"""The float64 yardstick of precision / recall / density / coverage (tests/prdc_ref64.py) against a brute-force double
loop, its tie / NaN / -0.0 rules, the decided-indicator intervals, and the argument errors of the Python layer and of the
two C entry points (raised before any GPU call)."""
import ctypes

import numpy as np
import pytest
import torch

import prdc_ref64 as R


def _unit(rows):
    return [[x / max(sum(v * v for v in r) ** 0.5, 1e-12) for x in r] for r in rows]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _kth_others(X, i, k):
    """k-th largest similarity of row i of X to the other rows, self left out by index."""
    return sorted((_dot(X[i], X[j]) for j in range(len(X)) if j != i), reverse=True)[k - 1]


def _brute(real, fake, k):
    Rn, Fn = _unit(real.tolist()), _unit(fake.tolist())
    t_R = [_kth_others(Rn, i, k) for i in range(len(Rn))]
    t_F = [_kth_others(Fn, j, k) for j in range(len(Fn))]
    n_prec = hits = 0
    covered, recalled = [False] * len(Rn), [False] * len(Rn)
    for j in range(len(Fn)):
        inside = False
        for i in range(len(Rn)):
            s = _dot(Fn[j], Rn[i])
            if s >= t_R[i]:
                hits += 1
                inside = covered[i] = True
            if s >= t_F[j]:
                recalled[i] = True
        n_prec += inside
    return {'fakes_in_real_balls': n_prec, 'hits': hits, 'reals_with_a_fake': sum(covered), 'reals_in_fake_balls': sum(recalled)}


@pytest.mark.parametrize('shape', [(7, 6, 3, 2), (9, 11, 4, 3), (5, 5, 2, 4)])
def test_yardstick_equals_brute_force(shape):
    n_r, n_f, d, k = shape
    r = np.random.RandomState(0)
    real, fake = r.randn(n_r, d), 0.5 * r.randn(n_f, d) + 0.3
    ref, brute = R.prdc_ref64(real, fake, k), _brute(real, fake, k)
    for name, v in brute.items():
        assert ref[name] == v, name
    assert ref['precision'] == brute['fakes_in_real_balls'] / n_f and ref['coverage'] == brute['reals_with_a_fake'] / n_r
    assert ref['recall'] == brute['reals_in_fake_balls'] / n_r and ref['density'] == brute['hits'] / (k * n_f)
    assert ref['lo'] == ref['hi'] == brute and all(w == 0 for w in ref['width'].values())      # gap 0: everything decided


def test_exact_kernels_on_a_given_S_equal_the_float64_path():
    """float32 S made from float64 features: the exact path on it and the float64 path agree where every indicator is
    decided (a wide margin here), so the two halves of the yardstick state one thing."""
    real, fake = R.manifold_sets(0, 24, 40, 30)
    Rn, Fn = R.normalize64(real), R.normalize64(fake)
    ref = R.prdc_ref64(real, fake, 3, gap=1e-6)
    assert ref['lo'] == ref['hi']
    got = R.prdc_from_S((Rn @ Rn.T).astype(np.float32), (Fn @ Fn.T).astype(np.float32), (Fn @ Rn.T).astype(np.float32), 3)
    for name in ref['lo']:
        assert got[name] == ref[name], name


def test_the_tie_is_inclusive():
    S = np.array([[1.0, 0.5, 0.5, 0.25], [0.5, 0.5, 0.5, 0.5]], np.float32)
    assert R.kth_exact(S, 2).tolist() == [0.5, 0.5] and R.kth_exact(S, 3).tolist() == [0.5, 0.5]
    assert R.kth_exact(S, 2, 0).tolist() == [0.5, 0.5]                 # row 0 without column 0: 0.5 0.5 0.25
    assert R.kth_exact(S, 3, 0).tolist() == [0.25, 0.5]
    row_hits, col_c, col_r = R.count_exact(S, thr_row=[0.5, 0.75], thr_col=[1.0, 0.5, 0.75, 0.25])
    assert row_hits.tolist() == [3, 2] and col_c.tolist() == [1, 2, 0, 2] and col_r.tolist() == [1, 1, 1, 0]
    # two copies of one point set: every fake sits on a real, its similarity 1 >= any threshold
    X = np.eye(4, 5)
    ref = R.prdc_ref64(X, X, 2)
    assert ref['precision'] == ref['recall'] == ref['coverage'] == 1.0


def test_nan_and_signed_zero_rules():
    S = np.array([[-0.0, 0.0, np.nan, -1.0]], np.float32)
    bits = lambda k, self0=-1: int(R.kth_exact(S, k, self0).view(np.uint32)[0])
    assert bits(1) == 0x80000000 and bits(2) == 0x00000000               # zeros by column whatever their sign: the very floats
    assert bits(3) == 0xbf800000 and bits(4) == 0x7fc00000              # NaN ranks below every number
    assert bits(1, 0) == 0x00000000 and bits(3, 0) == 0x7fc00000        # column 0 left out by index
    # exclusion is by index, not by value: the largest value elsewhere stays in
    T = np.array([[5.0, np.inf, 1.0], [3.0, 7.0, np.inf]], np.float32)
    assert R.kth_exact(T, 1, 0).tolist() == [np.inf, np.inf] and R.kth_exact(T, 1, 1).tolist() == [5.0, 7.0]
    # a NaN on either side of a comparison is no hit
    row_hits, col_c, col_r = R.count_exact(np.array([[np.nan, 1.0, 1.0]], np.float32), thr_row=[np.nan], thr_col=[0.0, np.nan, 1.0])
    assert row_hits.tolist() == [1] and col_c.tolist() == [0, 0, 1] and col_r.tolist() == [0, 0, 0]
    assert R.count_exact(S, thr_col=[0.0, -0.0, 0.0, 0.0])[1].tolist() == [1, 1, 0, 0]          # -0.0 >= +0.0


def test_intervals_count_undecided_indicators_for_the_upper_end_only():
    real, fake = R.manifold_sets(1, 24, 60, 50)
    ref = R.prdc_ref64(real, fake, 5, gap=0.05)
    for name in ref['lo']:
        assert ref['lo'][name] <= ref[name] <= ref['hi'][name]
    assert ref['hi']['hits'] > ref['lo']['hits'] and ref['width']['density'] > 0


def test_python_layer_argument_errors():
    from contrad_amd import ops, prdc
    S = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.prdc_kth(S, 8, 1)                                           # host S
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.prdc_count(S, 8, thr_col=torch.zeros(8), col_hits_c=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='CUDA float32'):
        prdc.prdc(torch.zeros(8, 4), torch.zeros(8, 4))
    for k, n_r, n_f in ((0, 10, 10), (5, 5, 10), (5, 10, 5), (9, 10, 9)):
        with pytest.raises(ValueError, match='prdc: k'):
            prdc.check_k(k, n_r, n_f)
    prdc.check_k(5, 6, 6)
    P = prdc.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--gen', 'run/gen.pt'])
    assert (P.k, P.n_real, P.n_fake, P.batch_size, P.seed, P.gen_arch, P.fake) == (5, None, None, 500, None, None, None)
    with pytest.raises(SystemExit):
        prdc.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz'])                        # neither --fake nor --gen
    with pytest.raises(SystemExit):
        prdc.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--fake', 'a.npz', '--gen', 'g.pt'])
    from contrad_amd import train_gan, train_stylegan2
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'])
        assert not [name for name in vars(Q) if name.startswith('prdc')]          # a flag not given leaves no attribute
        H = prdc.check_hook_arguments(Q)                                # off by default
        assert (H.prdc_data, H.prdc_encoder, H.prdc_encoder_arch, H.prdc_k, H.prdc_n, H.prdc_best) == (None, None, None, 5, 10000, None)
        Q = mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_data', 'c10.npz', '--prdc_encoder', 'e.pt', '--prdc_encoder_arch',
                            'snresnet18', '--prdc_k', '3', '--prdc_n', '500', '--prdc_best', 'recall'])
        H = prdc.check_hook_arguments(Q)
        assert (H.prdc_data, H.prdc_encoder, H.prdc_encoder_arch, H.prdc_k, H.prdc_n, H.prdc_best) == ('c10.npz', 'e.pt', 'snresnet18', 3, 500, 'recall')
        for stray in (['--prdc_encoder', 'e.pt'], ['--prdc_encoder_arch', 'sndcgan'], ['--prdc_k', '3'], ['--prdc_n', '500'],
                      ['--prdc_best', 'recall'], ['--prdc_k', '5', '--prdc_n', '10000']):        # (given, even at the default)
            with pytest.raises(ValueError, match='%s.* nothing without --prdc_data' % stray[0]):
                prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + stray))
        Q = mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_data', 'c10.npz'])
        with pytest.raises(ValueError, match='frozen encoder'):
            prdc.check_hook_arguments(Q)
        with pytest.raises(SystemExit):
            mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_best', 'fid'])


def test_best_value_of_a_resumed_run_comes_from_rows_up_to_its_checkpoint(tmp_path):
    from contrad_amd import features, prdc
    path = str(tmp_path / 'prdc_7.csv')
    rows = [(2, dict(precision=0.5, recall=0.25, density=0.75, coverage=0.125)),
            (4, dict(precision=0.25, recall=0.5, density=1.5, coverage=0.25)),
            (6, dict(precision=0.75, recall=0.125, density=0.5, coverage=0.5))]        # step 6: written, its networks never saved
    with open(path, 'w') as f:
        f.write(prdc.CSV_HEAD + '\n' + ''.join(prdc.csv_line(s, o) + '\n' for s, o in rows))
    assert prdc.best_in_csv(path, 'coverage', 6) == 0.5 and prdc.best_in_csv(path, 'coverage', 4) == 0.25
    assert prdc.best_in_csv(path, 'coverage', 5) == 0.25 and prdc.best_in_csv(path, 'precision', 4) == 0.5
    assert prdc.best_in_csv(path, 'density', 4) == 1.5 and prdc.best_in_csv(path, 'recall', 2) == 0.25
    assert prdc.best_in_csv(path, 'coverage', 1) is None and prdc.best_in_csv(path, 'coverage', 0) is None
    for upto in range(8):                                              # the one reader under both wrappers: column 1 + index, max
        for j, metric in enumerate(prdc.METRICS):
            assert features.best_in_csv(path, 1 + j, upto, max) == prdc.best_in_csv(path, metric, upto)
    assert features.best_in_csv(path, 3, 6, min) == 0.5                # (density: 0.75, 1.5, 0.5)
    with open(path, 'w') as f:
        f.write(prdc.CSV_HEAD + '\n')
    assert prdc.best_in_csv(path, 'coverage', 100) is None


def test_command_line_refuses_bad_sets_on_the_host(tmp_path):
    from contrad_amd import features
    r = np.random.RandomState(0)
    np.savez(str(tmp_path / 'real.npz'), x_train=r.randint(0, 255, (8, 32, 32, 3)).astype(np.uint8))
    np.savez(str(tmp_path / 'small.npz'), images=r.randint(0, 255, (8, 16, 16, 3)).astype(np.uint8))
    np.savez(str(tmp_path / 'empty.npz'), images=np.zeros((0, 32, 32, 3), np.uint8))
    np.savez(str(tmp_path / 'floats.npz'), images=np.zeros((8, 32, 32, 3), np.float32))
    assert features.load_images(str(tmp_path / 'real.npz'), 'x_train', 5).shape == (5, 32, 32, 3)
    with pytest.raises(ValueError, match='empty'):
        features.load_images(str(tmp_path / 'empty.npz'), 'images')
    with pytest.raises(ValueError, match='uint8'):
        features.load_images(str(tmp_path / 'floats.npz'), 'images')
    with pytest.raises(ValueError, match='holds no'):
        features.load_images(str(tmp_path / 'real.npz'), 'images')


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def _ip(a):
    return ctypes.cast(a, ctypes.POINTER(ctypes.c_int)) if a is not None else ctypes.POINTER(ctypes.c_int)()


def test_kth_entry_point_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    f = lib().raw('contrad_prdc_kth')
    M, n = 2, 8
    S, thr = (ctypes.c_float * (M * n))(), (ctypes.c_float * M)()

    def call(S=S, ldS=n, M=M, n=n, k=3, self0=0, thr=thr):
        return f(_vp(S), ctypes.c_longlong(ldS), M, n, k, ctypes.c_longlong(self0), _vp(thr), ctypes.c_void_p(0))

    for bad in (dict(S=None), dict(thr=None), dict(M=0), dict(n=0), dict(k=0), dict(k=n), dict(k=n + 1, self0=-1),
                dict(k=n, self0=n - 1), dict(ldS=n - 1)):
        assert call(**bad) == -22, bad
    assert all(v == 0 for v in thr)


def test_count_entry_point_rejects_bad_arguments_before_any_gpu_call():
    from contrad_amd._lib import lib
    f = lib().raw('contrad_prdc_count')
    M, n = 2, 8
    S, tr, tc = (ctypes.c_float * (M * n))(), (ctypes.c_float * M)(), (ctypes.c_float * n)()
    rh, cc, cr = (ctypes.c_int * M)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()

    def call(S=S, ldS=n, M=M, n=n, tr=tr, tc=tc, rh=rh, cc=cc, cr=cr):
        return f(_vp(S), ctypes.c_longlong(ldS), M, n, _vp(tr), _vp(tc), _ip(rh), _ip(cc), _ip(cr), ctypes.c_void_p(0))

    for bad in (dict(S=None), dict(tr=None, tc=None), dict(rh=None), dict(cc=None), dict(cr=None), dict(tr=None, rh=None),
                dict(tc=None, cr=None), dict(M=0), dict(n=0), dict(ldS=n - 1)):
        assert call(**bad) == -22, bad
    assert all(v == 0 for v in rh) and all(v == 0 for v in cc) and all(v == 0 for v in cr)
