"""The float64 yardstick of the kernel distance (tests/kid_ref64.py) against a brute-force double loop, the rule that self
pairs are left out by index, the subset draw, the argument errors of the Python layer and of the two C entry points
(raised before any GPU call), ``kid.best_in_csv`` and the refusals of the hook flags."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import kid_ref64 as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(rows):
    return [[x / max(sum(v * v for v in r) ** 0.5, 1e-12) for x in r] for r in rows]


def _k(a, b, gamma, coef0):
    return (gamma * sum(x * y for x, y in zip(a, b)) + coef0) ** 3


def _brute(real, fake, idx_r, idx_f, gamma=1.0, coef0=1.0):
    """MMD2 of every subset by double loops over plain Python floats."""
    Rn, Fn = _unit(real.tolist()), _unit(fake.tolist())
    out = []
    for ir, jf in zip(idx_r.tolist(), idx_f.tolist()):
        m = len(ir)
        A = sum(_k(Rn[ir[i]], Rn[ir[j]], gamma, coef0) for i in range(m) for j in range(m) if i != j)
        B = sum(_k(Fn[jf[i]], Fn[jf[j]], gamma, coef0) for i in range(m) for j in range(m) if i != j)
        C = sum(_k(Fn[jf[i]], Rn[ir[j]], gamma, coef0) for i in range(m) for j in range(m))
        out.append(((A + B) / (m * (m - 1)) - 2 * C / m ** 2, A, B, C))
    return out


@pytest.mark.parametrize('shape', [(7, 6, 3, 4, 3, 1.0, 1.0), (9, 11, 4, 5, 2, 1.0, 1.0), (5, 5, 2, 5, 1, 0.5, 2.0)])
def test_yardstick_equals_brute_force(shape):
    from contrad_amd import kid
    n_r, n_f, d, size, n_subsets, gamma, coef0 = shape
    r = np.random.RandomState(0)
    real, fake = r.randn(n_r, d), 0.5 * r.randn(n_f, d) + 0.3
    ref = K.kid_ref64(real, fake, n_subsets, size, seed=3, gamma=gamma, coef0=coef0)
    m = min(size, n_r, n_f)
    idx_r, idx_f = kid.subset_indices(n_r, n_f, m, n_subsets, 3)
    brute = _brute(real, fake, idx_r, idx_f, gamma, coef0)
    assert ref['subset_size'] == m and len(ref['sums']) == n_subsets
    for t, (mmd2, A, B, C) in enumerate(brute):
        for got, want in zip(ref['sums'][t], (A, B, C)):
            assert abs(got - want) <= 1e-12 * abs(want), (t, got, want)
        assert abs(K.mmd2_of(ref['sums'], m)[t] - mmd2) <= 1e-12
    mean = sum(b[0] for b in brute) / n_subsets
    assert abs(ref['kid'] - mean) <= 1e-12
    assert abs(ref['kid_std'] - (sum((b[0] - mean) ** 2 for b in brute) / n_subsets) ** 0.5) <= 1e-12       # ddof 0
    if n_subsets == 1:
        assert ref['kid_std'] == 0.0
    assert np.array_equal(kid.mmd2_of(ref['sums'], m), K.mmd2_of(ref['sums'], m))                            # the shipped host formula


def test_self_pairs_are_left_out_by_index_not_by_value():
    """Two equal rows inside a subset: their pair has similarity 1 like a self pair, and counts (both ways)."""
    X = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    S = (X @ X.T).astype(np.float32)
    # off-diagonal: (0,1) and (1,0) hold 1 -> (1 + 1)^3 = 8 each; the four others hold 0 -> 1 each
    assert K.block_sum(S, 0) == 2 * 8.0 + 4 * 1.0
    assert K.block_sum(S, -1) == 2 * 8.0 + 4 * 1.0 + 3 * 8.0           # nothing left out: the diagonal too
    assert K.block_sum(S[1:], 1) == 8.0 + 1.0 + 1.0 + 1.0              # a row chunk that starts at row 1
    assert K.block_sum(S, 5) == K.block_sum(S, -1)                     # an excluded column past n leaves nothing out
    T = S.copy()
    T[0, 0] = np.nan
    T[1, 1] = 1e30
    assert K.block_sum(T, 0) == K.block_sum(S, 0) and math.isfinite(K.block_bound(T, 0))      # never seen
    assert math.isnan(K.block_sum(T, -1))
    assert K.block_sum(np.zeros((1, 1), np.float32), 0) == 0.0 and K.block_bound(np.zeros((1, 1), np.float32), 0) == 0.0
    # a set against itself: the unbiased estimate is exactly 0 when both index sets are the same rows
    ref = K.subset_sums64(K.normalize64(X), K.normalize64(X), np.arange(3), np.arange(3))
    assert K.mmd2_of([ref], 3)[0] == (ref[0] + ref[1]) / 6 - 2 * ref[2] / 9 and ref[0] == ref[1]


def test_bound_is_far_below_one_dropped_element():
    r = np.random.RandomState(1)
    S = np.clip(r.randn(300, 300), -1, 1).astype(np.float32)
    x = (1.0 * S.astype(np.float64) + 1.0) ** 3
    assert K.block_bound(S, 0) < 1e-3 * np.median(x)                   # (a typical term is about 1)


def test_subset_indices():
    from contrad_amd import kid
    a_r, a_f = kid.subset_indices(50, 40, 30, 6, 7)
    assert a_r.shape == a_f.shape == (6, 30) and a_r.dtype == a_f.dtype == np.int64
    for t in range(6):
        assert len(set(a_r[t].tolist())) == 30 and 0 <= a_r[t].min() and a_r[t].max() < 50
        assert len(set(a_f[t].tolist())) == 30 and 0 <= a_f[t].min() and a_f[t].max() < 40
    b_r, b_f = kid.subset_indices(50, 40, 30, 6, 7)
    assert np.array_equal(a_r, b_r) and np.array_equal(a_f, b_f)       # the same seed: the same draw
    c_r, c_f = kid.subset_indices(50, 40, 30, 6, 8)
    assert not np.array_equal(a_r, c_r) and not np.array_equal(a_f, c_f)
    rng = np.random.default_rng(7)                                     # the stated order of the draws
    for t in range(6):
        assert np.array_equal(a_r[t], rng.choice(50, 30, replace=False))
        assert np.array_equal(a_f[t], rng.choice(40, 30, replace=False))
    full_r, full_f = kid.subset_indices(5, 9, 5, 2, 0)                 # m = n: a permutation of the whole set
    assert sorted(full_r[1].tolist()) == list(range(5))


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def test_entry_points_reject_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    query, f = lib().raw('contrad_kid_sums_workspace_bytes'), lib().raw('contrad_kid_sums')
    assert query(0, 8) == -22 and query(8, 0) == -22 and query(-1, -1) == -22
    assert query(1, 1) == 8 and query(1000, 1000) > 0 and query(1000, 1000) % 8 == 0
    M, n = 2, 8
    need = query(M, n)
    S, out, ws = (ctypes.c_float * (M * n))(), (ctypes.c_double * 1)(-7.0), (ctypes.c_double * (need // 8 + 1))()

    def call(S=S, ldS=n, M=M, n=n, self0=0, gamma=1.0, coef0=1.0, accumulate=0, out=out, ws=ws, ws_bytes=need):
        return f(_vp(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), gamma, coef0, accumulate, _vp(out), _vp(ws),
                 ctypes.c_longlong(ws_bytes), ctypes.c_void_p(0))

    for bad in (dict(S=None), dict(out=None), dict(M=0), dict(n=0), dict(M=-1), dict(ldS=n - 1), dict(gamma=float('nan')),
                dict(gamma=float('inf')), dict(coef0=float('nan')), dict(coef0=-float('inf')), dict(ws=None), dict(ws_bytes=need - 1),
                dict(ws_bytes=0), dict(accumulate=1, out=None)):
        assert call(**bad) == -22, bad
    assert out[0] == -7.0 and all(v == 0.0 for v in ws)


def test_python_layer_refusals():
    from contrad_amd import kid, ops
    S = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.kid_sums(S, 8)                                             # host S
    for bad in (dict(n_subsets=0), dict(subset_size=1), dict(n_real=1), dict(n_fake=1), dict(n_real=0), dict(n_fake=0)):
        a = dict(n_real=10, n_fake=10, n_subsets=100, subset_size=1000); a.update(bad)
        with pytest.raises(ValueError, match='kid: '):
            kid.check_sizes(**a)
    assert kid.check_sizes(10, 7) == 7 and kid.check_sizes(3000, 2000) == 1000 and kid.check_sizes(2, 2, 1, 2) == 2
    # ``kid`` refuses on the host, before any GPU work: host tensors get as far as the sizes
    f = torch.zeros(8, 4)
    for bad in (dict(n_subsets=0), dict(subset_size=1)):
        with pytest.raises(ValueError, match='kid: '):
            kid.kid(f, f, **bad)
    with pytest.raises(ValueError, match='two rows'):
        kid.kid(f[:1], f)
    with pytest.raises(ValueError, match='empty'):
        kid.kid(f, f[:0])
    with pytest.raises(ValueError, match='finite'):
        kid.kid(f, f, gamma=float('nan'))
    with pytest.raises(RuntimeError, match='CUDA float32'):
        kid.kid(f, f)                                                  # ... and no further
    with pytest.raises(RuntimeError, match='CUDA float32'):
        kid.kid(f.double(), f)
    P = kid.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--gen', 'run/gen.pt'])
    assert (P.n_subsets, P.subset_size, P.n_real, P.n_fake, P.batch_size, P.seed, P.gen_arch, P.fake) == \
        (100, 1000, None, None, 500, None, None, None)
    with pytest.raises(SystemExit):
        kid.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz'])                         # neither --fake nor --gen
    with pytest.raises(SystemExit):
        kid.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--fake', 'a.npz', '--gen', 'g.pt'])


def test_best_in_csv_is_the_minimum_up_to_the_checkpoint(tmp_path):
    from contrad_amd import features, kid
    path = str(tmp_path / 'kid_7.csv')
    rows = [(2, dict(kid=0.5, kid_std=0.01)), (4, dict(kid=0.25, kid_std=0.02)), (6, dict(kid=-0.000125, kid_std=0.03)),
            (8, dict(kid=0.75, kid_std=0.04))]                         # step 8: written, its networks never saved
    with open(path, 'w') as f:
        f.write(kid.CSV_HEAD + '\n' + ''.join(kid.csv_line(s, o) + '\n' for s, o in rows))
    with open(path) as f:
        assert f.read().split() == ['step,kid,kid_std', '2,0.500000,0.010000', '4,0.250000,0.020000', '6,-0.000125,0.030000',
                                    '8,0.750000,0.040000']
    assert kid.best_in_csv(path, 8) == -0.000125 and kid.best_in_csv(path, 6) == -0.000125      # not clamped
    assert kid.best_in_csv(path, 5) == 0.25 and kid.best_in_csv(path, 4) == 0.25 and kid.best_in_csv(path, 2) == 0.5
    assert kid.best_in_csv(path, 1) is None and kid.best_in_csv(path, 0) is None
    for upto in range(10):                                             # the one reader under both wrappers: column 1, min
        assert features.best_in_csv(path, 1, upto, min) == kid.best_in_csv(path, upto)
    assert features.best_in_csv(path, 1, 8, max) == 0.75 and features.best_in_csv(path, 2, 6, max) == 0.03
    with open(path, 'w') as f:
        f.write(kid.CSV_HEAD + '\n')
    assert kid.best_in_csv(path, 100) is None


def test_hook_flags_parse_and_are_refused_before_any_cuda_call(tmp_path):
    from contrad_amd import prdc, train_gan, train_stylegan2
    was_initialised = torch.cuda.is_initialized()
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'])
        assert not hasattr(Q, 'prdc_kid') and prdc.check_hook_arguments(Q).prdc_kid is False       # off, and no attribute
        on = ['--prdc_data', 'c10.npz', '--prdc_encoder', 'e.pt']
        H = prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid']))
        assert H.prdc_kid is True and H.prdc_best is None
        H = prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid', '--prdc_best', 'kid']))
        assert H.prdc_kid is True and H.prdc_best == 'kid'
        assert prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_kid', '--prdc_best', 'recall'])).prdc_best == 'recall'
        with pytest.raises(ValueError, match='--prdc_kid.* nothing without --prdc_data'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_kid']))
        with pytest.raises(ValueError, match='--prdc_best kid needs --prdc_kid'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_best', 'kid']))
    # through the script: the refusal comes before the first CUDA call and before the log directory is made
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    common = [gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', str(tmp_path / 'run')]
    with pytest.raises(ValueError, match='nothing without --prdc_data'):
        train_gan.main(common + ['--prdc_kid'])
    with pytest.raises(ValueError, match='--prdc_best kid needs --prdc_kid'):
        train_gan.main(common + ['--prdc_data', str(tmp_path / 'real.npz'), '--prdc_encoder', str(tmp_path / 'e.pt'), '--prdc_best', 'kid'])
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(str(tmp_path / 'run'))
    assert prdc.METRICS == ('precision', 'recall', 'density', 'coverage') and prdc.CSV_HEAD == 'step,precision,recall,density,coverage'


def test_the_evaluators_are_layered_on_features_not_on_each_other():
    """kid.py stands on features.py alone (no import of prdc, no toolkit name reached through it); prdc.py imports kid at the
    top of the file, not inside a function; the toolkit has one home (no copies or re-exports left in the old ones)."""
    import ast
    import inspect
    from contrad_amd import features, kid, knn, prdc
    toolkit = ('normalize_rows', 'new_bank', 'bank_of', 'S_CHUNK_FLOATS', 'MAX_CHUNK_ROWS', 'chunk_rows_of', 'similarities',
               'similarity_chunks', 'check_u8', 'to_float_nchw', 'extract_features', 'load_frozen', 'load_images', 'sample_u8')
    kid_src, prdc_src = inspect.getsource(kid), inspect.getsource(prdc)
    assert 'from . import prdc' not in kid_src and 'from .prdc' not in kid_src and 'import prdc' not in kid_src
    assert 'prdc.' not in kid_src.replace('contrad_amd/prdc.py', '').replace('``prdc.PRDCMonitor``', '')
    imports = [n for n in ast.walk(ast.parse(kid_src)) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert all('prdc' not in (getattr(n, 'module', None) or '') and all('prdc' not in a.name for a in n.names) for n in imports)
    tree = ast.parse(prdc_src)
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert any(isinstance(n, ast.ImportFrom) and n.level == 1 and not n.module and any(a.name == 'kid' for a in n.names) for n in top)
    nested = [n for f in ast.walk(tree) if isinstance(f, (ast.FunctionDef, ast.Lambda)) for n in ast.walk(f)
              if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not nested, [ast.dump(n) for n in nested]
    for name in toolkit:
        assert hasattr(features, name), name
        for old_home in (knn, prdc, kid):
            assert not hasattr(old_home, name), (old_home.__name__, name)
