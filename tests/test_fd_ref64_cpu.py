"""The yardstick of the Frechet distance (tests/fd_ref64.py) against three independent statements of it, the conditions of
the GPU cases that need no GPU, every host refusal of contrad_amd/fd.py and of the ``--prdc_fd`` flags (raised with
``torch.cuda.is_initialized()`` unchanged) and the ``-EINVAL`` cases of ``contrad_dot_sums`` on host pointers."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fd_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fd.npz')
FULL_RANK = [(40, 33, 12), (33, 40, 12), (120, 90, 7), (9, 11, 3)]         # (n_r, n_f, d), n > d


def _full_rank_sets(shape, seed=0):
    n_r, n_f, d = shape
    r = np.random.RandomState(seed)
    return (np.maximum(r.randn(n_r, d) + 0.3, 0.0) + 0.01 * r.rand(n_r, d), np.maximum(r.randn(n_f, d) * 0.7 + 0.6, 0.0) + 0.01 * r.rand(n_f, d))


# ---- (a) the textbook form ----
@pytest.mark.parametrize('shape', FULL_RANK, ids=lambda s: 'x'.join(map(str, s)))
def test_yardstick_equals_the_textbook_eigenvalue_form(shape):
    real, fake = _full_rank_sets(shape)
    ref = R.fd_ref64(real, fake, normalize=False)
    (mu_r, S_r), (mu_f, S_f) = R.moments(real), R.moments(fake)
    assert abs(ref['trace_real'] - np.trace(S_r)) <= 1e-12 and abs(ref['trace_fake'] - np.trace(S_f)) <= 1e-12
    assert abs(ref['mean_term'] - ((mu_r - mu_f) ** 2).sum()) <= 1e-14
    assert abs(ref['fd'] - R.textbook(real, fake)) <= 1e-10, (ref['fd'], R.textbook(real, fake))
    assert ref['fd'] > 0.01                                            # two different sets
    same = R.fd_ref64(real, real.copy(), normalize=False)
    assert abs(same['fd']) <= 1e-12 and same['mean_term'] == 0.0         # equal sets: all cancellation
    # ddof 0 in place of 1 is visible at the tolerance of every test here
    assert abs(ref['trace_real'] - np.trace(np.cov(real, rowvar=False, ddof=0))) >= 1e-3 * ref['trace_real'] / 2


# ---- (b) scipy's matrix square root, as the reference writes it ----
@pytest.mark.parametrize('shape', FULL_RANK, ids=lambda s: 'x'.join(map(str, s)))
def test_yardstick_equals_scipy_sqrtm(shape):
    linalg = pytest.importorskip('scipy').linalg
    real, fake = _full_rank_sets(shape, 1)
    (mu_r, S_r), (mu_f, S_f) = R.moments(real), R.moments(fake)
    covmean = linalg.sqrtm(S_r.dot(S_f))
    value = (mu_r - mu_f).dot(mu_r - mu_f) + np.trace(S_r) + np.trace(S_f) - 2.0 * np.trace(np.real(covmean))
    assert abs(R.fd_ref64(real, fake, normalize=False)['fd'] - value) <= 1e-8, value


# ---- (c) the value the reference's function returned ----
def test_yardstick_equals_the_recorded_reference_values():
    with np.load(GOLDEN) as z:
        values = z['fd']
        assert len(values) >= 3
        for i, v in enumerate(values):
            real, fake = z['real_%d' % i], z['fake_%d' % i]
            assert real.dtype == np.float64 and real.shape[0] > real.shape[1]
            got = R.fd_ref64(real, fake, normalize=False)['fd']
            assert abs(got - v) <= 1e-8, (i, got, v)


# ---- (d) the conditions of the GPU cases ----
@pytest.mark.parametrize('case', R.FEATURE_CASES, ids=lambda c: 'd%d-%dx%d-%s' % c)
def test_conditions_of_the_gpu_cases(case):
    real, fake = R.sets(case)
    ref = R.fd_ref64(real, fake)
    emu = R.emulate_fp32(R.normalize64(real).astype(np.float32), R.normalize64(fake).astype(np.float32), 60)
    err = abs(emu['fd'] - ref['fd']) / ref['scale']
    est = np.asarray(emu['estimates'])
    print('fd conditions d%d %dx%d %s: float64 fd %.9g  s %.6g  fd / s %.3g  |emulation - float64| / s %.3g  largest fall %.3g of the '
          'estimate' % (case + (ref['fd'], ref['scale'], ref['fd'] / ref['scale'], err, max(0.0, -np.diff(est).min()) / est[-1])))
    assert err <= R.TOL_CAP
    if case[3] == 'equal':
        assert abs(ref['fd']) <= 1e-12 * ref['scale']
    else:
        assert ref['fd'] >= R.MIN_FD * ref['scale']
    assert np.diff(est).min() >= -1e-6 * est[-1]


def test_emulation_converges_from_below_on_a_rank_deficient_case():
    real, fake = R.sets((24, 300, 257, 'moved'))
    Rn, Fn = R.normalize64(real), R.normalize64(fake)
    ref = R.fd_ref64(Rn, Fn, normalize=False)
    e10, e60 = (R.emulate_fp32(Rn.astype(np.float32), Fn.astype(np.float32), k) for k in (10, 60))
    assert e10['cross_term'] < e60['cross_term'] <= ref['cross_term'] * (1 + 1e-6)
    assert abs(e60['cross_term'] - ref['cross_term']) < abs(e10['cross_term'] - ref['cross_term'])


# ---- (e) host refusals ----
def test_fd_refuses_on_the_host_before_any_gpu_work():
    from contrad_amd import fd
    was_initialised = torch.cuda.is_initialized()
    f = torch.zeros(8, 4)
    for bad in (dict(n_real=1), dict(n_fake=1), dict(n_real=0), dict(n_iter=0), dict(n_iter=-3),
                dict(n_real=50000, n_fake=50000), dict(n_real=1 << 29, n_fake=4), dict(n_real=3, n_fake=(1 << 29) + 1),
                dict(n_real=5000, n_fake=6000, dim=1 << 19)):              # (the last: the bank [dim][round_up(q, 4)])
        a = dict(n_real=10, n_fake=10, n_iter=60); a.update(bad)
        with pytest.raises(ValueError, match='fd: '):
            fd.check_sizes(**a)
    assert fd.check_sizes(10, 7) == (10, 7) and fd.check_sizes(2, 2, 1) == (2, 2) and fd.check_sizes(10000, 50000, 60, 8192) == (50000, 10000)
    assert fd.check_sizes((1 << 29) - 1, 4) == ((1 << 29) - 1, 4)          # the limit itself: p * round_up(q, 4) < 2^31
    with pytest.raises(ValueError, match='two rows'):
        fd.fd(f[:1], f)
    with pytest.raises(ValueError, match='two rows'):
        fd.fd(f, f[:1])
    with pytest.raises(ValueError, match='n_iter'):
        fd.fd(f, f, n_iter=0)
    with pytest.raises(RuntimeError, match='width'):
        fd.fd(f, torch.zeros(8, 5))
    with pytest.raises(ValueError, match='2\\^31'):
        fd.fd(torch.empty(50000, 1), torch.empty(50000, 1))
    with pytest.raises(RuntimeError, match='CUDA float32'):
        fd.fd(f, f)                                                    # host tensors get as far as the sizes, and no further
    with pytest.raises(RuntimeError, match='CUDA float32'):
        fd.fd(f.double(), f)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        fd.fd(None, f)
    with pytest.raises(ValueError, match='two rows'):
        fd.real_state_of(torch.zeros(4, 4), 1)
    with pytest.raises(RuntimeError, match='real bank'):
        fd.real_state_of(torch.zeros(4, 7), 7)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        fd.real_state_of(torch.zeros(4, 8), 7)
    u8 = torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA uint8'):
        fd.fd_of(None, u8, u8)                                         # like kid_of: device-resident sets only
    assert torch.cuda.is_initialized() == was_initialised


def test_result_is_combined_on_the_host_in_float64():
    from contrad_amd import fd
    est = [1.0, 2.0, 2.5, 2.75, 2.875, 2.9375, 2.96875]
    out = fd.combine(est, 30.0, 8.0, 0.25, 11, 5, 16)
    assert out['trace_real'] == 3.0 and out['trace_fake'] == 2.0 and out['cross_term'] == est[-1] / math.sqrt(40.0)
    assert out['fd'] == 0.25 + 3.0 + 2.0 - 2.0 * out['cross_term'] and out['tail'] == est[-1] - est[-6]
    assert (out['n_iter'], out['n_real'], out['n_fake'], out['dim'], out['estimates']) == (7, 11, 5, 16, est)
    assert fd.combine(est[:5], 30.0, 8.0, 0.25, 11, 5, 16)['tail'] == 0.0
    assert 'never with Inception-based FID' in out['note'] and 'NEVER with the Inception-based FID' in ' '.join(fd.__doc__.split())
    assert 'WARNING' not in fd.line_of(dict(out, tail=1e-7 * est[-1])) and 'WARNING' in fd.line_of(dict(out, tail=-2e-6 * est[-1]))
    assert 'not an Inception FID' in fd.line_of(out)
    row = dict(fd=0.5, fd_mean_term=0.25, fd_trace_fake=2.0, fd_cross_term=1.5, fd_tail=-1.25e-9)
    assert fd.csv_line(4, row) == '4,0.500000,0.250000,2.000000,1.500000,-1.250e-09'
    assert fd.CSV_HEAD == 'step,fd,mean_term,trace_fake,cross_term,tail'


def test_command_line_parses_and_refuses_before_any_gpu_work(tmp_path, capsys):
    from contrad_amd import fd
    was_initialised = torch.cuda.is_initialized()
    P = fd.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--gen', 'run/gen.pt'])
    assert (P.n_iter, P.n_real, P.n_fake, P.batch_size, P.seed, P.gen_arch, P.fake) == (60, None, None, 500, None, None, None)
    assert fd.parse_args(['e.pt', 'sndcgan', '--real', 'c.npz', '--fake', 'a.npz', '--n_iter', '30']).n_iter == 30
    with pytest.raises(SystemExit):
        fd.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz'])                          # neither --fake nor --gen
    with pytest.raises(SystemExit):
        fd.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'c10.npz', '--fake', 'a.npz', '--gen', 'g.pt'])
    with pytest.raises(ValueError, match='--n_iter'):
        fd.main(['e.pt', 'sndcgan', '--real', str(tmp_path / 'c.npz'), '--fake', str(tmp_path / 'a.npz'), '--n_iter', '0'])
    with pytest.raises(SystemExit):
        fd.parse_args(['--help'])
    assert 'never with Inception-based FID' in ' '.join(capsys.readouterr().out.split())
    import test_fd
    assert test_fd.main is fd.main and 'never with the Inception-based FID' in ' '.join(test_fd.__doc__.split())
    assert torch.cuda.is_initialized() == was_initialised


def test_hook_flags_parse_and_are_refused_before_any_cuda_call(tmp_path):
    from contrad_amd import prdc, train_gan, train_stylegan2
    was_initialised = torch.cuda.is_initialized()
    on = ['--prdc_data', 'c10.npz', '--prdc_encoder', 'e.pt']
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'] + on)
        assert not hasattr(Q, 'prdc_fd') and not hasattr(Q, 'prdc_fd_iter')                     # off, and no attribute
        H = prdc.check_hook_arguments(Q)
        assert H.prdc_fd is False and H.prdc_fd_iter == 60
        H = prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_fd']))
        assert H.prdc_fd is True and H.prdc_fd_iter == 60 and H.prdc_best is None
        assert prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_fd', '--prdc_fd_iter', '30'])).prdc_fd_iter == 30
        with pytest.raises(ValueError, match='--prdc_fd does nothing without --prdc_data'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan', '--prdc_fd']))
        with pytest.raises(ValueError, match='--prdc_fd_iter needs --prdc_fd'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_fd_iter', '30']))
        with pytest.raises(ValueError, match='--prdc_fd_iter must be at least 1'):
            prdc.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_fd', '--prdc_fd_iter', '0']))
        with pytest.raises(SystemExit):                                                        # records only: no --prdc_best choice
            mod.parse_args(['cfg.gin', 'sndcgan'] + on + ['--prdc_fd', '--prdc_best', 'fd'])
    assert prdc.BEST_CHOICES == prdc.METRICS + ('kid',)
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    common = [gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', str(tmp_path / 'run')]
    with pytest.raises(ValueError, match='nothing without --prdc_data'):
        train_gan.main(common + ['--prdc_fd'])
    with pytest.raises(ValueError, match='--prdc_fd_iter needs --prdc_fd'):
        train_gan.main(common + ['--prdc_data', str(tmp_path / 'real.npz'), '--prdc_encoder', str(tmp_path / 'e.pt'), '--prdc_fd_iter', '9'])
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(str(tmp_path / 'run'))


# ---- (f) contrad_dot_sums on host pointers ----
def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def test_dot_sums_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    query, f, g = lib().raw('contrad_kid_sums_workspace_bytes'), lib().raw('contrad_dot_sums'), lib().raw('contrad_mmd_sums')
    M, n = 2, 8
    need = query(M, n)
    A, B, out, ws = (ctypes.c_float * (M * n))(), (ctypes.c_float * (M * n))(), (ctypes.c_double * 2)(-7.0, -7.0), (ctypes.c_double * (need // 8 + 1))()
    off4 = lambda buf: ctypes.c_void_p(ctypes.addressof(buf) + 4)

    def call(A=A, ldA=n, B=B, ldB=n, M=M, n=n, accumulate=0, out=out, ws=ws, ws_bytes=need):
        return f(_vp(A), ctypes.c_longlong(ldA), _vp(B), ctypes.c_longlong(ldB), M, n, accumulate, _vp(out), _vp(ws),
                 ctypes.c_longlong(ws_bytes), ctypes.c_void_p(0))

    for bad in (dict(A=None), dict(B=None), dict(out=None), dict(M=0), dict(M=-1), dict(n=0), dict(n=-2), dict(ldA=n - 1), dict(ldB=n - 1),
                dict(ldA=0), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=off4(ws)), dict(out=off4(out)),
                dict(accumulate=1, out=None), dict(A=None, B=None)):
        assert call(**bad) == -22, bad
    assert out[0] == -7.0 and out[1] == -7.0 and all(v == 0.0 for v in ws)
    # the two-operand kind is reachable through contrad_dot_sums only
    for kind in (2, 3, -1):
        assert g(_vp(A), ctypes.c_longlong(n), M, n, ctypes.c_longlong(-1), kind, 1.0, 1.0, 0, _vp(out), _vp(ws), ctypes.c_longlong(need),
                 ctypes.c_void_p(0)) == -22, kind


def test_dot_sums_wrapper_refusals():
    from contrad_amd import ops
    A = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.dot_sums(A, A, 8)                                          # host operands
    with pytest.raises(RuntimeError, match='two operands'):
        ops.dot_sums(A, None, 8)
    assert ops.MMD_KINDS == {'poly3': 0, 'rq': 1}                      # no name for the internal kind
