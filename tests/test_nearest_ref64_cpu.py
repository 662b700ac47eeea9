"""The float64 yardstick of the memorisation check (tests/nearest_ref64.py) against a brute-force loop, and everything of
contrad_amd/nearest.py, the leave-self-out entry point and the ``--prdc_auth`` flag that is refused on the host (raised
before any GPU call), the csv line and the flag's parsing in the three training scripts."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nearest_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _better(row, a, b):
    """Does column a come before column b in the neighbour order?"""
    va, vb = row[a], row[b]
    if np.isnan(va) or np.isnan(vb):
        if np.isnan(va) and np.isnan(vb):
            return a < b
        return np.isnan(vb)
    if va != vb:                      # -0.0 == +0.0 in this comparison, as the rule asks
        return va > vb
    return a < b


def _brute(S, k, self0):
    out = []
    for i in range(S.shape[0]):
        left = [j for j in range(S.shape[1]) if not (self0 >= 0 and j == self0 + i)]
        chosen = []
        for _ in range(k):
            best = left[0]
            for j in left[1:]:
                if _better(S[i], j, best):
                    best = j
            chosen.append(best)
            left.remove(best)
        out.append(chosen)
    return np.array(out)


@pytest.mark.parametrize('case', [(5, 5, 4, 0), (3, 8, 1, 0), (4, 9, 8, 7), (3, 9, 9, -1), (6, 12, 5, 6)], ids=lambda c: 'x'.join(map(str, c)))
def test_select_loo_equals_brute_force(case):
    M, n, k, self0 = case
    r = np.random.RandomState(1)
    S = r.randn(M, n).astype(np.float32)
    ties = (np.round(S * 2) / 2).astype(np.float32)
    special = ties.copy()
    special[:, ::3] = 0.0
    special[:, ::6] = -0.0
    for i in range(M):
        special[i, (5 * i + 1) % n] = np.nan
    own = S.copy()
    for i in range(M):
        if 0 <= self0 + i < n:
            own[i, self0 + i] = np.inf if i % 2 else np.nan
    for X in (S, ties, special, own):
        assert np.array_equal(R.select_loo(X, k, self0), _brute(X, k, self0))
    if self0 >= 0:
        got = R.select_loo(own, k, self0)
        for i in range(M):
            assert self0 + i not in got[i].tolist()


def test_a_duplicate_elsewhere_is_a_neighbour_and_the_verdicts():
    base = np.eye(4)
    real = base[[0, 1, 2, 0]]                                         # row 3 duplicates row 0
    ref = R.authenticity_ref64(real, np.array([[1.0, 0, 0, 0], [0, 1.0, 1.0, 0], [0, 0, 0, 1.0]]))
    assert ref['nn1'].tolist() == [3, 0, 0, 0] and ref['t1'].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert ref['i_star'].tolist() == [0, 1, 0]                        # ties go to the lower column
    # fake 0 sits on real 0, whose nearest other real is at similarity 1: 1 < 1 is false; fake 1: 0.707 < 0 false; fake 2: 0 < 1
    assert ref['authentic'].tolist() == [False, False, True] and ref['authenticity'] == 1.0 / 3.0
    assert R.most_similar(np.array([0.5, 0.9, 0.9, 0.1]), 3).tolist() == [1, 2, 0]
    idx, val, scores, pred = R.select_and_vote_loo(np.array([[9.0, 1.0, 1.0, 0.0]], np.float32), np.array([0, 1, 0, 1]), 2, 2, 1.0, 0)
    assert idx.tolist() == [[1, 2]] and np.allclose(scores, [[np.e, np.e]]) and pred.tolist() == [0]


def test_fragile_marks_the_near_ties():
    S_RR = np.array([[1.0, 0.5, 0.5 - 1e-6], [0.5, 1.0, 0.2], [0.5 - 1e-6, 0.2, 1.0]])
    S_FR = np.array([[0.9, 0.1, 0.0], [0.3, 0.3 - 1e-6, 0.0], [0.1, 0.2 + 1e-6, 0.0]])
    t1 = np.array([0.5, 0.5, 0.5 - 1e-6])
    fr, ff = R.fragile(S_RR, S_FR, t1, np.array([0, 0, 1]), np.array([0.9, 0.3, 0.5 + 1e-6]))
    assert fr.tolist() == [True, False, False] and ff.tolist() == [False, True, True]


def test_host_refusals_of_the_module():
    from contrad_amd import nearest, ops
    was_initialised = torch.cuda.is_initialized()
    rows, bank = torch.zeros(8, 4), torch.zeros(4, 8)
    for k, loo in ((0, False), (9, False), (8, True), (0, True)):
        with pytest.raises(ValueError, match='nearest: k'):
            nearest.neighbours(rows, bank, 8, k, leave_self_out=loo)
    with pytest.raises(ValueError, match='kernel limit'):
        nearest.neighbours(torch.zeros(3, 4), torch.zeros(4, 2000), 2000, ops.KNN_MAX_K + 1)
    with pytest.raises(ValueError, match='leave_self_out takes the rows of the bank itself'):
        nearest.neighbours(rows[:7], bank, 8, 1, leave_self_out=True)
    with pytest.raises(RuntimeError, match='a bank of'):
        nearest.neighbours(rows, torch.zeros(4, 9), 8, 1)
    with pytest.raises(RuntimeError, match='a bank of'):
        nearest.neighbours(torch.zeros(8, 5), bank, 8, 1)
    for k, loo in ((8, False), (7, True)):                            # the admitted limits get as far as the device check
        with pytest.raises(RuntimeError, match='CUDA float32'):
            nearest.neighbours(rows, bank, 8, k, leave_self_out=loo)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        nearest.real_state_of(torch.zeros(8, 4))
    with pytest.raises(ValueError, match='rows = 0'):
        nearest.check_retrieval(3, 0, 8, 8)
    with pytest.raises(ValueError, match='rows = 9'):
        nearest.check_retrieval(3, 9, 8, 8)
    with pytest.raises(ValueError, match='nearest: k'):
        nearest.check_retrieval(9, 2, 8, 8)
    assert nearest.most_similar(np.array([0.5, np.nan, 0.9, 0.9, -0.0, 0.0]), 6).tolist() == [2, 3, 0, 4, 5, 1]
    assert torch.cuda.is_initialized() == was_initialised


def test_command_line_refusals_and_defaults(tmp_path):
    from contrad_amd import nearest
    was_initialised = torch.cuda.is_initialized()
    P = nearest.parse_args(['enc/dis.pt', 'sndcgan', '--real', 'r.npz', '--fake', 'f.npz'])
    assert (P.k, P.rows, P.holdout, P.batch_size, P.seed, P.n_real, P.n_fake) == (8, 16, False, 500, None, None, None)
    no_test = str(tmp_path / 'no_test.npz')
    np.savez(no_test, x_train=np.zeros((8, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match='holds no x_test'):
        nearest.main(['enc/dis.pt', 'sndcgan', '--real', no_test, '--fake', no_test, '--holdout'])
    with pytest.raises(ValueError, match='--rows'):
        nearest.main(['enc/dis.pt', 'sndcgan', '--real', no_test, '--fake', no_test, '--rows', '-1'])
    assert torch.cuda.is_initialized() == was_initialised


def test_entry_point_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    f = lib().raw('contrad_knn_select_loo')
    M, n, k, C = 2, 8, 3, 2
    S, lab = (ctypes.c_float * (M * n))(), (ctypes.c_longlong * n)()
    idx, val = (ctypes.c_int * (M * n))(), (ctypes.c_float * (M * n))()
    sc, pred = (ctypes.c_float * (M * C))(), (ctypes.c_int * M)()
    ws = (ctypes.c_char * 16)()

    def call(S=S, ldS=n, M=M, n=n, self0=0, lab=lab, C=C, k=k, idx=idx, val=val, sc=sc, pred=pred, ws=ws, wsb_=16):
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)
        ip = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_int)) if a is not None else ctypes.POINTER(ctypes.c_int)()
        return f(vp(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), vp(lab), C, k, 10.0, ip(idx), vp(val), vp(sc),
                 ip(pred), vp(ws), ctypes.c_longlong(wsb_), ctypes.c_void_p(0))

    for bad in (dict(k=n), dict(k=n, self0=n - 1), dict(n=1, ldS=1, k=1), dict(n=1, ldS=1, k=1, M=1),
                dict(S=None), dict(lab=None), dict(idx=None), dict(val=None), dict(sc=None), dict(pred=None),
                dict(M=0), dict(n=0), dict(k=0), dict(k=n + 1, self0=-1), dict(k=n + 1, self0=n), dict(C=0), dict(C=1025),
                dict(n=2000, ldS=2000, k=1025), dict(ldS=n - 1), dict(wsb_=-1)):
        assert call(**bad) == -22, bad
    assert all(v == 0 for v in idx) and all(v == 0 for v in pred)
    assert lib().raw('contrad_abi_version')() == 3                    # an added entry point does not move the ABI version


def test_csv_line_and_the_hook_flag(tmp_path):
    from contrad_amd import nearest, prdc, train_gan, train_stylegan2
    was_initialised = torch.cuda.is_initialized()
    assert nearest.CSV_HEAD == 'step,authenticity,nearest_mean'
    assert nearest.csv_line(12, {'authenticity': 1.0 / 3.0, 'nearest_mean': 0.98765432}) == '12,0.333333,0.987654'
    assert prdc.HOOK_DEFAULTS['prdc_auth'] is False and 'authenticity' not in prdc.BEST_CHOICES
    on = ['--prdc_data', 'c10.npz', '--prdc_encoder', 'e.pt']
    parsers = (train_gan.parse_args, train_stylegan2.parse_args, lambda argv: train_stylegan2.parse_args(argv, contrad_script=True))
    for parse in parsers:
        Q = parse(['cfg.gin', 'sndcgan'])
        assert not hasattr(Q, 'prdc_auth') and prdc.check_hook_arguments(Q).prdc_auth is False         # off, and no attribute
        with_flag = vars(parse(['cfg.gin', 'sndcgan'] + on + ['--prdc_auth']))
        assert {k: v for k, v in with_flag.items() if not k.startswith('prdc_')} == vars(Q)         # the default dict is what it was
        assert prdc.check_hook_arguments(parse(['cfg.gin', 'sndcgan'] + on + ['--prdc_auth'])).prdc_auth is True
        assert prdc.check_hook_arguments(parse(['cfg.gin', 'sndcgan'] + on)).prdc_auth is False
        with pytest.raises(ValueError, match='--prdc_auth does nothing without --prdc_data'):
            prdc.check_hook_arguments(parse(['cfg.gin', 'sndcgan', '--prdc_auth']))
        with pytest.raises(SystemExit):
            parse(['cfg.gin', 'sndcgan'] + on + ['--prdc_best', 'authenticity'])
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    with pytest.raises(ValueError, match='--prdc_auth does nothing without --prdc_data'):
        train_gan.main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir',
                        str(tmp_path / 'run'), '--prdc_auth'])
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(str(tmp_path / 'run'))
