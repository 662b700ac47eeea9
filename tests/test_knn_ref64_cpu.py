"""The float64 yardstick of the kNN vote (tests/knn_ref64.py) against a brute-force loop, its tie / -0.0 / NaN rules,
the clamp of k, and the argument errors of the Python layer and of the C entry point (raised before any GPU call)."""
import ctypes

import numpy as np
import pytest
import torch

import knn_ref64 as R


def _better(S_row, a, b):
    """Does column a come before column b in the neighbour order?"""
    va, vb = S_row[a], S_row[b]
    if np.isnan(va) or np.isnan(vb):
        if np.isnan(va) and np.isnan(vb):
            return a < b
        return np.isnan(vb)
    if va != vb:                      # -0.0 == +0.0 in this comparison, as the rule asks
        return va > vb
    return a < b


def _brute(bank, labels, q, C, k, T):
    bn = np.array([r / max(np.sqrt(sum(x * x for x in r)), 1e-12) for r in bank])
    qn = np.array([r / max(np.sqrt(sum(x * x for x in r)), 1e-12) for r in q])
    preds, idxs, scs = [], [], []
    for i in range(len(qn)):
        s = np.array([sum(a * b for a, b in zip(qn[i], bn[j])) for j in range(len(bn))])
        left, chosen = list(range(len(bn))), []
        for _ in range(k):
            best = left[0]
            for j in left[1:]:
                if _better(s, j, best):
                    best = j
            chosen.append(best)
            left.remove(best)
        sc = [0.0] * C
        for j in chosen:
            sc[labels[j]] += np.exp(s[j] / T)
        best_c = 0
        for c in range(1, C):
            if sc[c] > sc[best_c]:
                best_c = c
        preds.append(best_c); idxs.append(chosen); scs.append(sc)
    return np.array(idxs), np.array(scs), np.array(preds)


@pytest.mark.parametrize('shape', [(3, 7, 3, 2), (3, 7, 7, 2)])
def test_yardstick_equals_brute_force(shape):
    M, n, k, C = shape
    r = np.random.RandomState(0)
    y = r.randint(0, C, n)
    bank, q = r.randn(n, 5), r.randn(M, 5)
    ref = R.knn_ref64(bank, y, q, C, k, 0.1)
    idx, sc, pred = _brute(bank, y, q, C, k, 0.1)
    assert np.array_equal(ref['idx'], idx) and np.array_equal(ref['pred'], pred)
    assert np.abs(ref['scores'] - sc).max() <= 1e-12 * np.abs(sc).max()


def test_duplicated_bank_rows_are_taken_in_column_order():
    base = np.eye(3, 4)                                      # axis vectors: every similarity is exactly 0 or 1
    bank = base[[0, 1, 0, 2, 0, 1, 0]]                       # columns 0, 2, 4, 6 are one point; 1 and 5 another
    y = np.array([0, 1, 1, 0, 1, 0, 0])
    ref = R.knn_ref64(bank, y, base[:1] * 3.0, 2, 3, 0.5)
    assert ref['idx'].tolist() == [[0, 2, 4]]                # similarity 1 four times: the first three columns
    assert np.allclose(ref['scores'], [[np.exp(2.0), 2 * np.exp(2.0)]]) and ref['pred'].tolist() == [1]
    assert R.knn_ref64(bank, y, base[:1] * 3.0, 2, 6, 0.5)['idx'].tolist() == [[0, 2, 4, 6, 1, 3]]   # then the zeros, by column
    # an exact score tie goes to the lowest class
    assert R.predict(np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 1.0]])).tolist() == [1, 0]


def test_signed_zero_and_nan_rule():
    S = np.array([[np.nan, -0.0, 1.0, 0.0, -1.0, np.nan, 0.0]], np.float32)
    idx = R.select(S, 7)
    assert idx.tolist() == [[2, 1, 3, 6, 4, 0, 5]]            # zeros by column whatever their sign; NaN last, by column
    idx, val, scores, pred = R.select_and_vote(S, np.array([0, 0, 1, 1, 0, 1, 1]), 2, 4, 2.0)
    assert idx.tolist() == [[2, 1, 3, 6]] and np.signbit(val[0, 1]) and not np.signbit(val[0, 2])   # the very floats
    assert np.allclose(scores, [[1.0, np.exp(2.0) + 2.0]]) and pred.tolist() == [1]
    # a NaN neighbour poisons its class's score; the prediction ranks that score below every number
    _, _, scores, pred = R.select_and_vote(S, np.array([1, 0, 1, 1, 0, 1, 1]), 2, 7, 2.0)
    assert np.isnan(scores[0, 1]) and not np.isnan(scores[0, 0]) and pred.tolist() == [0]
    assert R.predict(np.array([[np.nan, np.nan]])).tolist() == [0]
    # a label outside [0, C) votes for nobody
    _, _, scores, _ = R.select_and_vote(S, np.array([0, 5, -1, 1, 0, 1, 1]), 2, 3, 2.0)
    assert np.allclose(scores, [[0.0, 1.0]])


def test_k_is_clamped_to_the_bank():
    r = np.random.RandomState(2)
    bank, q, y = r.randn(7, 3), r.randn(2, 3), r.randint(0, 2, 7)
    a, b = R.knn_ref64(bank, y, q, 2, 200, 0.1), R.knn_ref64(bank, y, q, 2, 7, 0.1)
    assert a['k'] == 7 and np.array_equal(a['idx'], b['idx']) and np.array_equal(a['scores'], b['scores'])


def test_fragile_rows():
    S = np.array([[0.9, 0.5, 0.5 - 1e-6, 0.1], [0.9, 0.5, 0.4, 0.1]])
    sc = np.array([[1.0, 2.0], [1.0, 1.00001]])
    assert R.fragile_rows(S, np.array([[1.0, 2.0]] * 2), 2).tolist() == [True, False]
    assert R.fragile_rows(S, sc, 4).tolist() == [False, True]


def test_python_layer_argument_errors():
    from contrad_amd import knn, ops
    S = torch.zeros(2, 8)
    y = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.knn_select(S, 8, y, 2, 1, 10.0)                   # host S
    with pytest.raises(RuntimeError, match='CUDA float32'):
        knn.KNNClassifier(torch.zeros(8, 4), y, 2)            # host bank
    with pytest.raises(RuntimeError, match='CUDA float32'):
        knn.KNNClassifier(torch.zeros(8, 4, dtype=torch.float64), y, 2)
    with pytest.raises(ValueError, match='n_classes 2'):
        knn.check_labels(np.array([0, 1, 2]), 2)
    with pytest.raises(ValueError, match='n_classes 2'):
        knn.check_labels(np.array([-1, 1]), 2)
    knn.check_labels(np.array([0, 1]), 2)
    knn.check_labels(np.array([], np.int64), 2)
    P = knn.parse_args(['run/dis.pt', 'sndcgan', '--synthetic'])
    assert (P.k, P.temp, P.batch_size, P.n_classes, P.seed, P.data) == (200, 0.1, 500, 10, None, None)
    from contrad_amd import train_gan, train_stylegan2
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'])
        assert (Q.knn_data, Q.knn_k, Q.knn_temp) == (None, 200, 0.1)          # off by default


def test_entry_point_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    f = lib().raw('contrad_knn_select')
    wsb = lib().raw('contrad_knn_select_workspace_bytes')
    M, n, k, C = 2, 8, 3, 2
    S, lab = (ctypes.c_float * (M * n))(), (ctypes.c_longlong * n)()
    idx, val = (ctypes.c_int * (M * k))(), (ctypes.c_float * (M * k))()
    sc, pred = (ctypes.c_float * (M * C))(), (ctypes.c_int * M)()
    ws = (ctypes.c_char * 16)()

    def call(S=S, ldS=n, M=M, n=n, lab=lab, C=C, k=k, idx=idx, val=val, sc=sc, pred=pred, ws=ws, wsb_=16):
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)
        ip = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_int)) if a is not None else ctypes.POINTER(ctypes.c_int)()
        return f(vp(S), ctypes.c_longlong(ldS), M, n, vp(lab), C, k, 10.0, ip(idx), vp(val), vp(sc), ip(pred), vp(ws),
                 ctypes.c_longlong(wsb_), ctypes.c_void_p(0))

    for bad in (dict(S=None), dict(lab=None), dict(idx=None), dict(val=None), dict(sc=None), dict(pred=None),
                dict(M=0), dict(n=0), dict(k=0), dict(k=n + 1), dict(n=2000, ldS=2000, k=1025), dict(C=0), dict(C=1025),
                dict(ldS=n - 1), dict(wsb_=-1)):
        assert call(**bad) == -22, bad
    assert wsb(M, n, k, C) >= 0
    for bad in ((0, n, k, C), (M, 0, 1, C), (M, n, 0, C), (M, n, n + 1, C), (M, 2000, 1025, C), (M, n, k, 0), (M, n, k, 1025)):
        assert wsb(*bad) == -22, bad
    assert all(v == 0 for v in idx) and all(v == 0 for v in pred)
