"""Weighted kNN evaluation on the GPU against the float64 yardstick (tests/knn_ref64.py): the select-and-vote kernel
alone on a given S, the classifier on features, the accuracy through a discriminator, the command line and the
``--knn_data`` hook of the training scripts (which must not move the trajectory by a bit).

Score tolerance of the kernel on a given S, relative, per class: (k + 32) * 2^-24 --
  one rounding of s * inv_temp, |arg| <= 20: at most 20 * 2^-25 absolute in the exponent = 10 * 2^-24 relative in exp;
  a few ulp of expf; k - 1 fp32 additions of positive terms: (k - 1) * 2^-24.
On features the similarities carry the fp32 error of two normalisations and of a d-term dot product of unit vectors,
worst case to first order in u = 2^-24: a sum of d squares d * u relative, halved by the square root, one rounding each
for the root and the division -> (d / 2 + 2.5) * u per normalised row (so a row's norm is within (d / 2 + 4) * u of 1),
(d + 5) * u for the pair; the dot product in any summation order d * u * sum |q_i b_i| <= d * u (Cauchy-Schwarz).
Together |ds| <= (2 d + 8) * u, which enters a score as a relative |ds| / T."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import knn_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
GUARD = 64
INV_TEMP = float(np.float32(3.7))        # |randn| < 5.4 over the 280 000 draws of the largest shape: |arg| <= 20
SHAPES = [(1, 1, 1, 1), (3, 7, 7, 2), (5, 300, 200, 10), (2, 1025, 1, 3), (2, 1024, 1024, 7), (4, 70000, 200, 100)]


def _guarded(numel, dtype, fill):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _raw_select(S_dev, ldS, M, n, labels_dev, C, k, inv_temp):
    """contrad_knn_select on caller-owned outputs with guard bands before and after each of the four."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    outs = [_guarded(M * k, torch.int32, -7), _guarded(M * k, torch.float32, -7.0), _guarded(M * C, torch.float32, -7.0),
            _guarded(M, torch.int32, -7)]
    nbytes = lib().raw('contrad_knn_select_workspace_bytes')(M, n, k, C)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device='cuda')
    ip = lambda t: ctypes.cast(ops._p(t), ctypes.POINTER(ctypes.c_int))
    rc = lib().raw('contrad_knn_select')(ops._p(S_dev), ctypes.c_longlong(ldS), M, n, ops._p(labels_dev), C, k, float(inv_temp),
                                         ip(outs[0][1]), ops._p(outs[1][1]), ops._p(outs[2][1]), ip(outs[3][1]), ops._p(ws),
                                         ctypes.c_longlong(ws.numel()), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for (buf, _), fill in zip(outs, (-7, -7.0, -7.0, -7)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), 'guard band overwritten'
    idx, val, sc, pred = (o[1].cpu().numpy() for o in outs)
    return idx.reshape(M, k), val.reshape(M, k), sc.reshape(M, C), pred


def _inputs(shape):
    """The three S variants of a shape and its labels (a few of them outside [0, C): they vote for nobody)."""
    M, n, k, C = shape
    r = np.random.RandomState(0)
    S = r.randn(M, n).astype(np.float32)
    labels = r.randint(0, C, n).astype(np.int64)
    if n >= 7:
        labels[[1, n // 2]] = [-1, C]
    ties = (np.round(S * 8) / 8).astype(np.float32)
    special = S.copy()
    special[:, ::3] = 0.0
    special[:, ::6] = -0.0
    for i in range(M):
        special[i, (7 * i + 1) % n] = np.nan
    return {'randn': S, 'ties': ties, 'special': special}, labels


def _score_error(got, ref):
    """Largest relative error over the finite, positive reference scores; everything else must match in kind."""
    fin = np.isfinite(ref) & (ref > 0)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.all(got[ref == 0] == 0)
    return float((np.abs(got[fin].astype(np.float64) - ref[fin]) / ref[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_select_kernel_on_a_given_S(shape, pad, margin):
    M, n, k, C = shape
    variants, labels = _inputs(shape)
    labels_dev = torch.from_numpy(labels).cuda()
    for name, S in variants.items():
        full = np.full((M, n + pad), np.inf, np.float32)             # +inf in the padding columns: never selected
        full[:, :n] = S
        S_dev = torch.from_numpy(full).cuda()
        idx, val, sc, pred = _raw_select(S_dev, n + pad, M, n, labels_dev, C, k, INV_TEMP)
        r_idx, r_val, r_sc, r_pred = R.select_and_vote(S, labels, C, k, INV_TEMP)
        tag = 'knn select %s %s ld+%d' % ('x'.join(map(str, shape)), name, pad)
        assert np.array_equal(idx, r_idx), tag
        assert np.array_equal(val.view(np.uint32), r_val.view(np.uint32)), tag       # the very floats, -0.0 and NaN included
        assert np.array_equal(pred, r_pred), tag
        margin(tag + ' scores', _score_error(sc, r_sc), (k + 32) * EPS)
        again = _raw_select(S_dev, n + pad, M, n, labels_dev, C, k, INV_TEMP)
        for a, b in zip((idx, val, sc, pred), again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag + ': two calls differ'


def test_wrapper_equals_the_entry_point_and_checks_its_arguments():
    from contrad_amd import ops
    shape = (5, 300, 200, 10)
    variants, labels = _inputs(shape)
    S_dev, labels_dev = torch.from_numpy(variants['ties']).cuda(), torch.from_numpy(labels).cuda()
    raw = _raw_select(S_dev, 300, 5, 300, labels_dev, 10, 200, INV_TEMP)
    for a, b in zip(raw, ops.knn_select(S_dev, 300, labels_dev, 10, 200, INV_TEMP)):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    # a row view of a wider matrix: only the first n columns are read
    wide = torch.full((5, 304), float('inf'), device='cuda')
    wide[:, :300] = S_dev
    assert torch.equal(ops.knn_select(wide, 300, labels_dev, 10, 200, INV_TEMP)[0].cpu(), torch.from_numpy(raw[0]))
    for bad in (dict(n=301), dict(n=0), dict(k=0), dict(k=301), dict(C=0), dict(C=1025)):
        a = dict(n=300, k=200, C=10); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.knn_select(S_dev, a['n'], labels_dev, a['C'], a['k'], INV_TEMP)
    with pytest.raises(RuntimeError):
        ops.knn_select(S_dev, 300, labels_dev[:299], 10, 200, INV_TEMP)
    with pytest.raises(RuntimeError):
        ops.knn_select(S_dev, 300, labels_dev.int(), 10, 200, INV_TEMP)
    with pytest.raises(RuntimeError):
        ops.knn_select(S_dev, 300, labels, 10, 200, INV_TEMP)                       # host labels
    with pytest.raises(RuntimeError):
        ops.knn_select(S_dev.double(), 300, labels_dev, 10, 200, INV_TEMP)


def test_entry_point_returns_einval_on_device_pointers():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    f = lib().raw('contrad_knn_select')
    S, lab = torch.zeros(2, 8, device='cuda'), torch.zeros(8, dtype=torch.int64, device='cuda')
    idx, val = torch.full((2, 3), -7, dtype=torch.int32, device='cuda'), torch.full((2, 3), -7.0, device='cuda')
    sc, pred = torch.full((2, 2), -7.0, device='cuda'), torch.full((2,), -7, dtype=torch.int32, device='cuda')
    ip = lambda t: ctypes.cast(ops._p(t), ctypes.POINTER(ctypes.c_int))

    def call(S=S, ldS=8, M=2, n=8, lab=lab, C=2, k=3, idx=idx, val=val, sc=sc, pred=pred, wsb=0):
        return f(ops._p(S), ctypes.c_longlong(ldS), M, n, ops._p(lab), C, k, 10.0, ip(idx), ops._p(val), ops._p(sc), ip(pred),
                 ctypes.c_void_p(0), ctypes.c_longlong(wsb), ops._stream())

    for bad in (dict(S=None), dict(lab=None), dict(idx=None), dict(val=None), dict(sc=None), dict(pred=None), dict(M=0),
                dict(n=0), dict(k=0), dict(k=9), dict(k=1025), dict(C=0), dict(C=1025), dict(ldS=7), dict(wsb=-1)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((val == -7).all()) and bool((sc == -7).all()) and bool((pred == -7).all())
    need = lib().raw('contrad_knn_select_workspace_bytes')(2, 8, 3, 2)
    if need == 0:                                                     # then the null workspace above is a valid call
        assert call() == 0
        torch.cuda.synchronize()
        assert idx[0].tolist() == [0, 1, 2] and pred.tolist() == [0, 0]            # all similarities equal: by column


# ---- the classifier on features ----
CASES = [(70, 301, 24, 20, 5, 'plain', 0), (70, 301, 24, 20, 5, 'plain', 1), (70, 301, 24, 20, 5, 'plain', 2),
         (70, 301, 24, 200, 5, 'clustered', 0), (70, 301, 24, 200, 5, 'clustered', 1), (70, 301, 24, 200, 5, 'clustered', 2),
         (33, 1030, 8192, 200, 10, 'clustered', 0), (70, 301, 24, 301, 5, 'clustered', 0)]
TEMP = 0.1


def _features(M, n, d, C, kind, seed):
    r = np.random.RandomState(seed)
    y = r.randint(0, C, n)
    if kind == 'clustered':
        cen = r.randn(C, d)
        bank = cen[y] + r.randn(n, d)
        q = cen[r.randint(0, C, M)] + r.randn(M, d)
    else:
        bank = r.randn(n, d)
        q = r.randn(M, d)
    return bank, y.astype(np.int64), q


def _compare_on_kept_rows(tag, ref, idx, pred, scores, k, d, margin):
    """Neighbour sets, predictions and scores on the rows the guard rule keeps; at most 10 % may be left out."""
    out = R.fragile_rows(ref['S'], ref['scores'], ref['k'])
    assert out.sum() <= 0.1 * len(out), (tag, int(out.sum()), len(out))
    keep = ~out
    assert all(set(a) == set(b) for a, b in zip(idx[keep].tolist(), ref['idx'][keep].tolist())), tag
    assert np.array_equal(pred[keep], ref['pred'][keep]), tag
    margin(tag + ' scores', _score_error(scores[keep], ref['scores'][keep]), ((k + 32) + (2 * d + 8) / TEMP) * EPS)
    return out


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d-k%d-C%d-%s-%d' % c)
def test_classifier_on_features(case, margin):
    from contrad_amd.knn import KNNClassifier
    M, n, d, k, C, kind, seed = case
    bank, y, q = _features(M, n, d, C, kind, seed)
    ref = R.knn_ref64(bank, y, q, C, k, TEMP)
    clf = KNNClassifier(torch.from_numpy(bank).float().cuda(), y, C, k=k, temp=TEMP)
    pred, scores, idx, val = clf.predict(torch.from_numpy(q).float().cuda(), neighbours=True)
    assert tuple(clf.bankT.shape) == (d, (n + 3) // 4 * 4) and bool((clf.bankT[:, n:] == 0).all())
    tag = 'knn classifier %dx%dx%d k%d C%d %s seed %d' % case
    _compare_on_kept_rows(tag, ref, idx.cpu().numpy(), pred.cpu().numpy(), scores.cpu().numpy(), k, d, margin)
    s_err = np.abs(val.cpu().numpy().astype(np.float64) - np.take_along_axis(ref['S'], idx.cpu().numpy().astype(np.int64), 1)).max()
    margin(tag + ' similarities', s_err, (2 * d + 8) * EPS)


def test_classifier_chunks_rows_and_clamps_k(margin):
    from contrad_amd import knn
    bank, y, q = _features(70, 301, 24, 5, 'clustered', 0)
    bank_dev, q_dev = torch.from_numpy(bank).float().cuda(), torch.from_numpy(q).float().cuda()
    whole = knn.KNNClassifier(bank_dev, torch.from_numpy(y).cuda(), 5, k=500, temp=TEMP)
    assert whole.k == 301
    chunked = knn.KNNClassifier(bank_dev, y, 5, k=301, temp=TEMP)
    chunked.chunk_rows = 16                                           # 70 rows: four chunks of 16 and one of 6
    parts = [chunked.predict(q_dev[i:i + 16], neighbours=True) for i in range(0, 70, 16)]      # one chunk per call
    for j, a in enumerate(chunked.predict(q_dev, neighbours=True)):
        assert torch.equal(a.view(torch.int32), torch.cat([p[j] for p in parts]).view(torch.int32))
    assert torch.equal(whole.predict(q_dev)[0], chunked.predict(q_dev)[0])
    with pytest.raises(ValueError):
        knn.KNNClassifier(bank_dev, np.where(y == 0, 5, y), 5)        # a label outside [0, 5)
    with pytest.raises(RuntimeError):
        whole.predict(q_dev[:, :23].contiguous())


# ---- through a discriminator ----
def _accuracy_both_ways(arch, margin, settle=0, k=200):
    from contrad_amd import features, knn, lineval
    from contrad_amd.models.gan import get_architecture
    data = lineval.synthetic_set(3, 4, 256, 64)
    torch.manual_seed(3)
    _, D = get_architecture(arch, (32, 32, 3))
    D = D.cuda()
    for p in D.parameters():
        p.requires_grad_(False)
    if settle:
        # A freshly drawn u / v pair underestimates every layer's sigma, and eval mode never iterates: through the 20
        # layers of the ResNet the features leave the fp32 range and their squared norm overflows.  A few train-mode
        # forwards run the power iterations any checkpoint has behind it.
        x = torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
        with torch.no_grad():
            for _ in range(settle):
                D.train()(x)
    D.eval()
    got = knn.knn_accuracy(D, data, 4, k=k, temp=TEMP, batch=100)
    assert got['n_test'] == 64
    dev = knn.to_device(data, 4, torch.device('cuda', 0))
    f_train, f_test = features.extract_features(D, dev['x_train'], 100), features.extract_features(D, dev['x_test'], 100)
    assert tuple(f_train.shape) == (256, D.d_penul)
    norms = f_train.double().norm(dim=1)
    margin('knn %s feature row norms' % arch, float((norms - 1).abs().max()), (D.d_penul / 2 + 4) * EPS)
    clf = knn.KNNClassifier(f_train, dev['y_train'], 4, k=k, temp=TEMP, normalize=False)
    pred = clf.predict(f_test)[0].cpu().numpy()
    ref = R.knn_ref64(f_train.cpu().numpy(), data['y_train'], f_test.cpu().numpy(), 4, k, TEMP)
    out = R.fragile_rows(ref['S'], ref['scores'], ref['k'])
    assert out.sum() <= 0.1 * len(out), int(out.sum())
    agreed = np.where(out, pred, ref['pred'])                         # a left-out row counts as agreeing
    assert np.array_equal(pred[~out], ref['pred'][~out])
    assert got['acc@1'] == 100.0 * int((agreed == data['y_test']).sum()) / 64
    return D, got


def test_accuracy_through_sndcgan(margin):
    D, got = _accuracy_both_ways('sndcgan', margin)
    assert D.d_penul == 8192 and not D.training


def test_accuracy_through_snresnet18(margin):
    # The pooled features of an untrained ResNet are nearly collinear: all 64 x 256 similarities lie in [0.9957, 0.9990],
    # closer together than the guard rule's 1e-5 at almost every rank (52 of 64 rows are left out at k = 200, 46 at
    # k = 20).  With k above the bank size (clamped to 256: every image votes) no rank boundary exists and no row is left
    # out; the selection itself is covered above.
    _accuracy_both_ways('snresnet18', margin, settle=8, k=1000)


# ---- scripts ----
SEED = 5
_RUNS = {}


def _tiny_npz(factory):
    from contrad_amd import lineval
    if 'npz' not in _RUNS:
        path = str(factory.mktemp('knn_data') / 'tiny.npz')
        np.savez(path, **lineval.synthetic_set(1, 4, 96, 32))
        _RUNS['npz'] = path
    return _RUNS['npz']


def _run(factory, graph, knn):
    key = (graph, knn)
    if key not in _RUNS:
        from contrad_amd.train_gan import main
        logdir = str(factory.mktemp('knn_run_%d%d' % key))
        gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
              '--seed', str(SEED), '--logdir', logdir] + (['--graph'] if graph else []) +
             (['--knn_data', _tiny_npz(factory), '--knn_k', '20'] if knn else []))
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


def _csv_rows(logdir):
    name = 'knn_%d.csv' % int(np.random.RandomState(SEED).randint(10000))
    with open(os.path.join(logdir, name)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,acc@1'
    return [(int(s), float(a)) for s, a in (ln.split(',') for ln in lines[1:])]


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_hook_leaves_the_checkpoints_bitwise_alone(graph, tmp_path_factory):
    plain, hooked = _run(tmp_path_factory, graph, False), _run(tmp_path_factory, graph, True)
    for name in ('gen.pt', 'dis.pt', 'optim.pt'):
        _same(torch.load(os.path.join(plain, name), map_location='cpu'), torch.load(os.path.join(hooked, name), map_location='cpu'))
    rows = _csv_rows(hooked)
    assert [s for s, _ in rows] == [2, 4] and all(0.0 <= a <= 100.0 for _, a in rows)
    assert not [f for f in os.listdir(plain) if f.startswith('knn_')]
    # the logged figure is the checkpoint's: knn_accuracy on the saved discriminator gives the last row
    from contrad_amd import knn, lineval
    from contrad_amd.models.gan import get_architecture
    _, D = get_architecture('sndcgan', (32, 32, 3))
    D.load_state_dict(torch.load(os.path.join(hooked, 'dis.pt'), map_location='cpu'))
    D = D.cuda().eval()
    again = knn.knn_accuracy(D, lineval.load_npz(_tiny_npz(tmp_path_factory)), 4, k=20, temp=0.1)
    assert abs(again['acc@1'] - rows[-1][1]) < 1e-3                   # (the csv keeps four decimals)


def test_command_line_writes_the_json(tmp_path):
    import test_knn
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(4)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    torch.save(D.state_dict(), str(tmp_path / 'dis.pt'))
    path = test_knn.main([str(tmp_path / 'dis.pt'), 'sndcgan', '--n_classes', '4', '--synthetic', '--synthetic_size', '256', '64',
                          '--seed', '3', '--batch_size', '100'])
    assert path == str(tmp_path / 'knn_3.json')
    with open(path) as f:
        out = json.load(f)
    assert out['n_test'] == 64 and out['n_train'] == 256 and out['k'] == 200 and 0.0 <= out['acc@1'] <= 100.0
    with pytest.raises(ValueError):                                   # labels up to 3 with --n_classes 2
        test_knn.main([str(tmp_path / 'dis.pt'), 'sndcgan', '--n_classes', '2', '--data', _tiny_npz_at(tmp_path)])


def _tiny_npz_at(tmp_path):
    from contrad_amd import lineval
    path = str(tmp_path / 'tiny.npz')
    np.savez(path, **lineval.synthetic_set(1, 4, 96, 32))
    return path


def test_stylegan2_loop_with_the_hook(tmp_path):
    from contrad_amd import config
    from contrad_amd.train_stylegan2 import main
    logdir = str(tmp_path / 'run')
    main([os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
          '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
          '--seed', str(SEED), '--logdir', logdir, '--knn_data', _tiny_npz_at(tmp_path), '--knn_k', '20'])
    rows = _csv_rows(logdir)
    assert [s for s, _ in rows] == [2] and 0.0 <= rows[0][1] <= 100.0
