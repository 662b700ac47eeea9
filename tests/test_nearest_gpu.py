"""The memorisation check on the GPU against the float64 yardstick (tests/nearest_ref64.py): the leave-self-out argument of
the select-and-vote kernel alone on a given S (exact), the wrapper, ``nearest`` on features against float64, the retrieval
figure, the command line, the ``--prdc_auth`` hook of the training scripts (which must not move the trajectory by a bit)
and leave-one-out kNN.

Tolerances: the score tolerance of the kernel on a given S is tests/test_knn_gpu.py's (k + 32) * 2^-24 (every |value *
inv_temp| here stays below 20, as it asks); a device similarity of unit rows differs from the float64 one by at most
(2 d + 8) * 2^-24 (derived at the head of that file).  Rows the guard rule of ``nearest_ref64.fragile`` marks (top-two gap or
|s - t1| below 1e-5) are left out of the exact comparisons, at most 5 % of either set.

The two feature sets (RandomState(5); real row n_r - 1 duplicates row 0; the first fakes are copies, a real row plus
0.05 * randn), float64 reference on the CPU: (64, 300, 200) with 60 copies leaves out 0.5 % of the fakes and 1.3 % of the
reals, authenticity 0.325, 0 of the 60 copies authentic; (128, 1030, 70) with 20 copies leaves out 0 % / 0.4 %, authenticity
0.386, 0 of 20."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import grid_ref
import knn_ref64
import nearest_ref64 as R
import png_reader
import test_knn_gpu as TK
import test_prdc_gpu as TP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
INV_TEMP = TK.INV_TEMP
# (M, n, k, C, self0): k = n - 1, all others; k = 1; a chunk offset whose last row's own column is n - 1; rows 2 and 3 beyond the
# bank (nothing left out there); own columns 1021..1024 straddle the 1024-column compaction round; k at the LDS limit; no exclusion
CASES = [(5, 5, 4, 2, 0), (3, 8, 1, 1, 0), (6, 37, 5, 3, 31), (4, 37, 36, 3, 35), (4, 1030, 7, 10, 1021), (2, 2051, 1024, 7, 0),
         (3, 300, 200, 10, -1)]
T_TIE = np.float32(0.5)


def _raw_select_loo(S_dev, ldS, M, n, self0, labels_dev, C, k, inv_temp):
    """contrad_knn_select_loo on caller-owned outputs with guard bands before and after each of the four."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    outs = [TK._guarded(M * k, torch.int32, -7), TK._guarded(M * k, torch.float32, -7.0), TK._guarded(M * C, torch.float32, -7.0),
            TK._guarded(M, torch.int32, -7)]
    ip = lambda t: ctypes.cast(ops._p(t), ctypes.POINTER(ctypes.c_int))
    ws = torch.empty(16, dtype=torch.uint8, device='cuda')
    rc = lib().raw('contrad_knn_select_loo')(ops._p(S_dev), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), ops._p(labels_dev),
                                             C, k, float(inv_temp), ip(outs[0][1]), ops._p(outs[1][1]), ops._p(outs[2][1]),
                                             ip(outs[3][1]), ops._p(ws), ctypes.c_longlong(ws.numel()), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for (buf, _), fill in zip(outs, (-7, -7.0, -7.0, -7)):
        assert bool((buf[:TK.GUARD] == fill).all()) and bool((buf[-TK.GUARD:] == fill).all()), 'guard band overwritten'
    idx, val, sc, pred = (o[1].cpu().numpy() for o in outs)
    return idx.reshape(M, k), val.reshape(M, k), sc.reshape(M, C), pred


def _own(case, i):
    """The column row i leaves out, or None."""
    M, n, k, C, self0 = case
    return self0 + i if self0 >= 0 and self0 + i < n else None


def _tie_rows(case, r):
    """The ties variant, in eighths: per row ``a`` columns above T_TIE, a run of ``b`` columns equal to it, the rest below,
    with a < k <= a + b, and the row's own column holding exactly T_TIE -- the threshold value of the row.  The run lies
    after the own column (position 'before': the own column comes before the run), around it ('inside') or before it
    ('after'), by row, where the geometry allows.  Returns (S, [(position or None, run columns)])."""
    M, n, k, C, self0 = case
    S = np.empty((M, n), np.float32)
    info = []
    for i in range(M):
        e = _own(case, i)
        others = n - (e is not None)
        b = min(3, others)
        a = max(k - 2, 0) if max(k - 2, 0) + b <= others else others - b
        assert a < k <= a + b
        run, pos = None, None
        if e is not None:
            layouts = {'before': [e + 1 + j for j in range(b)], 'after': [e - 1 - j for j in range(b)],
                       'inside': [e - 1, e + 1] + ([e + 2] if e + 2 < n else [e - 2])[:b - 2]}
            for want in (('before', 'inside', 'after') * 2)[i % 3:i % 3 + 3]:
                if len(layouts[want]) == b and all(0 <= j < n for j in layouts[want]):
                    run, pos = layouts[want], want
                    break
        if run is None:                                               # no own column (or a bank too small to place the run by rule)
            free = [j for j in range(n) if j != e]
            run = [free[j] for j in r.choice(len(free), b, replace=False)]
        rest = np.array([j for j in range(n) if j != e and j not in run])
        above = set(rest[r.choice(len(rest), a, replace=False)].tolist()) if a else set()
        for j in range(n):
            S[i, j] = 1.0 + r.randint(0, 25) / 8.0 if j in above else -1.0 - r.randint(0, 25) / 8.0
        S[i, run] = T_TIE
        if e is not None:
            S[i, e] = T_TIE
        info.append((pos, sorted(run)))
    return S, info


def _inputs(case):
    M, n, k, C, self0 = case
    r = np.random.RandomState(0)
    S = r.randn(M, n).astype(np.float32)
    labels = r.randint(0, C, n).astype(np.int64)
    if n >= 7:
        labels[[1, n // 2]] = [-1, C]
    out = {}
    for name, v in (('own=max', np.float32(5.25)), ('own=nan', np.nan), ('own=inf', np.inf)):
        x = S.copy()
        for i in range(M):
            if _own(case, i) is not None:
                x[i, _own(case, i)] = v
        out[name] = x
    assert self0 < 0 or out['own=max'].max() == 5.25 and S.max() < 5.25      # the own column holds the row maximum
    ties, info = _tie_rows(case, r)
    out['ties'] = ties
    few = np.full((M, n), np.nan, np.float32)                         # fewer than k numbers among the others: the threshold is a NaN,
    for i in range(M):                                                # whose key the kernel also gives the column it skips
        free = [j for j in range(n) if j != _own(case, i)]
        few[i, r.choice(free, k // 2, replace=False)] = S[i, :k // 2]
        if _own(case, i) is not None:
            few[i, _own(case, i)] = 1.0 if i % 2 else np.nan
    out['nan-threshold'] = few
    return out, info, labels


def test_the_ties_variant_puts_the_own_column_before_inside_and_after_the_run():
    """On the reference side: in every row the k-th value is T_TIE, the own column holds it too, and over the chunk-offset
    case the own column lies before, inside and after the run of the other columns that equal it."""
    for case in CASES:
        M, n, k, C, self0 = case
        variants, info, labels = _inputs(case)
        S = variants['ties']
        idx = R.select_loo(S, k, self0)
        seen = set()
        for i in range(M):
            e = _own(case, i)
            run = [j for j in range(n) if j != e and S[i, j] == T_TIE]
            assert S[i, idx[i, k - 1]] == T_TIE and run == info[i][1] and len(run) >= min(2, n - 2), (case, i)
            if e is not None:
                assert S[i, e] == T_TIE and e not in idx[i].tolist()
                pos = 'before' if e < run[0] else 'after' if e > run[-1] else 'inside'
                assert info[i][0] in (pos, None)
                seen.add(pos)
        if case == (6, 37, 5, 3, 31):
            assert seen == {'before', 'inside', 'after'}
            assert all(len(info[i][1]) > k - int((S[i] > T_TIE).sum()) for i in range(M))      # the threshold cuts the run


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_select_kernel_leaves_the_own_column_out(case, pad, margin):
    M, n, k, C, self0 = case
    variants, _, labels = _inputs(case)
    labels_dev = torch.from_numpy(labels).cuda()
    for name, S in variants.items():
        full = np.full((M, n + pad), np.inf, np.float32)             # +inf in the padding columns: never selected
        full[:, :n] = S
        S_dev = torch.from_numpy(full).cuda()
        idx, val, sc, pred = _raw_select_loo(S_dev, n + pad, M, n, self0, labels_dev, C, k, INV_TEMP)
        r_idx, r_val, r_sc, r_pred = R.select_and_vote_loo(S, labels, C, k, INV_TEMP, self0)
        tag = 'knn select loo %s %s ld+%d' % ('x'.join(map(str, case)), name, pad)
        assert np.array_equal(idx, r_idx), tag
        assert np.array_equal(val.view(np.uint32), r_val.view(np.uint32)), tag       # the very floats
        assert np.array_equal(pred, r_pred), tag
        margin(tag + ' scores', TK._score_error(sc, r_sc), (k + 32) * EPS)
        for i in range(M):
            assert _own(case, i) not in idx[i].tolist(), tag
        again = _raw_select_loo(S_dev, n + pad, M, n, self0, labels_dev, C, k, INV_TEMP)
        for a, b in zip((idx, val, sc, pred), again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag + ': two calls differ'
        if self0 < 0:                                                 # nothing left out: contrad_knn_select bit for bit
            plain = TK._raw_select(S_dev, n + pad, M, n, labels_dev, C, k, INV_TEMP)
            for a, b in zip((idx, val, sc, pred), plain):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag + ': differs from contrad_knn_select'


def test_wrapper_equals_the_entry_point_and_checks_its_arguments():
    from contrad_amd import ops
    case = (6, 37, 5, 3, 31)
    variants, _, labels = _inputs(case)
    labels_dev = torch.from_numpy(labels).cuda()
    for name in ('own=inf', 'ties'):
        S_dev = torch.from_numpy(variants[name]).cuda()
        raw = _raw_select_loo(S_dev, 37, 6, 37, 31, labels_dev, 3, 5, INV_TEMP)
        for a, b in zip(raw, ops.knn_select(S_dev, 37, labels_dev, 3, 5, INV_TEMP, self0=31)):
            assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
        raw = TK._raw_select(S_dev, 37, 6, 37, labels_dev, 3, 5, INV_TEMP)
        for a, b in zip(raw, ops.knn_select(S_dev, 37, labels_dev, 3, 5, INV_TEMP)):                # the default leaves nothing out
            assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert ops.knn_select(S_dev, 37, labels_dev, 3, 36, INV_TEMP, self0=0)[0].shape == (6, 36)      # k = n - 1
    assert ops.knn_select(S_dev, 37, labels_dev, 3, 37, INV_TEMP, self0=37)[0].shape == (6, 37)     # no row has an own column
    for bad in (dict(k=37, self0=0), dict(k=37, self0=36), dict(k=38, self0=-1), dict(k=0, self0=3)):
        with pytest.raises(RuntimeError, match='outside'):
            ops.knn_select(S_dev, 37, labels_dev, 3, bad['k'], INV_TEMP, self0=bad['self0'])


# ---- features against float64 ----
SETS = [(64, 300, 200, 60), (128, 1030, 70, 20)]
_REF = {}


def _set(case):
    if case not in _REF:
        d, n_r, n_f, copies = case
        r = np.random.RandomState(5)
        real = r.randn(n_r, d)
        real[n_r - 1] = real[0]
        fake = r.randn(n_f, d)
        src = r.randint(0, n_r, copies)
        fake[:copies] = real[src] + 0.05 * r.randn(copies, d)
        _REF[case] = (real, fake, R.authenticity_ref64(real, fake))
    return _REF[case]


@pytest.mark.parametrize('case', SETS, ids=lambda c: 'd%d-%dx%d-%dcopies' % c)
def test_authenticity_on_features_against_float64(case, margin, monkeypatch):
    from contrad_amd import features, nearest, ops
    d, n_r, n_f, copies = case
    real, fake, ref = _set(case)
    fr, ff = ref['fragile_real'], ref['fragile_fake']
    print('nearest features d%d %dx%d: float64 authenticity %.4f, %d of %d copies authentic, left out %.1f %% of the fakes, %.1f %% of '
          'the reals' % (d, n_r, n_f, ref['authenticity'], int(ref['authentic'][:copies].sum()), copies, 100.0 * ff.mean(), 100.0 * fr.mean()))
    assert ff.sum() <= 0.05 * n_f and fr.sum() <= 0.05 * n_r                  # the cap, before anything is compared
    assert 0.2 < ref['authenticity'] < 0.6 and ref['authentic'][:copies].sum() <= 1 and ref['nn1'][0] == n_r - 1 and ref['nn1'][n_r - 1] == 0
    if n_r > 512:
        monkeypatch.setattr(features, 'MAX_CHUNK_ROWS', 256)                 # 1030 reals: chunks at rows 0, 256, 512, 768, 1024
        assert features.chunk_rows_of(ops.round_up(n_r, 4)) == 256
    Rd, Fd = torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda()
    state = nearest.real_state_of(Rd)
    bankT, t1, nn1 = state
    assert t1.dtype == torch.float32 and nn1.dtype == torch.int32 and tuple(t1.shape) == tuple(nn1.shape) == (n_r,)
    tag = 'nearest features d%d %dx%d' % (d, n_r, n_f)
    assert np.array_equal(nn1.cpu().numpy()[~fr], ref['nn1'][~fr]), tag
    margin(tag + ' t1', np.abs(t1.cpu().numpy().astype(np.float64) - ref['t1']).max(), (2 * d + 8) * EPS)
    rows = features.normalize_rows(Rd)
    kth = torch.empty(n_r, device='cuda')
    starts = []
    for i, S in features.similarity_chunks(rows, bankT):                       # the same chunks through the other kernel
        ops.prdc_kth(S, n_r, 1, self0=i, out=kth[i:i + S.shape[0]])
        starts.append(i)
    assert len(starts) == (5 if n_r > 512 else 1)
    assert torch.equal(t1.view(torch.int32), kth.view(torch.int32)), tag + ': select and prdc_kth disagree'
    i_star, s, authentic = (v.cpu().numpy() for v in nearest.verdicts(features.normalize_rows(Fd), state))
    assert np.array_equal(i_star[~ff], ref['i_star'][~ff]), tag
    assert np.array_equal(authentic[~ff], ref['authentic'][~ff]), tag
    margin(tag + ' s', np.abs(s.astype(np.float64) - ref['S_FR'][np.arange(n_f), i_star]).max(), (2 * d + 8) * EPS)
    out = nearest.authenticity(Rd, Fd)
    assert (out['n_real'], out['n_fake'], out['n_authentic']) == (n_r, n_f, int(authentic.sum()))
    assert out['authenticity'] == out['n_authentic'] / n_f and out['note'] == nearest.NOTE
    decided = int(ref['authentic'][~ff].sum())
    assert decided <= out['n_authentic'] <= decided + int(ff.sum())
    margin(tag + ' nearest_mean', abs(out['nearest_mean'] - s.astype(np.float64).mean()), n_f * 2.0 ** -52)
    margin(tag + ' real_nearest_mean', abs(out['real_nearest_mean'] - ref['t1'].mean()), (2 * d + 8) * EPS)
    assert nearest.authenticity(None, Fd, real_state=state) == out
    with pytest.raises(ValueError):
        nearest.real_state_of(Rd[:1])
    with pytest.raises(ValueError):
        nearest.authenticity(Rd, Fd[:0])


# ---- the figure ----
def test_retrieval_and_its_grid():
    from contrad_amd import nearest
    r = np.random.RandomState(2)
    real_f, fake_f = r.randn(12, 16), r.randn(7, 16)
    fake_f[2] = real_f[3] + 0.01 * r.randn(16)
    fake_f[5] = fake_f[2]                                             # a tie in s: the lower fake index comes first
    real_u8 = r.randint(0, 256, (12, 8, 8, 3)).astype(np.uint8)
    fake_u8 = r.randint(0, 256, (7, 8, 8, 3)).astype(np.uint8)
    S = R.normalize64(fake_f) @ R.normalize64(real_f).T
    want = R.most_similar(S.max(1), 4)
    assert want[:2].tolist() == [2, 5]
    Rd, Fd = torch.from_numpy(real_f).float().cuda(), torch.from_numpy(fake_f).float().cuda()
    chosen, idx, val = nearest.retrieval(Rd, Fd, 3, 4)
    assert chosen.tolist() == want.tolist()
    assert np.array_equal(idx.cpu().numpy(), R.select_loo(S[want], 3))
    assert np.abs(val.cpu().numpy() - np.take_along_axis(S[want], idx.cpu().numpy().astype(np.int64), 1)).max() < (2 * 16 + 8) * EPS
    canvas = nearest.retrieval_grid(torch.from_numpy(real_u8).cuda(), torch.from_numpy(fake_u8).cuda(), chosen, idx)
    cells = np.concatenate([np.concatenate([fake_u8[j:j + 1], real_u8[idx[i].cpu().numpy()]]) for i, j in enumerate(want)])
    host = cells.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    assert canvas.dtype == torch.uint8 and np.array_equal(canvas.cpu().numpy(), grid_ref.grid_ref(host, nrow=4))
    for bad in (dict(k=13), dict(k=0), dict(rows=0), dict(rows=8)):
        a = dict(k=3, rows=4); a.update(bad)
        with pytest.raises(ValueError):
            nearest.retrieval(Rd, Fd, a['k'], a['rows'])


# ---- scripts ----
def test_command_line_writes_the_json_and_the_png(tmp_path):
    import test_nearest
    from contrad_amd import lineval, nearest
    data = lineval.synthetic_set(1, 4, 96, 32)
    real = str(tmp_path / 'real.npz')
    np.savez(real, x_train=data['x_train'], x_test=data['x_test'])
    os.makedirs(str(tmp_path / 'samples'))
    os.makedirs(str(tmp_path / 'other'))
    images = np.concatenate([data['x_train'][:12], data['x_test'][:12]])
    fake, other = str(tmp_path / 'samples' / 'samples.npz'), str(tmp_path / 'other' / 'samples.npz')
    np.savez(fake, images=images)
    np.savez(other, images=images)
    torch.save(TP._encoder(4)[1].state_dict(), str(tmp_path / 'enc.pt'))
    args = [str(tmp_path / 'enc.pt'), 'sndcgan', '--real', real, '--fake', fake, '--seed', '3', '--k', '3', '--rows', '4', '--holdout']
    path = test_nearest.main(args)
    assert path == str(tmp_path / 'samples' / 'nearest_3.json')
    png = str(tmp_path / 'samples' / 'nearest_3.png')
    with open(path) as f:
        out = json.load(f)
    assert set(out) == {'authenticity', 'n_authentic', 'nearest_mean', 'real_nearest_mean', 'n_real', 'n_fake', 'note', 'k', 'rows',
                        'holdout_authenticity', 'holdout_nearest_mean', 'n_holdout', 'fakes', 'nearest', 'similarity'}
    assert (out['n_real'], out['n_fake'], out['n_holdout'], out['k'], out['rows']) == (96, 24, 32, 3, 4)
    assert out['authenticity'] == out['n_authentic'] / 24 and 0.0 <= out['holdout_authenticity'] <= 1.0
    assert len(set(out['fakes'])) == 4 and all(j < 12 for j in out['fakes'])               # the copies of training images come first
    assert [row[0] for row in out['nearest']] == out['fakes']                              # ... each next to the image it copies
    dev = torch.device('cuda', 0)
    canvas = nearest.retrieval_grid(torch.from_numpy(data['x_train']).to(dev), torch.from_numpy(images).to(dev),
                                    torch.tensor(out['fakes'], device=dev), torch.tensor(out['nearest'], device=dev, dtype=torch.int32))
    assert tuple(canvas.shape) == (4 * 34 + 2, 4 * 34 + 2, 3) and np.array_equal(png_reader.read_png(png), canvas.cpu().numpy())
    first = [open(p, 'rb').read() for p in (path, png)]
    assert test_nearest.main(args) == path and [open(p, 'rb').read() for p in (path, png)] == first      # byte-identical
    path = test_nearest.main(args[:4] + ['--fake', other, '--seed', '3', '--rows', '0'])
    with open(path) as f:
        out = json.load(f)
    assert sorted(os.listdir(str(tmp_path / 'other'))) == ['nearest_3.json', 'samples.npz']                # --rows 0: no png
    assert 'holdout_authenticity' not in out and 'fakes' not in out
    for bad in (['--fake', fake, '--rows', '25'], ['--fake', fake, '--k', '97'], ['--fake', fake, '--n_real', '1']):
        with pytest.raises(ValueError):
            test_nearest.main(args[:4] + bad)


def test_hook_appends_the_authenticity_and_leaves_the_checkpoints_bitwise_alone(tmp_path_factory):
    from contrad_amd import features, nearest
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_gan import main
    plain = TP._run(tmp_path_factory, False, False)
    d = TP._files(tmp_path_factory)
    hooked = str(tmp_path_factory.mktemp('auth_run'))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', hooked] + TP._hook_flags(tmp_path_factory, None) + ['--prdc_n', '64', '--prdc_auth'])
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    assert not [f for f in os.listdir(plain) if f.startswith('auth_')]
    with open(os.path.join(hooked, 'auth_%d.csv' % TP.EVAL_SEED)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,authenticity,nearest_mean' and len(lines) == 3
    dev = torch.device('cuda', 0)
    E = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[1], str(d / 'enc.pt'), dev)
    real_u8 = torch.from_numpy(features.load_images(str(d / 'real.npz'), 'x_train')).to(dev)
    for line, (step, name) in zip(lines[1:], ((2, 'gen_2.pt'), (4, 'gen.pt'))):
        G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, name), dev)
        with torch.no_grad():
            out = nearest.authenticity_of(E, real_u8, features.sample_u8(G, 64, 500, TP.EVAL_SEED))
        assert line == nearest.csv_line(step, out), (line, out)
    assert len(TP._csv_rows(hooked)) == 2                             # the PRDC rows are written as ever


# ---- leave-one-out kNN ----
def test_leave_one_out_classifier_against_float64(margin):
    from contrad_amd import knn
    n, d, C, k, temp = 70, 24, 5, 20, 0.1
    r = np.random.RandomState(0)
    y = r.randint(0, C, n).astype(np.int64)
    bank = r.randn(C, d)[y] + r.randn(n, d)
    S = knn_ref64.normalize64(bank) @ knn_ref64.normalize64(bank).T
    r_idx, r_val, r_sc, r_pred = R.select_and_vote_loo(S, y, C, k, 1.0 / temp, 0)
    masked = S.copy()
    np.fill_diagonal(masked, -np.inf)                                  # the guard rule looks at the candidates only
    out = knn_ref64.fragile_rows(masked, r_sc, k)
    assert out.sum() <= 0.1 * n, int(out.sum())
    bank_dev = torch.from_numpy(bank).float().cuda()
    clf = knn.KNNClassifier(bank_dev, y, C, k=k, temp=temp)
    clf.chunk_rows = 16                                               # five chunks: self0 = 0, 16, 32, 48, 64
    pred, scores, idx, val = (t.cpu().numpy() for t in clf.predict(bank_dev, neighbours=True, leave_self_out=True))
    assert all(i not in row for i, row in enumerate(idx.tolist()))
    keep = ~out
    assert all(set(a) == set(b) for a, b in zip(idx[keep].tolist(), r_idx[keep].tolist()))
    assert np.array_equal(pred[keep], r_pred[keep])
    margin('knn loo classifier scores', TK._score_error(scores[keep], r_sc[keep]), ((k + 32) + (2 * d + 8) / temp) * EPS)
    whole = knn.KNNClassifier(bank_dev, y, C, k=500, temp=temp)
    assert whole.k == 70 and whole.predict(bank_dev, neighbours=True, leave_self_out=True)[2].shape == (70, 69)      # k clamped to n - 1
    with pytest.raises(ValueError):
        clf.predict(bank_dev[:69], leave_self_out=True)


def test_loo_accuracy_and_the_command_line(tmp_path):
    import test_knn
    from contrad_amd import features, knn, lineval
    D = TP._encoder(4)[1]
    torch.save(D.state_dict(), str(tmp_path / 'dis.pt'))
    path = test_knn.main([str(tmp_path / 'dis.pt'), 'sndcgan', '--n_classes', '4', '--synthetic', '--synthetic_size', '64', '16',
                          '--seed', '3', '--batch_size', '50', '--k', '20', '--loo'])
    with open(path) as f:
        out = json.load(f)
    assert set(out) == {'acc@1', 'n_test', 'k', 'temp', 'n_train', 'loo'} and set(out['loo']) == {'acc@1', 'n', 'k'}
    assert (out['loo']['n'], out['loo']['k']) == (64, 20) and 0.0 <= out['loo']['acc@1'] <= 100.0
    data = lineval.synthetic_set(3, 4, 64, 16)
    D = features.freeze(D.cuda())
    x = torch.from_numpy(data['x_train']).cuda()
    with torch.no_grad():
        got = knn.loo_accuracy(D, x, data['y_train'], 4, k=20, batch=50)
        feats = features.extract_features(D, x, 50)
    pred = knn.KNNClassifier(feats, data['y_train'], 4, k=20, normalize=False).predict(feats, leave_self_out=True)[0].cpu().numpy()
    assert got == out['loo'] and got['acc@1'] == 100.0 * int((pred == data['y_train']).sum()) / 64
    assert knn.loo_accuracy(D, x, data['y_train'], 4, k=500)['k'] == 63
    with pytest.raises(ValueError):
        knn.loo_accuracy(D, x[:1], data['y_train'][:1], 4)
