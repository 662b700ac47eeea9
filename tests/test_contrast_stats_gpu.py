"""The contrastive diagnostics on the GPU against the yardstick (tests/contrast_ref64.py): ``contrad_gauss_sums`` alone on a
given S, ``contrast_stats`` on planted rows, ``contrast_of`` / ``ContrastMonitor`` through fixture discriminators, the
``--contrast_data`` hook of the training scripts and the command line.

Bounds (derived, not measured; tests/contrast_ref64.py).  On a given fp32 S the device sum must lie within
``2^-53 (sum term (t u + 5) + (M n + 16) sum term)`` of the ``math.fsum`` of the float64 terms (u exact, one rounding in
t u, 1 ulp each for the device's and the host's exp, the summation term of tests/kid_ref64.py).  On rows a device similarity
is within e = (2 d + 8) 2^-24 of the float64 one (tests/mmd_ref64.py's ``feature_bound``, tests/test_knn_gpu.py): alignment
has slope 2 in s, so |align - ref64| <= 2 e; a term exp(-t u) moves by the factor exp(+-2 t e), so does their mean, so
|uniform - ref64| <= 2 t e.  Ranks are compared row by row, rows with a competitor within 1e-5 of the positive left out (at
most 10 %).  NT-Xent: the 1e-3 relative tolerance of tests/test_contrast_gpu.py.  Every figure is printed before it is asserted.

Observed on the MI355X (profiles/contrast.txt): kernel on a given S |out - fsum| at most 1.42e-14 (on
a sum of 44.9, bound 6.7e-10) and at most 1.8e-3 of the bound anywhere (1.1e-16 on 0.43 at 5 x 257); on planted rows
|align - ref64| <= 1.1e-16 and |uniform - ref64| <= 2.3e-9 against bounds of 2.9e-6 and up, 0 - 1 rows left out, no other
row's rank differs, NT-Xent relative error <= 5.5e-8."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import contrast_ref64 as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NAN = float('nan')
EPS = 2.0 ** -24

# (M, n, ld, self0): scalar loads and a column-tile edge; 16-byte loads; two column tiles past 1024 with padding; own columns
# beyond the bank (nothing left out); the only small shape that takes the 32-rows-per-wave plan
SUM_SHAPES = [(1, 1, 1, -1), (1, 1, 1, 0), (5, 257, 257, 0), (65, 300, 300, 3), (130, 1030, 1032, 0), (6, 37, 40, 35), (131072, 1, 4, -1)]
TS = (0.0, 2.0, 10.0)
_SUM_REF = {}


def _bits(x):
    return np.float64(x).view(np.uint64)


def _excluded(M, n, self0):
    return [(i, self0 + i) for i in range(M) if 0 <= self0 + i < n] if self0 >= 0 else []


def _live_cell(M, n, self0):
    for i, j in ((M - 1, n - 1), (M // 2, n // 2), (0, 0), (0, n - 1)):
        if self0 < 0 or j != self0 + i:
            return i, j
    return None


def _sum_inputs(shape):
    """{(name, t): (S, fsum, bound)} for a shape, made once.  The excluded cells hold NaN in every S: they must never be seen."""
    if shape not in _SUM_REF:
        M, n, _, self0 = shape
        r = np.random.RandomState(0)
        data = {'random': r.uniform(-1, 1, (M, n)).astype(np.float32), 'clamp': np.full((M, n), 1 + 2.0 ** -23, np.float32),
                'minus': np.full((M, n), -1.0, np.float32)}
        cell = _live_cell(M, n, self0)
        if cell is not None:
            data['nan'] = data['random'].copy()
            data['nan'][cell] = NAN
        for S in data.values():
            for c in _excluded(M, n, self0):
                S[c] = NAN
        _SUM_REF[shape] = {(name, t): (S, C.gauss_block_sum(S, self0, t), C.gauss_block_bound(S, self0, t))
                           for name, S in data.items() for t in (TS if name == 'random' else (2.0,))}
    return _SUM_REF[shape]


def _device_S(S, ld, off):
    """S on the device in rows of ``ld`` floats, NaN behind every row (a padding column that is read shows); ``off``: the
    base pointer lies that many floats past a 16-byte boundary."""
    M, n = S.shape
    flat = torch.full((M * ld + 4,), NAN, device='cuda')
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + M * ld].view(M, ld)
    view[:, :n] = torch.from_numpy(S).cuda()
    assert view.data_ptr() % 16 == 4 * off
    return view


def _raw(view, M, n, self0, t, accumulate=False, out=None, row0=0):
    """contrad_gauss_sums on rows [row0, row0 + M) of ``view`` with guard bands around ``out`` and around a workspace of exactly
    the size the query names.  Returns (the float64 result, the guarded out buffer)."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    if out is None:
        out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    nbytes = lib().raw('contrad_kid_sums_workspace_bytes')(M, n)
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    rc = lib().raw('contrad_gauss_sums')(ops._p(view[row0:row0 + M]), ctypes.c_longlong(view.stride(0)), M, n, ctypes.c_longlong(self0), t,
                                         1 if accumulate else 0, ops._p(out[GUARD:]), ops._p(ws[GUARD:]), ctypes.c_longlong(nbytes),
                                         ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf in (out, ws):
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all()), 'guard band overwritten'
    return float(out[GUARD]), out


# ---- contrad_gauss_sums on a given S ----
@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'base+4B'])
@pytest.mark.parametrize('shape', SUM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gauss_sums_kernel_on_a_given_S(shape, off):
    M, n, ld, self0 = shape
    cells = M * n - len(_excluded(M, n, self0))
    worst = 0.0
    for (name, t), (S, ref, bound) in _sum_inputs(shape).items():
        tag = 'gauss sums %s %s t=%g base+%dB' % ('x'.join(map(str, shape)), name, t, 4 * off)
        view = _device_S(S, ld, off)
        got, _ = _raw(view, M, n, self0, t)
        print('%s: device %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (tag, got, ref, abs(got - ref), bound))
        if name == 'nan':
            assert math.isnan(got) and math.isnan(ref), tag + ': a NaN inside a live cell was lost'
            continue
        assert abs(got - ref) <= bound, tag
        worst = max(worst, abs(got - ref) / bound if bound > 0 else 0.0)
        if name == 'clamp' or t == 0.0:
            assert ref == float(cells) and got == ref, tag              # every term is exactly 1: the pair count
        if name == 'minus':
            assert abs(got - cells * math.exp(-8.0)) <= bound, tag
        if cells == 0:
            assert got == 0.0, tag                                      # the only cell is the one left out
        again, _ = _raw(view, M, n, self0, t)
        assert _bits(got) == _bits(again), tag + ': two calls differ'
    print('gauss sums %s base+%dB: largest |device - fsum| / bound %.3g' % ('x'.join(map(str, shape)), 4 * off, worst))


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'base+4B'])
def test_accumulate_over_two_row_chunks(off):
    shape = (130, 1030, 1032, 0)
    M, n, ld, self0 = shape
    S, ref, bound = _sum_inputs(shape)[('random', 2.0)]
    m1 = 67
    view = _device_S(S, ld, off)
    first, out = _raw(view, m1, n, self0, 2.0)
    assert abs(first - C.gauss_block_sum(S[:m1], self0, 2.0)) <= C.gauss_block_bound(S[:m1], self0, 2.0)
    both, _ = _raw(view, M - m1, n, self0 + m1, 2.0, accumulate=True, out=out, row0=m1)
    print('gauss sums %s base+%dB in chunks of %d + %d rows: %.17g  fsum %.17g  |diff| %.3g  bound %.3g'
          % ('x'.join(map(str, shape)), 4 * off, m1, M - m1, both, ref, abs(both - ref), bound))
    assert abs(both - ref) <= bound                                     # the whole-block reference, the whole-block bound
    out2 = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    _raw(view, m1, n, self0, 2.0, out=out2)
    again, _ = _raw(view, M - m1, n, self0 + m1, 2.0, accumulate=True, out=out2, row0=m1)
    assert _bits(both) == _bits(again)
    out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    out[GUARD] = 1e6                                                    # accumulate adds to what is there, and only then
    got, _ = _raw(view, M, n, self0, 2.0, accumulate=True, out=out)
    assert abs(got - (1e6 + ref)) <= bound + 2.0 ** -53 * (1e6 + ref)
    got, _ = _raw(view, M, n, self0, 2.0, accumulate=False, out=out)
    assert abs(got - ref) <= bound


def test_wrapper_equals_the_entry_point_and_checks_its_arguments():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    shape = (65, 300, 300, 3)
    M, n, ld, self0 = shape
    S = _sum_inputs(shape)[('random', 2.0)][0]
    view = _device_S(S, ld, 0)
    for t in TS:
        want, _ = _raw(view, M, n, self0, t)
        out = ops.gauss_sums(view, n, t, self0=self0)
        assert out.dtype == torch.float64 and tuple(out.shape) == (1,) and _bits(float(out)) == _bits(want)
    assert _bits(float(ops.gauss_sums(view, n, self0=self0))) == _bits(_raw(view, M, n, self0, 2.0)[0])      # t = 2 by default
    table = torch.zeros(2, 3, dtype=torch.float64, device='cuda')
    assert ops.gauss_sums(view[:33], n, self0=self0, out=table[1, 1:2]).data_ptr() == table[1, 1:2].data_ptr()
    ops.gauss_sums(view[33:], n, self0=self0 + 33, out=table[1, 1:2], accumulate=True)
    ref, bound = _sum_inputs(shape)[('random', 2.0)][1:]
    assert abs(float(table[1, 1]) - ref) <= bound and float(table.sum()) == float(table[1, 1])
    for bad in (dict(t=-1.0), dict(t=NAN), dict(t=float('inf')), dict(accumulate=True), dict(out=torch.zeros(1, device='cuda')),
                dict(out=torch.zeros(2, dtype=torch.float64, device='cuda')), dict(n=301)):
        a = dict(n=n); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.gauss_sums(view, **a)
    with pytest.raises(RuntimeError):
        ops.gauss_sums(view.double(), n)
    for kind in ('gauss', 2, 3):                                        # not a kind of mmd_sums
        with pytest.raises(RuntimeError):
            ops.mmd_sums(view, n, kind)
    # -EINVAL on device pointers, nothing written
    f, g, query = lib().raw('contrad_gauss_sums'), lib().raw('contrad_mmd_sums'), lib().raw('contrad_kid_sums_workspace_bytes')
    Z = torch.zeros(2, 8, device='cuda')
    out = torch.full((1,), -7.0, dtype=torch.float64, device='cuda')
    need = query(2, 8)
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device='cuda')
    for a in (dict(t=-1.0), dict(t=NAN), dict(t=float('inf')), dict(S=None), dict(out=None), dict(M=0), dict(n=0), dict(ldS=7), dict(ws=None),
              dict(ws_bytes=need - 1)):
        b = dict(S=Z, ldS=8, M=2, n=8, t=2.0, out=out, ws=ws, ws_bytes=need); b.update(a)
        assert f(ops._p(b['S']), ctypes.c_longlong(b['ldS']), b['M'], b['n'], ctypes.c_longlong(0), b['t'], 0, ops._p(b['out']),
                 ops._p(b['ws']), ctypes.c_longlong(b['ws_bytes']), ops._stream()) == -22, a
    for kind in (2, 3):
        assert g(ops._p(Z), ctypes.c_longlong(8), 2, 8, ctypes.c_longlong(0), kind, 1.0, 1.0, 0, ops._p(out), ops._p(ws),
                 ctypes.c_longlong(need), ops._stream()) == -22
    torch.cuda.synchronize()
    assert float(out) == -7.0 and bool((ws == -7.0).all())


# ---- contrast_stats on planted rows ----
STATS_CASES = [(d, n, batch) for d in (8, 16) for n, batch in ((96, 48), (260, 130), (100, 48))]
TEMP, T = 0.1, 2.0


def _device_ranks(pA, pB, batch):
    """The device's rank of every row, block by block (contrast.block_ranks on the rows contrast_stats sees)."""
    from contrad_amd import contrast
    return np.concatenate([contrast.block_ranks(torch.cat([pA[i:i + m], pB[i:i + m]]), m).cpu().numpy()
                           for i, m in C.blocks_of(pA.shape[0], batch)])


def _check_against_yardstick(tag, got, An, Bn, ranks_dev, batch, temp, t, d):
    """``got`` against the yardstick on float64 copies of the device's own normalised rows."""
    e = (2 * d + 8) * EPS
    A64, B64 = An.cpu().double().numpy(), Bn.cpu().double().numpy()
    rank, margin = C.ranks(A64, B64, batch)
    out = margin < 1e-5
    same = np.array_equal(ranks_dev[~out], rank[~out])
    ref_align, ref_uniform, ref_nt = C.alignment(A64, B64), C.uniformity(A64, t), C.nt_xent(A64, B64, batch, temp)
    print('%s: rows left out %d of %d, ranks of the others %s; acc@1 %.4f (float64 %.4f) rank_mean %.3f; |align - ref64| %.3g bound %.3g; '
          '|uniform - ref64| %.3g bound %.3g; nt_xent %.6f ref64 %.6f rel %.3g'
          % (tag, int(out.sum()), len(out), 'equal' if same else 'DIFFER', got['acc@1'], C.rank_stats(rank)['acc@1'], got['rank_mean'],
             abs(got['align'] - ref_align), 2 * e, abs(got['uniform'] - ref_uniform), 2 * t * e, got['nt_xent'], ref_nt,
             abs(got['nt_xent'] - ref_nt) / abs(ref_nt)))
    assert out.sum() <= 0.1 * len(out) and same
    agreed = np.where(out, ranks_dev, rank)                             # a left-out row counts as agreeing
    for key, want in C.rank_stats(agreed).items():
        assert abs(got[key] - want) <= 1e-12, key                       # the aggregates are those of the device's own ranks
    assert abs(got['align'] - ref_align) <= 2 * e and abs(got['uniform'] - ref_uniform) <= 2 * t * e
    assert abs(got['nt_xent'] - ref_nt) < 1e-3 * abs(ref_nt)
    return rank


@pytest.mark.parametrize('case', STATS_CASES, ids=lambda c: 'd%d-n%d-b%d' % c)
def test_contrast_stats_on_planted_rows(case):
    from contrad_amd import contrast, features
    d, n, batch = case
    A, B = C.planted_views(0, n, d)
    Ad, Bd = torch.from_numpy(A).float().cuda(), torch.from_numpy(B).float().cuda()
    got = contrast.contrast_stats(Ad, Bd, batch, TEMP, T, fA=Bd, fB=Ad)
    assert (got['n'], got['batch'], got['temp'], got['t'], got['chance']) == (n, batch, TEMP, T, 1.0 / (2 * batch - 2))
    An, Bn = features.normalize_rows(Ad), features.normalize_rows(Bd)
    rank = _check_against_yardstick('contrast stats d%d n%d batch%d' % case, got, An, Bn, _device_ranks(An, Bn, batch), batch, TEMP, T, d)
    assert 0.05 < C.rank_stats(rank)['acc@1'] < 0.6                     # the ranks are not trivial
    e = (2 * d + 8) * EPS                                               # the penultimate pair here: the same rows, swapped
    assert abs(got['align_pen'] - got['align']) <= 4 * e and abs(got['uniform_pen'] - C.uniformity(Bn.cpu().double().numpy(), T)) <= 2 * T * e
    assert contrast.contrast_stats(Ad, Bd, batch, TEMP, T, fA=Bd, fB=Ad) == got                    # two calls: the same dict
    plain = contrast.contrast_stats(An, Bn, batch, TEMP, T, normalize=False)
    assert 'align_pen' not in plain and all(plain[k] == got[k] for k in plain)


def test_closed_forms_on_the_device():
    from contrad_amd import contrast
    d, n, b = 8, 24, 12
    e = (2 * d + 8) * EPS
    A = torch.from_numpy(C.normalize64(np.random.default_rng(0).standard_normal((n, d)))).float().cuda()
    same = contrast.contrast_stats(A, A, b, TEMP, T)                     # identical views
    print('identical views: %s' % (same,))
    assert same['align'] <= 2 * e and (same['acc@1'], same['acc@5'], same['rank_mean']) == (1.0, 1.0, 0.0)
    ones = torch.zeros(n, d, device='cuda')
    ones[:, 0] = 1.0                                                    # all rows equal: every similarity is exactly 1
    flat = contrast.contrast_stats(ones, ones, b, TEMP, T)
    print('all rows equal: %s' % (flat,))
    assert flat['uniform'] == 0.0 and flat['align'] == 0.0 and (flat['acc@1'], flat['rank_mean']) == (0.0, 2.0 * b - 2)
    assert abs(flat['nt_xent'] - math.log(2 * b - 1.0)) < 1e-3 * math.log(2 * b - 1.0)
    anti = ones.clone()
    anti[n // 2:, 0] = -1.0                                             # two antipodal clusters
    m = n // 2
    for t in TS:
        got = contrast.contrast_stats(anti, -anti, n, TEMP, t)
        want = math.log((2 * m * (m - 1) + 2 * m * m * math.exp(-4.0 * t)) / (2 * m * (2 * m - 1.0)))
        print('antipodal clusters t=%g: uniform %.17g closed form %.17g; align %.17g' % (t, got['uniform'], want, got['align']))
        assert abs(got['uniform'] - want) <= 2 * t * e + 1e-15 and got['align'] == 4.0 and got['rank_mean'] == 2.0 * n - 2
        if t == 0.0:
            assert got['uniform'] == 0.0                                # t = 0: the exact pair count


# ---- contrast_of, the monitor, the hook and the command line ----
N_IMG, BATCH = 64, 32


def _fixture_D(arch, settle):
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(3)
    _, D = get_architecture(arch, (32, 32, 3))
    D = D.cuda()
    for p in D.parameters():
        p.requires_grad_(False)
    if settle:          # a few train-mode forwards run the power iterations any checkpoint has behind it (tests/test_knn_gpu.py)
        x = torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
        with torch.no_grad():
            for _ in range(settle):
                D.train()(x)
    return D.eval()


def _images(n=N_IMG, seed=3):
    from contrad_amd import lineval
    return lineval.synthetic_set(seed, 4, n, 1)['x_train']


@pytest.mark.parametrize('arch,settle', [('sndcgan', 0), ('snresnet18', 8)])
def test_contrast_of_and_the_monitor(arch, settle, tmp_path):
    from contrad_amd import contrast
    from contrad_amd.augment import NoAugment, SimCLRAugment
    from contrad_amd.evaluate.gan import eval_seed_of
    dev = torch.device('cuda', 0)
    D = _fixture_D(arch, settle)
    x = torch.from_numpy(_images()).to(dev)
    aug = SimCLRAugment(scale=(0.2, 1.0))
    torch.manual_seed(11); np.random.seed(11); torch.cuda.manual_seed(11)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev), np.random.get_state()[1].copy())
    got = contrast.contrast_of(D, x, aug, N_IMG, BATCH, TEMP, T, seed=7, fwd_batch=40)
    print('%s contrast_of: %s' % (arch, got))
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state(dev))
    assert np.array_equal(before[2], np.random.get_state()[1])          # the global streams are where they were
    assert (got['n'], got['batch'], got['chance']) == (N_IMG, BATCH, 1.0 / 62) and set(contrast.KEYS) <= set(got)
    assert all(math.isfinite(got[k]) for k in contrast.KEYS)
    assert 0.0 <= got['acc@1'] <= got['acc@5'] <= 1.0 and 0.0 <= got['rank_mean'] <= 2 * BATCH - 2
    assert 0.0 <= got['align'] <= 4.0 and -4.0 * T <= got['uniform'] <= 0.0 and 0.0 <= got['align_pen'] <= 4.0 and got['uniform_pen'] <= 0.0
    assert contrast.contrast_of(D, x, aug, N_IMG, BATCH, TEMP, T, seed=7, fwd_batch=40) == got       # the same views come back
    assert contrast.contrast_of(D, x, aug, N_IMG, BATCH, TEMP, T, seed=8, fwd_batch=40) != got       # ... and others under another seed
    none = contrast.contrast_of(D, x, NoAugment(), N_IMG, BATCH, TEMP, T, seed=7)
    d_proj = D.d_project
    print('%s identical views: %s' % (arch, none))
    assert none['align'] <= 2 * (2 * d_proj + 8) * EPS and none['align_pen'] <= 2 * (2 * D.d_penul + 8) * EPS      # align = 0 within the GEMM's e
    assert (none['acc@1'], none['rank_mean']) == (1.0, 0.0)             # an image's other view is itself: no other row reaches it
    for a, match in ((dict(n=1), 'at least 2 images'), (dict(batch=1), 'fewer than 2 images'), (dict(temp=0.0), 'temp must be positive'),
                     (dict(t=-1.0), 't must be finite'), (dict(n=66), 'asked for 66 images'), (dict(n=33), 'last block of 1 image')):
        kw = dict(n=N_IMG, batch=BATCH, temp=TEMP, t=T); kw.update(a)
        with pytest.raises(ValueError, match=match):
            contrast.contrast_of(D, x, aug, kw['n'], kw['batch'], kw['temp'], kw['t'])
    with pytest.raises(RuntimeError, match='eval mode'):
        contrast.contrast_of(D.train(), x, aug, N_IMG, BATCH, TEMP, T)
    D.eval()
    # the monitor: two updates with unchanged weights write equal rows; the global streams are unchanged across an update
    path = str(tmp_path / 'held_out.npz')
    np.savez(path, x_train=_images(80))
    mon = contrast.ContrastMonitor(str(tmp_path), arch, (32, 32, 3), dev, 5, path, n=N_IMG, t=T, aug=aug, batch=BATCH, temp=TEMP)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev), np.random.get_state()[1].copy())
    first, second = mon.update(2, D), mon.update(4, D)
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state(dev))
    assert np.array_equal(before[2], np.random.get_state()[1])
    with open(os.path.join(str(tmp_path), 'contrast_%d.csv' % eval_seed_of(5))) as f:
        lines = f.read().split()
    assert lines[0] == contrast.CSV_HEADER and len(lines) == 3
    assert lines[1].split(',', 1)[1] == lines[2].split(',', 1)[1] and [ln.split(',')[0] for ln in lines[1:]] == ['2', '4']
    assert first == second and lines[1] == contrast.csv_row(2, first)
    assert first == contrast.contrast_of(D, mon.x, aug, N_IMG, BATCH, TEMP, T, seed=eval_seed_of(5))   # the monitor's D holds D's weights
    assert not D.training and not mon.D.training
    with pytest.raises(ValueError, match='the discriminator takes'):
        contrast.ContrastMonitor(str(tmp_path), arch, (64, 64, 3), dev, 5, path, aug=aug, batch=BATCH, temp=TEMP)


def test_hook_leaves_the_checkpoints_bitwise_alone(tmp_path_factory, tmp_path):
    import test_knn_gpu as TK
    from contrad_amd import contrast
    from contrad_amd.evaluate.gan import eval_seed_of
    from contrad_amd.train_gan import main
    plain = TK._run(tmp_path_factory, False, False)
    data = str(tmp_path / 'held_out.npz')
    np.savez(data, x_train=_images(96, seed=1))
    logdir = str(tmp_path / 'run')
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
          '--seed', str(TK.SEED), '--logdir', logdir, '--contrast_data', data, '--contrast_n', '64'])
    rows = _hook_rows(logdir, TK.SEED, [2, 4], 1.0 / 126)               # blocks of the run's batch, 64
    for name in ('gen.pt', 'dis.pt', 'optim.pt'):                       # the trajectory did not move by a bit
        TK._same(torch.load(os.path.join(plain, name), map_location='cpu'), torch.load(os.path.join(logdir, name), map_location='cpu'))
    assert not [f for f in os.listdir(plain) if f.startswith('contrast_')]
    # the logged figures are the checkpoint's: contrast_of on the saved discriminator under the run's augmentation gives the last row
    from contrad_amd import features
    from contrad_amd.augment import get_augment
    from contrad_amd.models.gan import get_architecture
    dev = torch.device('cuda', 0)
    contrast.bind_augment_config(logdir)
    D = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[1], os.path.join(logdir, 'dis.pt'), dev)
    again = contrast.contrast_of(D, torch.from_numpy(_images(96, seed=1)).to(dev), get_augment(mode='simclr').to(dev), 64, 64, 0.1, 2.0,
                                 seed=eval_seed_of(TK.SEED))
    assert contrast.csv_row(4, again).split(',') == ['%d' % rows[-1][0]] + ['%.6f' % v for v in rows[-1][1:]]


def _hook_rows(logdir, seed, steps, chance):
    from contrad_amd import contrast
    from contrad_amd.evaluate.gan import eval_seed_of
    with open(os.path.join(logdir, 'contrast_%d.csv' % eval_seed_of(seed))) as f:
        lines = f.read().split()
    assert lines[0] == contrast.CSV_HEADER
    rows = [[float(v) for v in ln.split(',')] for ln in lines[1:]]
    print('contrast rows of %s: %s' % (logdir, rows))
    assert [r[0] for r in rows] == steps and all(math.isfinite(v) for r in rows for v in r)
    with open(os.path.join(logdir, 'log.txt')) as f:
        log = f.read()
    assert log.count('[NT-Xent ') == len(steps) and '[pos Acc@1 ' in log and 'chance %.4f' % chance in log
    return rows


def test_stylegan2_loop_with_the_hook_and_identical_views(tmp_path):
    """``--aug none`` (the default of ``--mode=std``): the two views are the image itself; the monitor still runs."""
    import test_knn_gpu as TK
    from contrad_amd import config
    from contrad_amd.train_stylegan2 import main
    data = str(tmp_path / 'held_out.npz')
    np.savez(data, x_train=_images(96, seed=1))
    logdir = str(tmp_path / 'run')
    main([os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
          '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
          '--seed', str(TK.SEED), '--logdir', logdir, '--contrast_data', data, '--contrast_n', '64', '--contrast_t', '3'])
    rows = _hook_rows(logdir, TK.SEED, [2], 1.0 / 14)
    assert rows[0][5] == 0.0 and rows[0][7] == 0.0                      # align and align_pen to the csv's six decimals


def test_command_line_writes_the_json(tmp_path):
    import shutil
    import test_contrast
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(4)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    torch.save(D.state_dict(), str(tmp_path / 'dis.pt'))
    path = test_contrast.main([str(tmp_path / 'dis.pt'), 'sndcgan', '--synthetic', '--n', '64', '--batch_size', '32', '--seed', '3'])
    assert path == str(tmp_path / 'contrast_3.json')
    with open(path) as f:
        out = json.load(f)
    print('command line: %s' % (out,))
    assert (out['n'], out['batch'], out['temp'], out['t'], out['aug'], out['chance'], out['seed']) == (64, 32, 0.1, 2.0, 'simclr', 1.0 / 62, 3)
    assert all(math.isfinite(out[k]) for k in ('nt_xent', 'acc@1', 'acc@5', 'rank_mean', 'align', 'uniform', 'align_pen', 'uniform_pen'))
    data = str(tmp_path / 'x.npz')
    np.savez(data, x_train=_images(70))
    shutil.copy(os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin'), str(tmp_path / 'c10_b64.gin'))
    with open(test_contrast.main([str(tmp_path / 'dis.pt'), 'sndcgan', '--data', data, '--aug', 'none', '--temp', '0.2', '--t', '3', '--seed', '4'])) as f:
        out = json.load(f)                                              # the block size is the run's: batch_size of the *.gin beside the checkpoint
    assert (out['n'], out['batch'], out['temp'], out['t'], out['aug'], out['acc@1']) == (70, 64, 0.2, 3.0, 'none', 1.0)
    assert out['align'] <= 2 * (2 * D.d_project + 8) * EPS               # identical views
    for bad, match in ((['--synthetic', '--n', '1'], 'at least 2'), (['--data', data, '--batch_size', '1'], 'fewer than 2 images'),
                       (['--data', data, '--batch_size', '69'], 'last block of 1 image'), (['--data', data, '--temp', '0'], 'temp must be positive'),
                       (['--data', data, '--t', '-1'], 't must be finite')):
        with pytest.raises(ValueError, match=match):
            test_contrast.main([str(tmp_path / 'dis.pt'), 'sndcgan'] + bad)
