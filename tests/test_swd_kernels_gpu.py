"""The sliced Wasserstein distance on the GPU against the yardstick (tests/swd_ref64.py): every kernel of csrc/eval/swd.hip
alone, ``swd_of`` end to end, the command line and the training hook.  Outputs sit in guard storage (NaN outside).

Bounds (derived, not measured; tests/swd_ref64.py's docstring).  Pyramid: elementwise gamma_25 on the stencil's absolute sums
plus the propagated error of the level above (``pyramid_bounds``); the uint8 level is exact, and so are G_1, G_2 and L_0 of a
uint8 set (their bound is 0 and they are compared for equality).  Gather: bitwise against numpy
indexing; the channel sums within n_terms 2^-53 sum |terms| of ``math.fsum``.  Sort: equal to ``np.sort`` of the same fp32 row,
bitwise wherever the value is not a zero.  Abs-diff: within n 2^-53 sum |terms| of ``math.fsum``.  End to end: sorting is
1-Lipschitz in the sup norm, so a level moves by at most the two sets' projection errors (``projection_bound``, the pyramid
bound carried through gamma_148) times 1e3.  Every figure goes through ``margin`` (conftest.py), which keeps the observed
error next to the bound.

Observed on the MI355X (profiles/swd.txt): every pyramid level whose bound is 0 exact, the others at most 0.15 of their bound;
channel sums within 7.5e-9 (bounds from 6.5e-5); abs-diff within 5.8e-11 (bound 2.1e-6); ``swd_of`` within 7.4e-7 / 4.8e-6 of
float64 at levels 32 / 16."""
import json
import os

import numpy as np
import pytest
import torch

import swd_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NAN = float('nan')


def _guarded(shape, dtype=torch.float32):
    """(view, check): a contiguous tensor of ``shape`` inside NaN guard bands; ``check()`` asserts the bands are untouched."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), NAN, device='cuda', dtype=dtype)

    def check():
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + numel:]).all())
    return flat[GUARD:GUARD + numel].view(*shape), check


def _planes(x):
    """[n, R, R, 3] -> [n * 3, R, R]."""
    n, Rr = x.shape[0], x.shape[1]
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))).reshape(n * 3, Rr, Rr)


def _nhwc(p):
    n3, Rr = p.shape[0], p.shape[1]
    return np.transpose(p.reshape(n3 // 3, 3, Rr, Rr), (0, 2, 3, 1))


# ---- pyramid ----
def _device_pyramid(x_u8, n_levels):
    from contrad_amd import ops
    n, size = x_u8.shape[0], x_u8.shape[1]
    checks, pyr = [], []
    lv, c = _guarded((n * 3, size, size))
    checks.append(c)
    pyr.append(ops.swd_u8_planes(torch.from_numpy(x_u8).cuda(), out=lv))
    for i in range(1, n_levels):
        lv, c = _guarded((n * 3, size >> i, size >> i))
        checks.append(c)
        pyr.append(ops.swd_pyr_down(pyr[i - 1], out=lv))
        ops.swd_pyr_up_sub(pyr[i - 1], pyr[i])
    torch.cuda.synchronize()
    for c in checks:
        c()
    return [_nhwc(p.cpu().numpy()) for p in pyr]


def _ratio(err, bound):
    """max err / bound; an element whose bound is 0 must be exact."""
    assert np.all(err[bound == 0] == 0)
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize('n,size,kind', [(3, 32, 'smooth'), (3, 32, 'noise'), (1, 64, 'smooth'), (1, 64, 'noise'),
                                         (1, 128, 'noise')])        # (128: the first size whose last level rounds in `down`)
def test_pyramid_against_float64(margin, n, size, kind):
    n_levels = len(R.levels_of(size))
    x = R.smooth_noise(n, size, 1) if kind == 'smooth' else np.random.RandomState(2).randint(0, 256, (n, size, size, 3)).astype(np.uint8)
    x[0, 0, 0] = 255; x[0, -1, -1] = 0; x[0, 0, -1] = 255; x[0, -1, 0] = 0         # the corners carry weight
    ref, bounds = R.pyramid(x, n_levels), R.pyramid_bounds(x, n_levels)
    got = _device_pyramid(x, n_levels)
    for i, (g, r, b) in enumerate(zip(got, ref, bounds)):
        assert g.shape == r.shape
        err = np.abs(g.astype(np.float64) - r)
        margin('swd pyramid %dx%d %s level %d' % (n, size, kind, i), _ratio(err, b), 1.0)
        edge = np.zeros(r.shape, bool)                               # the rows and columns the mirror rule feeds
        edge[:, :2] = edge[:, -2:] = True
        edge[:, :, :2] = edge[:, :, -2:] = True
        margin('swd pyramid %dx%d %s level %d mirror rows' % (n, size, kind, i), _ratio(err[edge], b[edge]), 1.0)
        assert np.abs(r[edge]).max() > 1.0                            # (they are not trivially small)


def test_u8_level_is_exact():
    from contrad_amd import ops
    x = np.random.RandomState(0).randint(0, 256, (5, 16, 16, 3)).astype(np.uint8)
    out, check = _guarded((15, 16, 16))
    ops.swd_u8_planes(torch.from_numpy(x).cuda(), out=out)
    check()
    assert np.array_equal(out.cpu().numpy(), _planes(x.astype(np.float32)))


# ---- gather ----
def _gather_inputs(n, size, nhoods):
    """(level, pos) on the host and (planes, cx, cy) on the device.  (Shared with tests/test_workspace_contract_gpu.py.)"""
    r = np.random.RandomState(n)
    level = (r.randn(n, size, size, 3) * 40 + 7).astype(np.float32)
    n_desc = n * nhoods
    pos = r.randint(3, size - 3, (n_desc, 2)).astype(np.int32)
    pos[:4] = [(3, 3), (3, size - 4), (size - 4, 3), (size - 4, size - 4)]           # all four extreme centres
    pos[-1] = (size - 4, size - 4)
    dev_level = torch.from_numpy(_planes(level)).cuda()
    cx, cy = torch.from_numpy(pos[:, 0].copy()).cuda(), torch.from_numpy(pos[:, 1].copy()).cuda()
    return level, pos, dev_level, cx, cy


@pytest.mark.parametrize('n,size,nhoods', [(3, 16, 5), (24, 32, 16), (2, 64, 300)])
def test_gather_bitwise_and_channel_sums(margin, n, size, nhoods):
    from contrad_amd import ops
    level, pos, dev_level, cx, cy = _gather_inputs(n, size, nhoods)
    n_desc = n * nhoods
    n_pad = (n_desc + 3) // 4 * 4
    want = R.descriptors(level, pos, nhoods)                                           # float32 indexing: exact
    runs = []
    for _ in range(2):
        bank, cb = _guarded((148, n_pad))
        stats, cs = _guarded((6,), torch.float64)
        ops.swd_gather(dev_level, cx, cy, nhoods, bank=bank, stats=stats)
        torch.cuda.synchronize()
        cb(); cs()
        runs.append((bank.cpu().numpy(), stats.cpu().numpy()))
    bank, stats = runs[0]
    assert np.array_equal(bank[:147, :n_desc].view(np.uint32), np.ascontiguousarray(want.T).view(np.uint32))
    assert np.all(bank[147].view(np.uint32) == 0) and np.all(bank[:, n_desc:].view(np.uint32) == 0)
    assert np.array_equal(runs[1][0].view(np.uint32), bank.view(np.uint32))
    assert np.array_equal(runs[1][1].view(np.uint64), stats.view(np.uint64))           # two calls: bitwise equal
    d = want.astype(np.float64).reshape(n_desc, 3, 49)
    terms = n_desc * 49
    for c in range(3):
        v = d[:, c].ravel()
        margin('swd gather sum %dx%dx%d c%d' % (n, size, nhoods, c), abs(stats[c] - R.fsum(v)),
               R.fsum_bound(terms, R.fsum(np.abs(v))))
        margin('swd gather sumsq %dx%dx%d c%d' % (n, size, nhoods, c), abs(stats[3 + c] - R.fsum(v * v)),
               R.fsum_bound(terms, R.fsum(v * v)))


# ---- sort ----
def _sort_lengths():
    from contrad_amd import ops
    T = ops.swd_sort_tile()
    return [1, 2, 3, 1000, T, T + 1, 3 * T + 5, 2 ** 15 + 7]


def _sort_inputs(rows, n, seed):
    r = np.random.RandomState(seed)
    rand = r.randn(rows, n).astype(np.float32)
    zeros = rand.copy()
    zeros[:, ::3] = 0.0
    zeros[:, 1::6] = -0.0
    return {'random': rand, 'sorted': np.sort(rand, axis=1), 'reversed': np.sort(rand, axis=1)[:, ::-1].copy(),
            'four values': r.choice(np.array([-2.5, 0.25, 1.0, 7.0], np.float32), (rows, n)), 'zeros of both signs': zeros}


@pytest.mark.parametrize('rows', [1, 5, 128])
@pytest.mark.parametrize('which', range(8))
def test_sort_rows_against_numpy(rows, which):
    from contrad_amd import ops
    n = _sort_lengths()[which]
    ld = n + 3                                                         # ld > n, odd: no 16-byte alignment to lean on
    for name, x in _sort_inputs(rows, n, 7 * which + rows).items():
        host = np.full((rows, ld), 12345.0, np.float32)
        host[:, n:] = NAN                                              # the padding of a row is neither read nor written
        host[:, :n] = x
        outs = []
        for _ in range(2):
            flat = torch.full((rows * ld + 2 * GUARD,), NAN, device='cuda')
            view = flat[GUARD:GUARD + rows * ld].view(rows, ld)
            view.copy_(torch.from_numpy(host))
            ops.swd_sort_rows(view, n)
            outs.append(flat.cpu().numpy())
        full = outs[0]
        assert np.array_equal(outs[1].view(np.uint32), full.view(np.uint32)), name     # two calls: bitwise equal
        assert np.all(np.isnan(full[:GUARD])) and np.all(np.isnan(full[GUARD + rows * ld:])), name
        got = full[GUARD:GUARD + rows * ld].reshape(rows, ld)
        assert np.all(np.isnan(got[:, n:])), name
        want = np.sort(x, axis=1)
        assert np.array_equal(got[:, :n], want), name                  # (as values: -0.0 == 0.0)
        nz = want != 0
        assert np.array_equal(got[:, :n].view(np.uint32)[nz], want.view(np.uint32)[nz]), name
        if name == 'zeros of both signs':                              # the zeros are the input's, each sign as often
            assert np.array_equal(np.signbit(got[:, :n]).sum(axis=1), np.signbit(x).sum(axis=1))


def test_sort_refusals():
    from contrad_amd import ops
    x = torch.zeros(4, 16, device='cuda')
    for bad in (lambda: ops.swd_sort_rows(x, 17), lambda: ops.swd_sort_rows(x, 0), lambda: ops.swd_sort_rows(x.double(), 4),
                lambda: ops.swd_sort_rows(x.cpu(), 4), lambda: ops.swd_sort_rows(x[0], 4), lambda: ops.swd_sort_rows(x.t(), 2)):
        with pytest.raises(RuntimeError):
            bad()


def test_pyramid_and_gather_refusals():
    from contrad_amd import ops
    p = torch.zeros(6, 16, 16, device='cuda')
    c = torch.zeros(12, dtype=torch.int32, device='cuda')
    for bad in (lambda: ops.swd_u8_planes(p), lambda: ops.swd_u8_planes(torch.zeros(2, 16, 8, 3, dtype=torch.uint8, device='cuda')),
                lambda: ops.swd_u8_planes(torch.zeros(2, 16, 16, 3, dtype=torch.uint8)),
                lambda: ops.swd_u8_planes(torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device='cuda'), out=p[:3]),
                lambda: ops.swd_pyr_down(p[:5]), lambda: ops.swd_pyr_down(p[:, :, :8]), lambda: ops.swd_pyr_down(p.cpu()),
                lambda: ops.swd_pyr_down(torch.zeros(3, 15, 15, device='cuda')), lambda: ops.swd_pyr_down(p, out=p[:, :8, :8]),
                lambda: ops.swd_pyr_up_sub(p, p), lambda: ops.swd_pyr_up_sub(p, torch.zeros(3, 8, 8, device='cuda')),
                lambda: ops.swd_gather(p, c, c, 0), lambda: ops.swd_gather(p, c, c, 5), lambda: ops.swd_gather(p, c.long(), c, 6),
                lambda: ops.swd_gather(p, c.cpu(), c, 6), lambda: ops.swd_gather(p, None, c, 6),
                lambda: ops.swd_gather(torch.zeros(3, 6, 6, device='cuda'), c[:3], c[:3], 3),
                lambda: ops.swd_gather(p, c, c, 6, bank=torch.zeros(148, 16, device='cuda')),
                lambda: ops.swd_gather(p, c, c, 6, stats=torch.zeros(6, device='cuda'))):
        with pytest.raises(RuntimeError):
            bad()
    bank, stats = ops.swd_gather(p, c, c, 6)                           # centres outside [3, R - 4] are clamped, nothing faults
    assert tuple(bank.shape) == (148, 12) and not bool(bank.any()) and not bool(stats.any())


# ---- abs-diff ----
def _absdiff_inputs(rows, n):
    """(A, B, off) on the host and the two device operands.  (Shared with tests/test_workspace_contract_gpu.py.)"""
    r = np.random.RandomState(rows + n)
    A, B = r.randn(rows, n).astype(np.float32), r.randn(rows, n).astype(np.float32)
    off = r.randn(rows) * 0.1
    dev = []
    for M, pad in ((A, 5), (B, 2)):                                    # leading dimensions of their own, NaN behind column n
        t = torch.full((rows, n + pad), NAN, device='cuda')
        t[:, :n] = torch.from_numpy(M).cuda()
        dev.append(t)
    return A, B, off, dev


@pytest.mark.parametrize('rows,n', [(1, 1), (5, 4096), (5, 4097), (3, 10007), (128, 999)])
def test_absdiff_against_fsum(margin, rows, n):
    from contrad_amd import ops
    A, B, off, dev = _absdiff_inputs(rows, n)
    for o in (None, off):
        terms = R.absdiff_terms(A, B, o)
        ref, bound = R.fsum(terms), R.fsum_bound(rows * n + 1, R.fsum(terms))
        o_dev = None if o is None else torch.from_numpy(o).cuda()
        buf = torch.full((3,), NAN, device='cuda', dtype=torch.float64)
        out = ops.swd_absdiff_sums(dev[0], dev[1], n, row_offset=o_dev, out=buf[1:2])
        first = buf.cpu().numpy().copy()
        assert np.isnan(first[0]) and np.isnan(first[2])
        margin('swd absdiff %dx%d off=%s' % (rows, n, o is not None), abs(first[1] - ref), bound if ref else 1e-300)
        again = ops.swd_absdiff_sums(dev[0], dev[1], n, row_offset=o_dev)
        assert again.cpu().numpy().view(np.uint64)[0] == first.view(np.uint64)[1]     # two calls: bitwise equal
        ops.swd_absdiff_sums(dev[0], dev[1], n, row_offset=o_dev, out=out, accumulate=True)
        margin('swd absdiff accumulate %dx%d off=%s' % (rows, n, o is not None), abs(float(buf[1]) - 2 * ref), 2 * bound if ref else 1e-300)
    with pytest.raises(RuntimeError):
        ops.swd_absdiff_sums(dev[0], dev[1], n, accumulate=True)
    with pytest.raises(RuntimeError):
        ops.swd_absdiff_sums(dev[0], dev[1][:, :n - 1] if n > 1 else dev[1][:0], n)


# ---- end to end ----
def _level_bound(x, fake, D, nhoods):
    """Per level: 1e3 x (the projection bound of the real set + that of the fake set)."""
    out = []
    br, bf = R.pyramid_bounds(x, len(D)), R.pyramid_bounds(fake, len(D))
    pr, pf = R.pyramid(x, len(D)), R.pyramid(fake, len(D))
    for i, lv in enumerate(D):
        a = R.projection_bound(R.descriptors(pr[i], lv['real'], nhoods), lv['dirs'], br[i].max())
        b = R.projection_bound(R.descriptors(pf[i], lv['fake'], nhoods), lv['dirs'], bf[i].max())
        out.append(1e3 * (a + b) * (1 + 1e-9))                         # (1e-9: the float64 sum of |A - B| and the division)
    return out


def test_swd_of_against_the_yardstick(margin):
    from contrad_amd import swd
    n, nhoods = 24, 16
    x = R.smooth_noise(2 * n, 32, 3)
    a, b = x[:n], x[n:]
    D = swd.draws(9, n, [32, 16], nhoods)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = swd.swd_of(da, db, seed=9, nhoods=nhoods, draws=D)
    ref, ref_avg = R.swd(a, b, D, nhoods)
    assert out['levels'] == [32, 16] and out['n'] == n and out['nhoods'] == nhoods
    assert (out['dir_repeats'], out['dirs_per_repeat'], out['seed']) == (4, 128, 9)
    for res, got, want, bound in zip(out['levels'], out['swd'], ref, _level_bound(a, b, D, nhoods)):
        print('level %d: device %.9f yardstick %.9f bound %.3e' % (res, got, want, bound))
        assert want > 1.0
        margin('swd_of level %d against float64' % res, abs(got - want), bound)
    assert abs(out['avg'] - ref_avg) <= max(_level_bound(a, b, D, nhoods))
    again = swd.swd_of(da, db, seed=9, nhoods=nhoods)                  # the default draws are draws(seed, ...): bitwise the same
    assert again['swd'] == out['swd'] and again['avg'] == out['avg']
    same = [dict(lv, fake=lv['real']) for lv in D]
    zero = swd.swd_of(da, da.clone(), seed=9, nhoods=nhoods, draws=same)
    assert zero['swd'] == [0.0, 0.0] and zero['avg'] == 0.0


def test_blur_shows_at_the_finest_level():
    from contrad_amd import swd
    x = R.smooth_noise(128, 32, 5)
    a, b = x[:64], x[64:]
    da = torch.from_numpy(a).cuda()
    splits = swd.swd_of(da, torch.from_numpy(b).cuda(), seed=5, nhoods=32)['swd']
    blur = swd.swd_of(da, torch.from_numpy(R.blurred(b)).cuda(), seed=5, nhoods=32)['swd']
    print('splits %s blurred %s' % (splits, blur))
    assert blur[0] >= 1.5 * splits[0]


def test_swd_of_refusals():
    from contrad_amd import swd
    def u8(*shape):
        return torch.randint(0, 256, shape, device='cuda', dtype=torch.uint8)
    ok = u8(4, 32, 32, 3)
    for bad in ((ok.float(), ok), (ok, ok.cpu()), (ok[..., :2], ok), (ok[0], ok)):
        with pytest.raises(RuntimeError):
            swd.swd_of(*bad)
    for bad in ((u8(4, 32, 16, 3),) * 2, (u8(4, 24, 24, 3),) * 2, (u8(4, 8, 8, 3),) * 2, (ok, u8(5, 32, 32, 3)), (ok, u8(4, 16, 16, 3)),
                (ok[:0], ok[:0])):
        with pytest.raises(ValueError):
            swd.swd_of(*bad)
    with pytest.raises(ValueError):
        swd.swd_of(ok, ok, nhoods=0)
    flat = ok.clone()
    flat[..., 1] = 7                                                   # a channel without variance
    with pytest.raises(ValueError, match='no variance'):
        swd.swd_of(ok, flat, nhoods=4, dir_repeats=1, dirs_per_repeat=8)


# ---- the command line and the training hook ----
def test_command_line_writes_the_json(tmp_path):
    import test_prdc_gpu as TP
    import test_swd
    from contrad_amd import features, swd
    x = R.smooth_noise(80, 32, 11)
    np.savez(str(tmp_path / 'real.npz'), x_train=x[:48])
    os.makedirs(str(tmp_path / 'samples'))
    np.savez(str(tmp_path / 'samples' / 'samples.npz'), images=x[40:])
    small = ['--nhoods', '8', '--dir_repeats', '2', '--dirs', '16']
    path = test_swd.main(['--real', str(tmp_path / 'real.npz'), '--fake', str(tmp_path / 'samples' / 'samples.npz'), '--seed', '3'] + small)
    assert path == str(tmp_path / 'samples' / 'swd_3.json')
    with open(path) as f:
        out = json.load(f)
    assert out['n'] == 40 and out['levels'] == [32, 16] and len(out['swd']) == 2 and out['seed'] == 3
    want = swd.swd_of(torch.from_numpy(x[:40]).cuda(), torch.from_numpy(x[40:]).cuda(), seed=3, nhoods=8, dir_repeats=2, dirs_per_repeat=16)
    assert out == want and all(v > 0 for v in out['swd']) and out['avg'] == float(np.mean(out['swd']))
    G = TP._encoder(6)[0]
    os.makedirs(str(tmp_path / 'run'))
    torch.save(G.state_dict(), str(tmp_path / 'run' / 'gen.pt'))
    path = test_swd.main(['--real', str(tmp_path / 'real.npz'), '--gen', str(tmp_path / 'run' / 'gen.pt'), '--gen_arch', 'sndcgan',
                          '--n', '32', '--seed', '4', '--batch_size', '20'] + small)
    assert path == str(tmp_path / 'run' / 'swd_4.json')
    with open(path) as f:
        out = json.load(f)
    Gd = features.load_frozen(TP._encoder(6)[0], str(tmp_path / 'run' / 'gen.pt'), torch.device('cuda', 0))
    want = swd.swd_of(torch.from_numpy(x[:32]).cuda(), features.sample_u8(Gd, 32, 20, 4), seed=4, nhoods=8, dir_repeats=2, dirs_per_repeat=16)
    assert out == want and out['n'] == 32
    for bad in (['--n', '41'], ['--n', '0'], ['--nhoods', '0'], ['--batch_size', '0']):
        with pytest.raises(ValueError):
            test_swd.main(['--real', str(tmp_path / 'real.npz'), '--fake', str(tmp_path / 'samples' / 'samples.npz')] + bad)


def test_hook_appends_the_rows_and_leaves_the_checkpoints_bitwise_alone(tmp_path_factory):
    import test_prdc_gpu as TP
    from contrad_amd import features, swd
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_gan import main
    plain = TP._run(tmp_path_factory, False, False)
    d = tmp_path_factory.mktemp('swd_files')
    x = R.smooth_noise(64, 32, 13)
    np.savez(str(d / 'real.npz'), x_train=x)
    hooked = str(tmp_path_factory.mktemp('swd_run'))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', hooked, '--swd_data', str(d / 'real.npz'), '--swd_n', '48'])
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    assert not [f for f in os.listdir(plain) if f.startswith('swd_')]
    assert sorted(f for f in os.listdir(hooked) if f.endswith('.csv')) == ['swd_%d.csv' % TP.EVAL_SEED]
    with open(os.path.join(hooked, 'swd_%d.csv' % TP.EVAL_SEED)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,swd_32,swd_16,swd_avg' and len(lines) == 3
    dev = torch.device('cuda', 0)
    real = torch.from_numpy(x[:48]).to(dev)
    for line, (step, name) in zip(lines[1:], ((2, 'gen_2.pt'), (4, 'gen.pt'))):
        G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, name), dev)
        out = swd.swd_of(real, features.sample_u8(G, 48, 500, TP.EVAL_SEED), seed=TP.EVAL_SEED)
        assert line == swd.csv_line(step, out), (line, out)
    with pytest.raises(ValueError):
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', hooked, '--swd_n', '8'])
