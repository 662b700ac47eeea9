"""The sliced Wasserstein distance without a GPU: properties of the yardstick (tests/swd_ref64.py), the host side of
contrad_amd/swd.py (levels, draws, refusals, the hook's and the command line's flags) and -EINVAL from every entry point of
csrc/eval/swd.hip before any GPU call.

The property cases: 2 x 64 synthetic 32 x 32 images (uniform noise smoothed with sigma = 1, rescaled to 0 ... 255, floored),
nhoods = 32, seeds 5 to 8.  The same set under the same positions gives exactly 0.0 at both levels; a split against a
sigma = 1.5 blur of the other split must give at least 1.5 times what the two splits give at the finest level (a blur
removes what the finest Laplacian level holds).  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import swd_ref64 as R
from contrad_amd import swd

SEEDS = (5, 6, 7, 8)
N, SIZE, NHOODS = 64, 32, 32


def _sets(seed):
    x = R.smooth_noise(2 * N, SIZE, seed)
    return x[:N], x[N:]


@pytest.mark.parametrize('seed', SEEDS)
def test_yardstick_properties(seed):
    a, b = _sets(seed)
    D = swd.draws(seed, N, R.levels_of(SIZE), NHOODS)
    same = [dict(lv, fake=lv['real']) for lv in D]
    zero, zero_avg = R.swd(a, a, same, NHOODS)
    assert zero == [0.0, 0.0] and zero_avg == 0.0
    splits, _ = R.swd(a, b, D, NHOODS)
    blur, _ = R.swd(a, R.blurred(b), D, NHOODS)
    print('seed %d: splits %s blurred %s ratio at 32: %.3f' % (seed, splits, blur, blur[0] / splits[0]))
    assert all(np.isfinite(splits)) and all(v > 0 for v in splits)
    assert blur[0] >= 1.5 * splits[0]


def test_pyramid_reconstructs_and_the_mirror_rule():
    x = R.smooth_noise(2, 32, 0).astype(np.float64)
    pyr = R.pyramid(x, 2)
    assert np.abs(pyr[0] + R.up(pyr[1]) - x).max() < 1e-10
    ramp = np.tile(np.arange(8.0)[None, None, :, None], (1, 8, 1, 3))        # d c b | a b c d ...: column -1 reads column 1
    got = R.down(ramp)[0, 0, :, 0]
    assert abs(got[0] - (1 * 2 + 4 * 1 + 6 * 0 + 4 * 1 + 1 * 2) / 16.0) < 1e-12
    assert abs(got[3] - (1 * 4 + 4 * 5 + 6 * 6 + 4 * 7 + 1 * 6) / 16.0) < 1e-12      # column 8 reads column 6
    b = R.pyramid_bounds(x, 2)
    assert b[0].shape == x.shape and b[1].shape == (2, 16, 16, 3) and b[0].max() < 1e-3 and b[1].min() > 0


def test_levels():
    assert swd.levels_of(16) == [16] and swd.levels_of(32) == [32, 16]
    assert swd.levels_of(128) == [128, 64, 32, 16] and len(swd.levels_of(512)) == 6
    assert swd.levels_of(512) == R.levels_of(512)
    for bad in (8, 0, 24, 48, 100, -16):
        with pytest.raises(ValueError):
            swd.levels_of(bad)


def test_draws_order_and_ranges():
    n, nh, rep, m = 5, 3, 2, 7
    D = swd.draws(11, n, [32, 16], nh, rep, m)
    rs = np.random.RandomState(11)
    for lv, res in zip(D, (32, 16)):
        assert lv['res'] == res
        for what in ('real', 'fake'):                                # real positions, fake positions, ...
            want = rs.randint(3, res - 3, (n * nh, 2))
            assert lv[what].dtype == np.int32 and np.array_equal(lv[what], want)
            assert lv[what].min() >= 3 and lv[what].max() <= res - 4
        for r in range(rep):                                         # ... then the directions of each repeat
            d = rs.randn(147, m)
            assert np.array_equal(lv['dirs'][r], d / np.sqrt((d * d).sum(axis=0, keepdims=True)))
        assert np.abs(np.sqrt((lv['dirs'] ** 2).sum(axis=1)) - 1).max() < 1e-15
    big = swd.draws(0, 64, [16], 128, 1, 1)[0]                       # both ends of [3, res - 4] are drawn
    assert big['real'].min() == 3 and big['real'].max() == 12
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            swd.draws(0, bad[0], [16], *bad[1:])


def test_refusals_that_need_no_device():
    x = torch.zeros(4, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        swd.swd_of(x, x)                                             # not on the device
    with pytest.raises(RuntimeError):
        swd.swd_of(np.zeros((4, 32, 32, 3), np.uint8), x)
    D = swd.draws(0, 2, [32, 16], 4, 1, 8)
    swd.check_draws(D, 2, [32, 16], 4, 1, 8)
    for breakit in (lambda d: d.pop(), lambda d: d[0].__setitem__('res', 16),
                    lambda d: d[1].__setitem__('real', d[0]['real']),           # centres of the 32 level at the 16 level
                    lambda d: d[0].__setitem__('fake', d[0]['fake'][:-1]),
                    lambda d: d[0].__setitem__('dirs', d[0]['dirs'][:, :, :4])):
        bad = [dict(lv) for lv in D]
        breakit(bad)
        with pytest.raises(ValueError):
            swd.check_draws(bad, 2, [32, 16], 4, 1, 8)
    mu, sigma = swd.channel_stats([6.0, 12.0, 0.0, 20.0, 60.0, 0.0], 2)
    assert mu.tolist() == [3.0, 6.0, 0.0] and sigma.tolist() == [1.0, 0.0, 0.0]        # (a negative rounding residue is clipped)
    rows, shift = swd.projection_operands(np.ones((147, 2)), np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 4.0]))
    assert rows.shape == (2, 148) and rows.dtype == np.float32 and rows[0, 147] == 0 and rows[0, 0] == 1 and rows[1, 146] == 0.25
    assert shift.tolist() == [-49 * (1 + 1 + 0.75)] * 2


def test_hook_and_command_line_flags():
    from argparse import ArgumentParser, Namespace
    p = ArgumentParser()
    swd.add_hook_arguments(p)
    assert vars(p.parse_args([])) == {}                              # a run without the hook parses to what it did before
    H = swd.check_hook_arguments(p.parse_args([]))
    assert H.swd_data is None and H.swd_n == 8192
    H = swd.check_hook_arguments(p.parse_args(['--swd_data', 'a.npz', '--swd_n', '64']))
    assert H.swd_data == 'a.npz' and H.swd_n == 64
    with pytest.raises(ValueError):
        swd.check_hook_arguments(Namespace(swd_n=5))
    with pytest.raises(ValueError):
        swd.check_hook_arguments(Namespace(swd_data='a.npz', swd_n=0))
    P = swd.parse_args(['--real', 'r.npz', '--fake', 'f.npz'])
    assert (P.n, P.nhoods, P.dir_repeats, P.dirs, P.batch_size, P.seed, P.gen) == (None, 128, 4, 128, 500, None, None)
    P = swd.parse_args(['--real', 'r.npz', '--gen', 'g.pt', '--gen_arch', 'sndcgan', '--n', '9', '--seed', '3', '--dirs', '16'])
    assert (P.gen, P.gen_arch, P.n, P.seed, P.dirs) == ('g.pt', 'sndcgan', 9, 3, 16)
    for bad in (['--real', 'r.npz'], ['--fake', 'f.npz'], ['--real', 'r.npz', '--fake', 'f.npz', '--gen', 'g.pt'],
                ['--real', 'r.npz', '--gen', 'g.pt'], ['--real', 'r.npz', '--fake', 'f.npz', '--gen_arch', 'sndcgan']):
        with pytest.raises(SystemExit):
            swd.parse_args(bad)
    from contrad_amd.train_gan import parse_args as train_parse
    assert not hasattr(train_parse(['cfg.gin', 'sndcgan']), 'swd_data')
    assert train_parse(['cfg.gin', 'sndcgan', '--swd_data', 'a.npz']).swd_data == 'a.npz'
    assert swd.csv_head([32, 16]) == 'step,swd_32,swd_16,swd_avg'
    assert swd.csv_line(4, {'swd': [1.5, 2.25], 'avg': 1.875}) == '4,1.500000,2.250000,1.875000'


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    from contrad_amd import _lib
    __graft_entry__.build()
    return _lib.lib()


def test_entry_points_refuse_before_any_gpu_call(built):
    """-EINVAL (-22) without a device: null pointers and bad shapes never reach a launch."""
    buf = (ctypes.c_double * 64)()
    p, null, LL = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0), ctypes.c_longlong
    ip, inull = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(ctypes.c_int)()
    assert built.raw('contrad_swd_sort_tile')() in (4096, 8192, 16384, 32768)
    planes = built.raw('contrad_swd_u8_planes')
    assert planes(null, p, LL(1), 16, null) == -22 and planes(p, null, LL(1), 16, null) == -22
    assert planes(p, p, LL(0), 16, null) == -22 and planes(p, p, LL(1), 0, null) == -22
    for name in ('contrad_swd_pyr_down', 'contrad_swd_pyr_up_sub'):
        f = built.raw(name)
        q = ctypes.c_void_p(p.value + 256)
        assert f(null, q, LL(3), 16, null) == -22 and f(p, null, LL(3), 16, null) == -22 and f(p, p, LL(3), 16, null) == -22
        assert f(p, q, LL(0), 16, null) == -22 and f(p, q, LL(3), 15, null) == -22 and f(p, q, LL(3), 2, null) == -22
    wsq = built.raw('contrad_swd_gather_workspace_bytes')
    assert wsq(LL(0)) == -22 and wsq(LL(1)) == 48 and wsq(LL(256)) == 48 and wsq(LL(257)) == 96
    g = built.raw('contrad_swd_gather')
    ok = dict(level=p, n=LL(1), R=16, cx=ip, cy=ip, nhoods=4, bank=p, n_pad=LL(4), stats=p, ws=p, wsb=LL(48))
    for k, v in (('level', null), ('cx', inull), ('cy', inull), ('bank', null), ('stats', null), ('ws', null), ('n', LL(0)),
                 ('R', 6), ('nhoods', 0), ('n_pad', LL(5)), ('n_pad', LL(8)), ('wsb', LL(40)),
                 ('stats', ctypes.c_void_p(p.value + 4)), ('ws', ctypes.c_void_p(p.value + 4))):
        a = dict(ok, **{k: v})
        assert g(a['level'], a['n'], a['R'], a['cx'], a['cy'], a['nhoods'], a['bank'], a['n_pad'], a['stats'], a['ws'], a['wsb'],
                 null) == -22, k
    s = built.raw('contrad_swd_sort_rows')
    assert s(null, LL(8), 1, 8, null) == -22 and s(p, LL(8), 0, 8, null) == -22 and s(p, LL(8), 1, 0, null) == -22
    assert s(p, LL(7), 1, 8, null) == -22 and s(p, LL(1 << 31), 1, (1 << 30) + 1, null) == -22
    assert s(p, LL(1), 3, 1, null) == 0                              # one column: nothing to do, nothing launched
    aq = built.raw('contrad_swd_absdiff_workspace_bytes')
    assert aq(0, 5) == -22 and aq(5, 0) == -22 and aq(3, 4096) == 24 and aq(3, 4097) == 48
    ab = built.raw('contrad_swd_absdiff_sums')
    ok = dict(A=p, ldA=LL(8), B=p, ldB=LL(8), off=null, rows=2, n=8, out=p, ws=p, wsb=LL(16))
    for k, v in (('A', null), ('B', null), ('out', null), ('ws', null), ('rows', 0), ('n', 0), ('ldA', LL(7)), ('ldB', LL(7)),
                 ('wsb', LL(8)), ('out', ctypes.c_void_p(p.value + 4)), ('off', ctypes.c_void_p(p.value + 4)),
                 ('ws', ctypes.c_void_p(p.value + 4))):
        a = dict(ok, **{k: v})
        assert ab(a['A'], a['ldA'], a['B'], a['ldB'], a['off'], a['rows'], a['n'], 0, a['out'], a['ws'], a['wsb'], null) == -22, k
