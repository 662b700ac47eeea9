"""The yardstick of the radial power spectrum (tests/spectrum_ref64.py) against closed forms, the host side of
contrad_amd/spectrum.py (bin table, twiddles, refusals, parser, hook flags) against the yardstick.  No GPU."""
import argparse
import math

import numpy as np
import pytest
import torch

import spectrum_ref64 as R
from contrad_amd import spectrum


@pytest.mark.parametrize('S', R.SIDES)
def test_bin_table_against_the_yardsticks_own_binning(S):
    table, K, counts = spectrum.bin_table(S)
    full, Kr, counts_r = R.bins(S)
    assert table.dtype == np.int32 and table.shape == (S, S // 2 + 1) and table.flags['C_CONTIGUOUS']
    assert K == Kr == R.KMAX[S] + 1 and int(table[S // 2, S // 2]) == R.KMAX[S]
    assert np.array_equal(table, full[:, :S // 2 + 1])
    assert np.array_equal(counts, counts_r) and counts.sum() == S * S and counts.min() >= 1
    assert list(counts[:4]) == [1, 8, 12, 16]
    assert np.array_equal(table[1:], table[1:][::-1])                        # u -> S - u
    assert np.array_equal(full, full.T) and np.array_equal(full[:, 1:], full[:, 1:][:, ::-1])
    half = table[:S // 2 + 1]                                                # what the radial kernel's walk leans on
    assert np.all(np.diff(half, axis=1) >= 0) and np.all(np.diff(half, axis=0) >= 0) and np.all(half[:, 0] == np.arange(S // 2 + 1))
    assert spectrum.bin_table(S)[0] is table                                 # cached


def test_bins_are_the_rounded_radius_in_integers():
    full = R.bins(64)[0]
    for (u, v) in ((0, 0), (0, 1), (1, 1), (3, 4), (32, 32), (7, 7), (63, 1), (40, 50)):
        fu, fv = (u if u <= 32 else u - 64), (v if v <= 32 else v - 64)
        k, r4 = int(full[u, v]), 4 * (fu * fu + fv * fv)
        assert k == 0 if r4 == 0 else (2 * k - 1) ** 2 <= r4 < (2 * k + 1) ** 2
        assert k == int(round(math.sqrt(fu * fu + fv * fv)))                 # (no tie can occur: 4 r2 is even, the bounds odd)


@pytest.mark.parametrize('S', R.SIDES)
def test_twiddles(S):
    t = spectrum.twiddles(S)
    assert t.dtype == np.float32 and t.shape == (S // 2, 2)
    a = 2 * np.pi * np.arange(S // 2) / S
    want = np.stack([np.cos(a), -np.sin(a)], axis=1)
    assert np.all(np.abs(t - want) <= 2.0 ** -24)                            # one fp32 rounding of values in [-1, 1]
    assert tuple(t[0]) == (1.0, 0.0) and tuple(t[S // 4]) == (0.0, -1.0)


def test_rounding_chain_is_under_the_cap():
    assert [R.rounding_chain(S) for S in R.SIDES] == [38, 53, 68, 83, 98, 113]
    assert all(R.rounding_chain(S) <= 2 * S + 8 for S in R.SIDES)


@pytest.mark.parametrize('S', (16, 64))
def test_parseval_and_dc(S):
    x = R.uniform_noise(3, S, S)
    s = R.spectrum(x)
    Y = R.luma(x)
    F = np.fft.fft2(Y, axes=(1, 2))
    P = (F.real ** 2 + F.imag ** 2) / float(S) ** 4
    xi = x.astype(np.int64)
    num = 77 * xi[..., 0] + 150 * xi[..., 1] + 29 * xi[..., 2]                           # 256 Y, integers
    for i in range(3):
        want = int((num[i] ** 2).sum())
        assert abs(P[i].sum() * S * S * 65536.0 - want) <= 1e-10 * want                 # sum P S^2 = sum Y^2
        assert abs(s['profiles'][i, 0] - Y[i].mean() ** 2) <= 1e-12 * Y[i].mean() ** 2  # P[0, 0] is the squared mean
    counts = R.bins(S)[2]
    assert np.allclose((s['profiles'] * counts).sum(axis=1), P.sum(axis=(1, 2)), rtol=1e-12)
    assert np.allclose(s['map'], P.mean(axis=0)[:, :S // 2 + 1])


def test_closed_forms_of_the_yardstick():
    S = 16
    x = np.zeros((4, S, S, 3), np.uint8)
    x[0, 3, 5] = 255                                                         # one pixel
    x[1] = 200                                                               # constant
    x[2, :, 1::2] = 255                                                      # columns alternate along x
    x[3, 1::2, :] = 255                                                      # rows alternate along y
    F = R.rfft2(x)
    assert np.allclose(np.abs(F[0]), 255.0)
    assert abs(F[1][0, 0] - 200.0 * S * S) < 1e-9 and np.abs(F[1]).sum() - abs(F[1][0, 0]) < 1e-9
    on = np.zeros((S, S // 2 + 1), bool)
    on[0, 0] = on[0, S // 2] = True
    assert np.all(np.abs(F[2][~on]) < 1e-9) and np.all(np.abs(F[2][on]) > 1.0)
    on[0, S // 2], on[S // 2, 0] = False, True
    assert np.all(np.abs(F[3][~on]) < 1e-9) and np.all(np.abs(F[3][on]) > 1.0)


def test_host_compare_against_the_yardstick():
    a, b = R.smooth_noise(12, 16, 1), R.smooth_noise(10, 16, 2)
    ra, rb = R.spectrum(a), R.spectrum(b)
    want = R.compare(ra, rb)
    got = spectrum.compare(ra, dict(rb, profiles=None))
    assert np.allclose(got['R'], want['R'], rtol=0, atol=1e-12) and abs(got['lsd_db'] - want['lsd_db']) < 1e-12
    assert abs(got['hf_db'] - want['hf_db']) < 1e-12 and np.allclose(got['nyquist_db'], want['nyquist_db'], rtol=0, atol=1e-12)
    assert abs(got['floor_db'] - R.floor_db(ra['profiles'])) < 1e-12 and (got['n_real'], got['n_fake']) == (12, 10)
    same = spectrum.compare(ra, ra)
    assert same['R'] == [0.0] * ra['K'] and same['lsd_db'] == 0.0 and same['hf_db'] == 0.0 and same['nyquist_db'] == [0.0] * 3
    dead = dict(rb, mean=rb['mean'].copy())
    dead['mean'][5] = 0.0
    with pytest.raises(ValueError, match='radial bin'):
        spectrum.compare(ra, dead)
    dead = dict(rb, map=rb['map'].copy())
    dead['map'][8, 8] = 0.0
    with pytest.raises(ValueError, match='Nyquist'):
        spectrum.compare(ra, dead)
    with pytest.raises(ValueError):
        spectrum.compare(ra, R.spectrum(R.smooth_noise(2, 32, 3)))
    assert spectrum.compare(dict(ra, profiles=ra['profiles'][:1]), rb)['floor_db'] is None


def test_the_monitors_compare_records_nan_where_compare_raises():
    ra, rb = R.spectrum(R.smooth_noise(6, 16, 1)), R.spectrum(R.smooth_noise(6, 16, 2))
    real = {k: ra[k] for k in ('S', 'n', 'K', 'mean', 'map')}
    real['floor_db'] = 0.5
    good = spectrum.compare_or_nan(real, rb)
    assert good == spectrum.compare(real, rb) and good['floor_db'] == 0.5
    dead = dict(rb, mean=rb['mean'].copy())
    dead['mean'][3] = 0.0
    out = spectrum.compare_or_nan(real, dead)
    assert np.isnan(out['lsd_db']) and np.isnan(out['hf_db']) and np.all(np.isnan(out['nyquist_db'])) and np.all(np.isnan(out['R']))
    assert (out['S'], out['K'], out['n_real'], out['n_fake'], out['floor_db']) == (16, ra['K'], 6, 6, 0.5)
    assert spectrum.csv_line(7, out) == '7,nan,nan,nan,nan,nan' and 'nan' in spectrum.log_line(7, out)
    with pytest.raises(ValueError):
        spectrum.compare_or_nan(real, R.spectrum(R.smooth_noise(2, 32, 3)))


def test_figure_layout():
    a, b = R.spectrum(R.smooth_noise(4, 16, 1)), R.spectrum(R.smooth_noise(4, 16, 2))
    full = spectrum.full_map(a['map'])
    Y = R.luma(R.smooth_noise(4, 16, 1))
    F = np.fft.fft2(Y, axes=(1, 2))
    assert np.allclose(full, np.fft.fftshift(((F.real ** 2 + F.imag ** 2) / 16.0 ** 4).mean(axis=0)))
    img = spectrum.figure(a['map'], b['map'])
    assert img.dtype == np.uint8 and img.shape == (16, 48, 3) and np.array_equal(img[..., 0], img[..., 2])
    assert img[8, 8, 0] == 255                                               # DC, the largest value, in the centre
    assert np.all(spectrum.figure(a['map'], a['map'])[:, 32:] == 128)


def test_host_refusals_need_no_device():
    for bad in (np.zeros((2, 16, 16, 3), np.uint8), torch.zeros(2, 16, 16, 3, dtype=torch.uint8), None):
        with pytest.raises(RuntimeError):
            spectrum.spectrum_of(bad)
    for S in (0, 8, 24, 48, 1024, 15):
        with pytest.raises(ValueError):
            spectrum.check_side(S)
        with pytest.raises(ValueError):
            spectrum.bin_table(S)
        with pytest.raises(ValueError):
            spectrum.twiddles(S)
    assert [spectrum.default_chunk(S) * S * (S // 2 + 1) * 8 <= 1 << 30 for S in R.SIDES] == [True] * 6
    assert spectrum.default_chunk(512) == 1020


def test_parser_errors(capsys):
    ok = ['--real', 'r.npz']
    for bad in (ok, ok + ['--fake', 'f.npz', '--gen', 'g.pt'], ok + ['--gen', 'g.pt'], ok + ['--fake', 'f.npz', '--gen_arch', 'sndcgan'],
                ['--fake', 'f.npz'], ok + ['--fake', 'f.npz', '--n_real', 'x']):
        with pytest.raises(SystemExit):
            spectrum.parse_args(bad)
    capsys.readouterr()
    P = spectrum.parse_args(ok + ['--fake', 'f.npz', '--n_real', '5', '--n_fake', '7', '--figure', '--seed', '3'])
    assert (P.n_real, P.n_fake, P.figure, P.seed, P.batch_size) == (5, 7, True, 3, 500)


def test_hook_flag_checks():
    parser = argparse.ArgumentParser()
    spectrum.add_hook_arguments(parser)
    H = spectrum.check_hook_arguments(parser.parse_args([]))
    assert H.spectrum_data is None and H.spectrum_n == 8192
    H = spectrum.check_hook_arguments(parser.parse_args(['--spectrum_data', 'x.npz']))
    assert H.spectrum_data == 'x.npz' and H.spectrum_n == 8192
    assert spectrum.check_hook_arguments(parser.parse_args(['--spectrum_data', 'x.npz', '--spectrum_n', '9'])).spectrum_n == 9
    for bad in (['--spectrum_n', '8'], ['--spectrum_data', 'x.npz', '--spectrum_n', '0']):
        with pytest.raises(ValueError):
            spectrum.check_hook_arguments(parser.parse_args(bad))


def test_the_training_scripts_take_the_flags():
    """The parsers of the training scripts accept the spectrum hook's flags and its check hands them back -- and so for
    every hook the driver registers."""
    import hook_flags
    from contrad_amd import train_driver
    assert spectrum.HOOK in train_driver.HOOKS
    assert [hook.switch for hook in train_driver.HOOKS] == list(hook_flags.GIVEN)        # every registered hook is walked
    for name, parse in hook_flags.script_parsers().items():
        H = spectrum.check_hook_arguments(parse(hook_flags.MINIMAL + ['--spectrum_data', 'x.npz', '--spectrum_n', '9']))
        assert (H.spectrum_data, H.spectrum_n) == ('x.npz', 9), name
        for hook in train_driver.HOOKS:
            flags, want = hook_flags.GIVEN[hook.switch]
            P = parse(hook_flags.MINIMAL + flags)
            assert hook.on(P) and vars(hook.check(P)) == want, (name, hook.switch)
