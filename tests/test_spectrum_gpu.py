"""contrad_amd/spectrum.py on the GPU: ``spectrum_of`` + ``compare`` end to end against the yardstick (tests/spectrum_ref64.py)
under the propagated bound of its docstring, what the numbers do on seeded sets with a known defect, the refusals, the command
line and the training hook.

Observed on the MI355X (profiles/spectrum.txt): every R[k] and summary number of the uniform-noise sets lies within 0.003 of its
propagated bound."""
import json
import os

import numpy as np
import pytest
import torch

import spectrum_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _of(x, **kw):
    from contrad_amd import spectrum
    return spectrum.spectrum_of(torch.from_numpy(np.ascontiguousarray(x)).cuda(), **kw)


@pytest.mark.parametrize('n,S', [(24, 16), (24, 32), (8, 64), (3, 128)])
def test_spectrum_of_and_compare_against_the_yardstick(margin, n, S):
    from contrad_amd import spectrum
    a, b = R.uniform_noise(n, S, 3 * S), R.uniform_noise(n + 1, S, 3 * S + 1)            # (unequal counts are accepted)
    ra, rb = R.spectrum(a), R.spectrum(b)
    want, tol = R.compare(ra, rb), R.tolerances(ra, rb)
    assert float(tol['R'].max()) < 0.05 and tol['lsd_db'] < 0.05             # (the propagated bound is a tight one at these inputs)
    da, db = _of(a), _of(b, chunk=5)                                         # (one set in chunks that do not divide it)
    assert (da['S'], da['n'], da['K'], db['n']) == (S, n, R.KMAX[S] + 1, n + 1)
    assert tuple(da['profiles'].shape) == (n, da['K']) and da['profiles'].is_cuda and da['profiles'].dtype == torch.float64
    assert da['mean'].shape == (da['K'],) and da['map'].shape == (S, S // 2 + 1)
    got = spectrum.compare(da, db)
    for k in range(da['K']):
        margin('spectrum R[%d] %dx%d' % (k, n, S), abs(got['R'][k] - want['R'][k]), tol['R'][k])
    margin('spectrum lsd_db %dx%d' % (n, S), abs(got['lsd_db'] - want['lsd_db']), tol['lsd_db'])
    margin('spectrum hf_db %dx%d' % (n, S), abs(got['hf_db'] - want['hf_db']), tol['hf_db'])
    for i in range(3):
        margin('spectrum nyquist_db[%d] %dx%d' % (i, n, S), abs(got['nyquist_db'][i] - want['nyquist_db'][i]), tol['nyquist_db'][i])
    halves = R.spectrum(a[0::2]), R.spectrum(a[1::2])                        # floor_db: the same distance between the real halves
    margin('spectrum floor_db %dx%d' % (n, S), abs(got['floor_db'] - R.floor_db(ra['profiles'])), R.tolerances(*halves)['lsd_db'])
    assert (got['n_real'], got['n_fake']) == (n, n + 1)
    print('%dx%d: lsd %.6f (yardstick %.6f, bound %.2e) hf %.6f floor %.6f' % (n, S, got['lsd_db'], want['lsd_db'], tol['lsd_db'],
                                                                               got['hf_db'], got['floor_db']))


def test_known_defects_show_where_they_should():
    """Seeded smooth sets at (n, S) = (24, 32): real a, an independent draw b (the floor), b with a checkerboard of +6, b blurred
    with sigma 1.  On the CPU the yardstick gives lsd 0.33 / 10.3 / 8.8 dB, hf +0.1 / +4.5 / -9.3 dB and a diagonal Nyquist
    point of 0.0 / +48.9 / -5.8 dB; the thresholds below are the issue's, far inside those.  These figures belong to the
    yardstick's own generator (tests/spectrum_ref64.py: a noise field per channel, periodic filter, variance normalised over the
    set), whose luma has little in the high band but quantisation noise; sets whose channels share one noise field read a
    checkerboard of +6 at 31 ... 43 dB and lsd 5.4 ... 7.6 dB and the blur at hf -2.1 ... -2.9 dB.  Both are right for their sets."""
    from contrad_amd import spectrum
    a, b = R.smooth_noise(24, 32, 1), R.smooth_noise(24, 32, 2)
    da = _of(a)
    floor, check, blur = (spectrum.compare(da, _of(f)) for f in (b, R.checkerboarded(b), R.blurred(b)))
    print('floor %s\ncheckerboard %s\nblur %s' % tuple({k: v for k, v in o.items() if k != 'R'} for o in (floor, check, blur)))
    assert check['nyquist_db'][2] > 20 and check['lsd_db'] > 3
    assert blur['hf_db'] < -1
    assert floor['lsd_db'] < 1.5
    ra, rc = R.spectrum(a), R.spectrum(R.checkerboarded(b))
    ref, tol = R.compare(ra, rc), R.tolerances(ra, rc)
    assert abs(check['nyquist_db'][2] - ref['nyquist_db'][2]) <= tol['nyquist_db'][2] and abs(check['lsd_db'] - ref['lsd_db']) <= tol['lsd_db']


def test_identical_sets_and_dead_frequencies():
    from contrad_amd import spectrum
    a = R.smooth_noise(6, 16, 4)
    da = _of(a)
    same = spectrum.compare(da, _of(a.copy()))
    assert same['R'] == [0.0] * da['K'] and same['lsd_db'] == 0.0 and same['hf_db'] == 0.0 and same['nyquist_db'] == [0.0, 0.0, 0.0]
    const = np.full((4, 16, 16, 3), 77, np.uint8)
    dc = _of(const)
    assert dc['mean'][0] == 77.0 ** 2 and not dc['mean'][1:].any()           # a constant image has exactly no power off DC
    with pytest.raises(ValueError, match='without power'):
        spectrum.compare(da, dc)
    assert spectrum.compare(da, _of(a[:1]))['n_fake'] == 1                   # one image is a set
    assert spectrum.compare(_of(a[:1]), da)['floor_db'] is None


def test_spectrum_of_refusals():
    from contrad_amd import spectrum

    def u8(*shape):
        return torch.randint(0, 256, shape, device='cuda', dtype=torch.uint8)
    ok = u8(4, 32, 32, 3)
    for bad in (ok.float(), ok.cpu(), ok[..., :2], ok[0], None):
        with pytest.raises(RuntimeError):
            spectrum.spectrum_of(bad)
    for bad in (u8(4, 32, 16, 3), u8(4, 24, 24, 3), u8(4, 8, 8, 3), u8(1, 1024, 1024, 3), ok[:0]):
        with pytest.raises(ValueError):
            spectrum.spectrum_of(bad)
    with pytest.raises(ValueError):
        spectrum.spectrum_of(ok, chunk=0)
    out = spectrum.spectrum_of(ok.permute(0, 2, 1, 3))                       # (a view that is not contiguous is copied, not refused)
    assert out['n'] == 4 and np.all(np.isfinite(out['mean']))


# ---- the command line and the training hook ----
def test_command_line_writes_the_json_and_the_figure(tmp_path):
    import png_reader
    import test_spectrum
    from contrad_amd import spectrum
    x = R.smooth_noise(36, 32, 11)
    np.savez(str(tmp_path / 'real.npz'), x_train=x[:20])
    os.makedirs(str(tmp_path / 'samples'))
    np.savez(str(tmp_path / 'samples' / 'samples.npz'), images=R.checkerboarded(x[20:]))
    args = ['--real', str(tmp_path / 'real.npz'), '--fake', str(tmp_path / 'samples' / 'samples.npz')]
    path = test_spectrum.main(args + ['--seed', '3', '--n_real', '16', '--figure'])
    assert path == str(tmp_path / 'samples' / 'spectrum_3.json')
    with open(path) as f:
        out = json.load(f)
    assert sorted(out) == sorted(['S', 'K', 'n_real', 'n_fake', 'R', 'lsd_db', 'hf_db', 'nyquist_db', 'floor_db', 'seed', 'mean_real',
                                  'mean_fake'])
    assert (out['S'], out['K'], out['n_real'], out['n_fake'], out['seed']) == (32, 24, 16, 16, 3)
    assert len(out['R']) == len(out['mean_real']) == len(out['mean_fake']) == 24 and len(out['nyquist_db']) == 3
    sr, sf = _of(x[:16]), _of(R.checkerboarded(x[20:]))
    want = spectrum.compare(sr, sf)
    assert all(out[k] == want[k] for k in want) and out['mean_real'] == sr['mean'].tolist() and out['nyquist_db'][2] > 20
    img = png_reader.read_png(str(tmp_path / 'samples' / 'spectrum_3.png'))
    assert img.shape == (32, 96, 3) and np.array_equal(img, spectrum.figure(sr['map'], sf['map']))
    assert img[16, 16, 0] == 255 or img[16, 48, 0] == 255                    # DC in the centre of a panel
    assert not os.path.exists(str(tmp_path / 'samples' / 'spectrum_4.png'))
    test_spectrum.main(args + ['--seed', '4'])
    assert os.path.exists(str(tmp_path / 'samples' / 'spectrum_4.json')) and not os.path.exists(str(tmp_path / 'samples' / 'spectrum_4.png'))
    for bad in (['--n_real', '21'], ['--n_real', '0'], ['--n_fake', '17'], ['--n_fake', '0'], ['--batch_size', '0']):
        with pytest.raises(ValueError):
            test_spectrum.main(args + bad)


def test_command_line_samples_a_generator(tmp_path):
    import test_prdc_gpu as TP
    import test_spectrum
    from contrad_amd import features, spectrum
    x = R.smooth_noise(16, 32, 12)
    np.savez(str(tmp_path / 'real.npz'), x_train=x)
    G = TP._encoder(6)[0]
    torch.save(G.state_dict(), str(tmp_path / 'gen.pt'))
    path = test_spectrum.main(['--real', str(tmp_path / 'real.npz'), '--gen', str(tmp_path / 'gen.pt'), '--gen_arch', 'sndcgan',
                               '--n_fake', '12', '--seed', '4', '--batch_size', '5'])
    assert path == str(tmp_path / 'spectrum_4.json')
    with open(path) as f:
        out = json.load(f)
    Gd = features.load_frozen(TP._encoder(6)[0], str(tmp_path / 'gen.pt'), torch.device('cuda', 0))
    want = spectrum.compare(_of(x), spectrum.spectrum_of(features.sample_u8(Gd, 12, 5, 4)))
    assert all(out[k] == want[k] for k in want) and (out['n_real'], out['n_fake']) == (16, 12)


def test_hook_appends_the_rows_and_leaves_the_checkpoints_bitwise_alone(tmp_path_factory):
    import test_prdc_gpu as TP
    from contrad_amd import features, spectrum
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_gan import main
    plain = TP._run(tmp_path_factory, False, False)
    d = tmp_path_factory.mktemp('spectrum_files')
    x = R.smooth_noise(64, 32, 13)
    np.savez(str(d / 'real.npz'), x_train=x)
    hooked = str(tmp_path_factory.mktemp('spectrum_run'))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', hooked, '--spectrum_data', str(d / 'real.npz'), '--spectrum_n', '48'])
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    assert not [f for f in os.listdir(plain) if f.startswith('spectrum_')]
    assert sorted(f for f in os.listdir(hooked) if f.endswith('.csv')) == ['spectrum_%d.csv' % TP.EVAL_SEED]
    with open(os.path.join(hooked, 'spectrum_%d.csv' % TP.EVAL_SEED)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,lsd_db,hf_db,nyq_h,nyq_v,nyq_d' and len(lines) == 3
    dev = torch.device('cuda', 0)
    real = spectrum.spectrum_of(torch.from_numpy(x[:48]).to(dev))
    for line, (step, name) in zip(lines[1:], ((2, 'gen_2.pt'), (4, 'gen.pt'))):
        G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, name), dev)
        out = spectrum.compare(real, spectrum.spectrum_of(features.sample_u8(G, 48, 500, TP.EVAL_SEED)))
        assert line == spectrum.csv_line(step, out), (line, out)
    with pytest.raises(ValueError):
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', hooked, '--spectrum_n', '8'])
