"""The float64 yardstick of the StyleGAN2 projector (tests/project_ref64.py) against float64 autograd of the literal formulas,
the level counts, the schedule, the zero-variance rule, the host refusals of contrad_amd/project.py and of
``test_gan_walk.py --latents``, the -EINVAL cases of the four entry points, and the descent of the float64 loop at the settings
test_project_gpu.py uses.  No GPU."""
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch

import project_ref64 as R
from conftest import ROOT

EINVAL = -22


# ---- the hand-derived gradients against autograd of the literal formulas ----
@pytest.mark.parametrize('size,lam', [(8, (1.0,)), (16, (1.0, 0.5)), (32, (0.25, 1.0, 2.0, 0.5))])
def test_image_end_gradient_is_autograd_of_the_definition(size, lam):
    g = np.random.RandomState(size)
    x, t = g.rand(3, 3, size, size), g.rand(3, 3, size, size)
    pix, gx = R.image_end(x, t, lam)
    xt = torch.from_numpy(x).requires_grad_()
    total, rows = R.image_end_torch(xt, torch.from_numpy(t), lam)
    total.backward()
    assert np.abs(pix - rows.detach().numpy()).max() <= 1e-14 * np.abs(pix).max()
    assert np.abs(gx - xt.grad.numpy()).max() <= 1e-14 * np.abs(gx).max()
    zero_pix, zero_g = R.image_end(x, x, lam)
    assert not zero_pix.any() and not zero_g.any()


@pytest.mark.parametrize('R_', [4, 8, 16, 32, 64])
def test_noise_reg_gradient_is_autograd_of_the_loop(R_):
    g = np.random.RandomState(R_)
    m = g.randn(2, 1, R_, R_)
    reg, grad = R.noise_reg(m)
    mt = torch.from_numpy(m).requires_grad_()
    want = R.noise_reg_torch(mt)
    want.sum().backward()
    assert np.abs(reg - want.detach().numpy()).max() <= 1e-13 * np.abs(reg).max()
    assert np.abs(grad - mt.grad.numpy()).max() <= 1e-13 * np.abs(grad).max()


def test_noise_grad_is_autograd_of_the_epilogue():
    g = torch.Generator().manual_seed(3)
    y, noise = torch.randn(2, 5, 7, 24, generator=g, dtype=torch.float64), torch.randn(2, 1, 5, 7, generator=g, dtype=torch.float64)
    noise.requires_grad_()
    nw, gy = 0.3, torch.randn(2, 5, 7, 24, generator=g, dtype=torch.float64)
    pre = y + nw * noise.permute(0, 2, 3, 1)
    (pre * gy).sum().backward()
    assert np.abs(R.noise_grad(gy.numpy(), nw) - noise.grad.numpy()).max() <= 1e-14 * float(noise.grad.abs().max())


def test_level_counts():
    from contrad_amd import ops
    assert [R.reg_levels(r) for r in (4, 8, 16, 32, 512)] == [1, 1, 2, 3, 7]
    assert [ops.proj_noise_levels(r) for r in (4, 8, 16, 32, 64, 512, 1024)] == [R.reg_levels(r) for r in (4, 8, 16, 32, 64, 512, 1024)]
    assert [len(R._pyramid(np.zeros((1, 1, r, r)))) for r in (4, 8, 16, 32, 512)] == [1, 1, 2, 3, 7]
    # the scratch formula of the header, restated
    for N, r in ((1, 4), (3, 64), (1, 512), (2, 1024)):
        J = R.reg_levels(r)
        want = N * (sum((r >> j) ** 2 for j in range(1, J)) + 2 * J * R.cdiv(r * r, 4096) + 2 * J)
        assert ops.proj_noise_reg_scratch_floats(N, r) == want
    assert ops.proj_image_end_partial_floats(4, 3, 32, 32) == 4 * 3 * 3 * (32 // R.image_end_rows(4, 32, 32))
    assert R.image_end_rows(1, 512, 512) == 8 and R.image_end_rows(4, 8, 8) == 8 and R.image_end_rows(4, 1024, 1024) == 8


def test_schedule_values():
    from contrad_amd import project
    for f in (R.schedule, project.schedule):
        assert f(0.0) == 0.0                                                  # the first step does not move
        assert f(0.05) == 1.0 and f(0.75) == 1.0 and f(0.5) == 1.0            # the rampup and 1 - rampdown boundaries
        assert abs(f(0.025) - 0.5) < 1e-15
        assert abs(f(0.875) - 0.5) < 1e-15                                    # half way down the cosine
        assert 0.0 < f(1.0 - 1e-9) < 1e-15                                    # t -> 1
        assert f(1.0) == 0.0
    for t in np.linspace(0.0, 1.0, 41):
        assert project.schedule(float(t)) == R.schedule(float(t))
        assert project.perturbation(float(t), 2.0) == R.perturbation(float(t), 2.0)
    assert R.perturbation(0.0, 2.0) == 2.0 * 0.05 and R.perturbation(0.75, 2.0) == 0.0 and R.perturbation(0.9, 2.0) == 0.0


def test_a_zero_variance_map_normalises_to_zeros():
    m = np.full((2, 1, 8, 8), np.float32(0.1), np.float64)           # (an fp32 value: its float64 sums are exact)
    m[1] = np.random.RandomState(0).randn(1, 8, 8)
    out = R.noise_normalize(m)
    assert not out[0].any()
    assert abs(out[1].mean()) < 1e-15 and abs((out[1] ** 2).mean() - 1.0) < 1e-14
    assert np.all(np.isfinite(R.noise_normalize_bound(m)))


# ---- host refusals ----
def _run_dir(tmp_path, gin=('gan', 'stylegan2', 'c10_style64.gin')):
    run = tmp_path / 'run'
    run.mkdir()
    shutil.copy(os.path.join(ROOT, 'configs', *gin), str(run / gin[-1]))
    return run


def test_command_line_refusals_touch_no_gpu(tmp_path):
    import test_gan_project  # noqa: F401  (the entry script imports)
    from contrad_amd import project
    was = torch.cuda.is_initialized()
    run = _run_dir(tmp_path)
    gen = str(run / 'gen_ema.pt')
    np.savez(str(tmp_path / 'set.npz'), x_train=np.random.RandomState(0).randint(0, 255, (4, 32, 32, 3)).astype(np.uint8))
    data = ['--data', str(tmp_path / 'set.npz')]
    for bad, what in ((['--steps', '0'], 'steps'), (['--n', '0'], 'steps'), (['--batch_size', '0'], 'steps'), (['--w_avg_n', '0'], 'steps'),
                      (['--level_weights', '1', '1', '1', '1', '1'], 'level_weights'), (['--level_weights', '0'], 'level_weights'),
                      (['--level_weights=-1'], 'level_weights'), (['--reg_weight=-1'], 'reg_weight'), (['--lr=-0.1'], 'reg_weight'),
                      (['--rows=-1'], '--rows'), (['--n', '8'], 'beyond the 4 images'), (['--n', '2', '--holdout'], 'x_test'),
                      (['--n', '2', '--rows', '2'], '--rows 2')):
        with pytest.raises(ValueError, match=what):
            project.main([gen, 'stylegan2'] + bad + data)
    with pytest.raises(SystemExit):
        project.main([gen, 'stylegan2', '--space', 'z'] + data)
    with pytest.raises(SystemExit):
        project.main([gen, 'stylegan2', '--noise', 'free'] + data)
    srun = tmp_path / 's'
    srun.mkdir()
    shutil.copy(os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin'), str(srun / 'c10_b64.gin'))
    with pytest.raises(ValueError, match='no W'):                              # latent.need_w: no mapping network
        project.main([str(srun / 'gen.pt'), 'sndcgan', '--n', '2'] + data)
    assert project.check_arguments('wplus', 'fixed', (1, 0, 2), 0.0, 0.1) == [1.0, 0.0, 2.0]
    assert torch.cuda.is_initialized() == was


def test_projector_refusals_touch_no_gpu():
    from contrad_amd import project
    from contrad_amd.models.gan.stylegan2.generator import Generator
    was = torch.cuda.is_initialized()
    G = Generator(size=8).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        project.Projector(G, 2)
    with pytest.raises(ValueError, match='space'):
        project.Projector(G, 2, space='z')
    with pytest.raises(ValueError, match='noise'):
        project.Projector(G, 2, noise='free')
    with pytest.raises(ValueError, match='no W'):
        project.Projector(torch.nn.Linear(2, 2).eval(), 2)
    G.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        project.Projector(G, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.synthesize(torch.zeros(1, G.n_latent, 512), [None] * G.num_layers)
    assert torch.cuda.is_initialized() == was


def test_walk_latents_refusals_touch_no_gpu(tmp_path):
    import test_gan_walk
    from contrad_amd import recover
    was = torch.cuda.is_initialized()
    run = _run_dir(tmp_path)
    gen = str(run / 'gen_ema.pt')
    recover.write_npz(str(tmp_path / 'no_w.npz'), pix=np.zeros(3, np.float32))
    recover.write_npz(str(tmp_path / 'p.npz'), w=np.zeros((3, 8, 512), np.float32))
    recover.write_npz(str(tmp_path / 'flat.npz'), w=np.zeros((3, 512), np.float32))
    with pytest.raises(ValueError, match='holds no w'):
        test_gan_walk.main([gen, 'stylegan2', '--latents', str(tmp_path / 'no_w.npz')])
    with pytest.raises(ValueError, match='holds 3 codes'):
        test_gan_walk.main([gen, 'stylegan2', '--latents', str(tmp_path / 'p.npz'), '--latent_rows', '0', '3'])
    with pytest.raises(ValueError, match='holds 3 codes'):
        test_gan_walk.main([gen, 'stylegan2', '--latents', str(tmp_path / 'p.npz'), '--latent_rows', '1', '-1'])
    with pytest.raises(ValueError, match='at least two'):
        test_gan_walk.main([gen, 'stylegan2', '--latents', str(tmp_path / 'p.npz'), '--latent_rows', '1'])
    with pytest.raises(ValueError, match='n_latent'):
        test_gan_walk.main([gen, 'stylegan2', '--latents', str(tmp_path / 'flat.npz')])
    with pytest.raises(ValueError, match='without --latents'):
        test_gan_walk.main([gen, 'stylegan2', '--latent_rows', '0', '1'])
    with pytest.raises(ValueError, match='no W'):
        test_gan_walk.main([gen, 'sndcgan', '--latents', str(tmp_path / 'p.npz')])
    assert torch.cuda.is_initialized() == was


# ---- the entry points' own refusals ----
@pytest.fixture(scope='module')
def built():
    from contrad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_without_gpu(built):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base % 16))
    q = ctypes.c_void_p(p.value + 4096)
    ll = ctypes.c_longlong
    lam = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    img = built.raw('contrad_proj_image_end')
    good = [p, p, lam, 2, p, q, p, ll(1 << 20), 2, 8, 8, None]
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (6, None), (3, 0), (3, 5), (8, 0), (8, 65536), (9, 7), (10, 7),
                   (5, p), (7, ll(2 * 2 * 3 * 1 - 1))):
        args = list(good)
        args[i] = bad
        assert img(*args) == EINVAL, (i, bad)
    assert img(p, p, (ctypes.c_float * 1)(float('nan')), 1, p, q, p, ll(1 << 20), 2, 8, 8, None) == EINVAL
    assert img(p, p, lam, 4, p, q, p, ll(1 << 20), 1, 8, 2048, None) == EINVAL          # 8 rows of 2048 do not fit a workgroup
    ng = built.raw('contrad_proj_noise_grad')
    for args in ((None, p, p, ll(4), 8, None), (p, None, p, ll(4), 8, None), (p, p, None, ll(4), 8, None), (p, p, p, ll(0), 8, None),
                 (p, p, p, ll(4), 0, None), (p, p, p, ll(4), 65537, None)):
        assert ng(*args) == EINVAL, args
    reg = built.raw('contrad_proj_noise_reg')
    good = [p, p, q, 1.0, p, ll(1 << 20), 1, 16, None]
    off = ctypes.c_void_p(p.value + 4)
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (6, 0), (7, 2), (7, 24), (7, 2048), (0, off), (4, off), (3, float('inf')),
                   (2, p), (5, ll(64 + 2 * 2 + 2 * 2 - 1))):
        args = list(good)
        args[i] = bad
        assert reg(*args) == EINVAL, (i, bad)
    nm = built.raw('contrad_proj_noise_normalize')
    for args in ((None, 1, 8, None), (p, 0, 8, None), (p, 1, 2, None), (p, 1, 12, None), (p, 1, 2048, None), (off, 1, 8, None)):
        assert nm(*args) == EINVAL, args


# ---- the descent case of test_project_gpu.py ----
def test_the_float64_loop_descends_at_the_gpu_tests_settings():
    import test_project_gpu as T
    case = T.descent_case()
    steps = R.projector(case['sd'], case['size'], case['n_latent'], case['target'], case['w0'], case['maps'],
                        [torch.zeros_like(case['w0'])] * T.DESCENT_STEPS, (1.0,), 0.0, T.DESCENT_LR, False)
    first, last = steps[0]['pix'][0], steps[-1]['pix'][0]
    print('float64 pix_opt: first %s last %s' % (first.tolist(), last.tolist()))
    assert bool((last < first).all())
    assert bool((last < 0.9 * first).all())                                 # (a margin the fp32 path cannot eat)
