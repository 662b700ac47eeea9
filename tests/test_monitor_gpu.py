"""``--monitor``: the grids are written, and the training trajectory does not move by a bit."""
import glob
import os

import numpy as np
import pytest
import torch

from grid_ref import grid_ref
from png_reader import read_frames, read_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
_RUNS = {}


def _eval_seed():
    return int(np.random.RandomState(SEED).randint(10000))


def _run(factory, graph, monitor):
    """One 4-step train_gan run per (graph, monitor), shared by the tests of this module."""
    key = (graph, monitor)
    if key not in _RUNS:
        from contrad_amd.train_gan import main
        logdir = str(factory.mktemp('run_%d%d' % key))
        gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2',
              '--seed', str(SEED), '--logdir', logdir] + (['--graph'] if graph else []) + (['--monitor'] if monitor else []))
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


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_monitoring_leaves_the_checkpoints_bitwise_alone(graph, tmp_path_factory):
    plain, mon = _run(tmp_path_factory, graph, False), _run(tmp_path_factory, graph, True)
    for name in ('gen.pt', 'dis.pt', 'optim.pt'):
        _same(torch.load(os.path.join(plain, name), map_location='cpu'), torch.load(os.path.join(mon, name), map_location='cpu'))
    s = _eval_seed()
    made = ['progress_%d' % s, 'training_progress_%d.png' % s, 'real_augment_%d.png' % s]
    assert all(os.path.exists(os.path.join(mon, m)) for m in made)
    assert sorted(os.listdir(os.path.join(mon, 'progress_%d' % s))) == ['step_2.png', 'step_4.png']
    assert not glob.glob(os.path.join(plain, '*.png')) and not glob.glob(os.path.join(plain, 'progress_*'))
    assert not glob.glob(os.path.join(mon, 'fixed_gen_*'))
    step2, step4 = (read_png(os.path.join(mon, 'progress_%d' % s, 'step_%d.png' % k)) for k in (2, 4))
    assert step2.shape == step4.shape == (138, 138, 3)              # 16 samples of 32 x 32, 4 per row, padding 2
    assert not np.array_equal(step2, step4)                         # the weights moved
    frames = read_frames(os.path.join(mon, 'training_progress_%d.png' % s))
    assert len(frames) == 2 and np.array_equal(frames[0], step2) and np.array_equal(frames[1], step4)
    aug = read_png(os.path.join(mon, 'real_augment_%d.png' % s))
    assert aug.shape == (274, 274, 3) and len(np.unique(aug)) > 16  # 64 images of 32 x 32, 8 per row


def test_fixed_latent_grids_follow_the_weights_not_the_run(tmp_path_factory):
    from contrad_amd.evaluate.gan import N_FIXED, fixed_latent
    from contrad_amd.models.gan import get_architecture
    s = _eval_seed()
    eager, graph = _run(tmp_path_factory, False, True), _run(tmp_path_factory, True, True)
    for k in (2, 4):
        a, b = (read_png(os.path.join(d, 'progress_%d' % s, 'step_%d.png' % k)) for d in (eager, graph))
        assert np.array_equal(a, b), k
    # step 4 is the checkpoint's generator, in eval mode, at the seeded latents
    G, _ = get_architecture('sndcgan', (32, 32, 3))
    G.load_state_dict(torch.load(os.path.join(eager, 'gen.pt'), map_location='cpu'))
    G = G.to('cuda').eval()
    for p in G.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        want = grid_ref(G(fixed_latent(G, N_FIXED, s)).cpu(), 4, 2)
    assert np.array_equal(read_png(os.path.join(eager, 'progress_%d' % s, 'step_4.png')), want)


def test_no_gif_keeps_one_file(tmp_path):
    from contrad_amd.train_gan import main
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    logdir = str(tmp_path / 'run')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '2', '--evaluate_every', '1',
          '--seed', str(SEED), '--logdir', logdir, '--monitor', '--no_gif'])
    s = _eval_seed()
    assert sorted(f for f in os.listdir(logdir) if f.endswith('.png')) == ['fixed_gen_%d.png' % s, 'real_augment_%d.png' % s]
    assert not glob.glob(os.path.join(logdir, 'progress_*'))
    assert read_png(os.path.join(logdir, 'fixed_gen_%d.png' % s)).shape == (138, 138, 3)


def test_stylegan2_loop_shows_g_ema(tmp_path):
    from contrad_amd import config
    from contrad_amd.evaluate.gan import N_FIXED, fixed_latent
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_stylegan2 import main
    logdir = str(tmp_path / 'run')
    main([os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
          '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
          '--seed', str(SEED), '--logdir', logdir, '--monitor'])
    s = _eval_seed()
    grid = read_png(os.path.join(logdir, 'progress_%d' % s, 'step_2.png'))
    assert grid.shape == (138, 138, 3)
    assert len(read_frames(os.path.join(logdir, 'training_progress_%d.png' % s))) == 1
    assert read_png(os.path.join(logdir, 'real_augment_%d.png' % s)).shape == (36, 274, 3)      # the 8 images of the batch
    # the grid is gen_ema.pt's generator (not gen.pt's) at the seeded latents, per-layer noise from the seeded device stream
    shown = {}
    for name in ('gen_ema.pt', 'gen.pt'):
        G, _ = get_architecture('stylegan2', (32, 32, 3))
        G.load_state_dict(torch.load(os.path.join(logdir, name), map_location='cpu'))
        G = G.to('cuda').eval()
        for p in G.parameters():
            p.requires_grad_(False)
        torch.cuda.manual_seed(s)
        with torch.no_grad():
            shown[name] = grid_ref(G(fixed_latent(G, N_FIXED, s)).cpu(), 4, 2)
    assert np.array_equal(grid, shown['gen_ema.pt']) and not np.array_equal(grid, shown['gen.pt'])
