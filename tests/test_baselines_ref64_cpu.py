"""Baseline training modes, the part that needs no GPU: the host samplers replay the reference's recorded draws, the
float64 restatements (tests/baselines_ref64.py) reproduce the reference's outputs (tests/golden/baselines.npz) and their
hand-written adjoints equal float64 autograd, the file-name rules of ``setup(P)``, and what keeps raising."""
import argparse
import os

import pytest
import torch

import baselines_ref64 as R
from contrad_amd import config
from contrad_amd.augment import DiffAugLayer, HorizontalFlipLayer, HorizontalFlipRandomCrop, NoAugment, get_augment
from contrad_amd.penalty import compute_penalty
from contrad_amd.training.gan import setup

POLICIES = ('color', 'translation', 'cutout', 'color,cutout', 'color,translation,cutout')
HFRT_CASES = ('hfrt32', 'hfrt8', 'hfrt8m4')


def _bind_defaults():
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin')])


def T(a):
    return torch.from_numpy(a)


def test_hfrt_sampler_replays_the_recorded_draws(golden):
    g = golden('baselines')
    _bind_defaults()
    for tag in HFRT_CASES:
        x = T(g[tag + '/x'])
        layer = get_augment(mode='hfrt') if tag == 'hfrt32' else \
            HorizontalFlipRandomCrop(max_pixels=int(g[tag + '/m']), width=x.shape[2], padding_mode='reflection')
        assert (layer.max_pixels, layer.width) == (int(g[tag + '/m']), x.shape[2])
        torch.manual_seed(int(g[tag + '/seed']))
        assert torch.equal(layer.sample(x.shape[0]), T(g[tag + '/P'])), tag
    # the step fixtures: CR augments the N reals, bCR all 2N images, aug the N reals
    N = int(g['step/N'])
    for tag, B in (('std+cr+hfrt', N), ('std+bcr+hfrt', 2 * N), ('aug+hfrt', N)):
        torch.manual_seed(int(g['step/%s/seed' % tag]))
        assert torch.equal(get_augment(mode='hfrt').sample(B), T(g['step/%s/P' % tag])), tag
    # hflip draws the signs only
    torch.manual_seed(5)
    signs = HorizontalFlipLayer().sample(7)
    torch.manual_seed(5)
    assert torch.equal(signs[:, 0], torch.bernoulli(torch.ones(7) * 0.5) * 2 - 1) and signs[:, 1:].abs().max() == 0


def test_diffaug_sampler_replays_the_recorded_draws(golden):
    g = golden('baselines')
    x = T(g['diffaug/x'])
    for policy in POLICIES:
        torch.manual_seed(int(g['diffaug/%s/seed' % policy]))
        P = DiffAugLayer(policy=policy).sample(x.shape[0], x.shape[2], x.shape[3])
        assert torch.equal(P, T(g['diffaug/%s/P' % policy])), policy
    N = int(g['step/N'])
    _bind_defaults()
    with pytest.raises(NotImplementedError, match='diffaug_policy'):      # off until the configuration binds a policy
        get_augment(mode='diffaug')
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'gan', 'diffaug', 'c10_diffaug.gin')])
    layer = get_augment(mode='diffaug')
    assert layer.policy == 'color,cutout'
    for key, B in (('step/aug_both+diffaug/', 2 * N), ('gstep/', N)):
        torch.manual_seed(int(g[key + 'seed']))
        assert torch.equal(layer.sample(B, 32, 32), T(g[key + 'P'])), key


def test_ref64_reproduces_the_reference_outputs(golden):
    """fp32 reference data: 1e-6; the hfrt index formula reproduces the reference bit for bit."""
    g = golden('baselines')
    for tag in HFRT_CASES:
        assert torch.equal(R.hfrt_forward(T(g[tag + '/x']), T(g[tag + '/P'])), T(g[tag + '/y'])), tag
    x = T(g['diffaug/x'])
    for policy in POLICIES:
        y = R.diffaug_forward(x, T(g['diffaug/%s/P' % policy]), policy)
        err = (y - T(g['diffaug/%s/y' % policy]).double()).abs().max().item()
        assert err < 1e-6, (policy, err)
        dead = R.diffaug_dead_outputs(T(g['diffaug/%s/P' % policy]), policy, x.shape[2], x.shape[3])
        assert (y.permute(0, 2, 3, 1)[dead] == 0.5).all()


def _forced_hfrt_rows(m):
    return torch.tensor([[s, kx, ky, 0.] for s in (1., -1.) for kx in (-m, 0, m) for ky in (-m, 1, m)])


def test_adjoints_match_float64_autograd():
    gen = torch.Generator().manual_seed(9)
    for W, m in ((32, 4), (8, 7), (8, 4)):
        P = _forced_hfrt_rows(m)
        x = torch.rand(P.shape[0], 3, W, W, generator=gen, dtype=torch.float64).requires_grad_()
        g = torch.rand(x.shape, generator=gen, dtype=torch.float64)
        want, = torch.autograd.grad((R.hfrt_forward(x, P) * g).sum(), x)
        assert (R.hfrt_adjoint(g, P) - want).abs().max().item() < 1e-12, (W, m)
    for H, W in ((32, 32), (30, 20), (16, 12)):
        sx, sy, cx, cy = int(H * .125 + .5), int(W * .125 + .5), int(H * .5 + .5), int(W * .5 + .5)
        P = torch.tensor([[0.3, 0.0, 0.5, sx, -sy, 0, W - cy % 2, 0], [-0.4, 1.7, 1.4, -sx, sy, H - cx % 2, 0, 0],
                          [0.1, 0.6, 0.9, 1, -1, H // 2, W // 3, 0]])
        x = torch.rand(3, 3, H, W, generator=gen, dtype=torch.float64).requires_grad_()
        g = torch.rand(x.shape, generator=gen, dtype=torch.float64)
        for policy in POLICIES:
            want, = torch.autograd.grad((R.diffaug_forward(x, P, policy) * g).sum(), x)
            assert (R.diffaug_backward(g, P, policy) - want).abs().max().item() < 1e-12, (H, W, policy)
    a = torch.rand(10, 1, generator=gen, dtype=torch.float64).requires_grad_()
    b = torch.rand(10, 1, generator=gen, dtype=torch.float64).requires_grad_()
    for n0, n1, l0, l1 in ((10, 0, 10.0, 0.0), (5, 5, 10.0, 3.0)):
        want = l0 * (a[:n0] - b[:n0]).pow(2).mean() + (l1 * (a[n0:] - b[n0:]).pow(2).mean() if n1 else 0.0)
        ga, gb = torch.autograd.grad(want, (a, b))
        val, ha, hb = R.consistency(a.detach(), b.detach(), n0, n1, l0, l1)
        assert abs(val.item() - want.item()) < 1e-12
        assert (ha - ga).abs().max().item() < 1e-12 and (hb - gb).abs().max().item() < 1e-12


def test_setup_file_names_follow_the_reference_rules():
    def name(**kw):
        base = dict(mode='std', penalty='none', aug='none', temp=0.1, lbd_a=1.0)
        base.update(kw)
        return setup(argparse.Namespace(**base)).filename
    assert name() == 'std_none'
    assert name(penalty='cr', aug='hfrt') == 'std_cr_hfrt' and name(penalty='bcr', aug='hfrt') == 'std_bcr_hfrt'
    assert name(penalty='gp', aug='hfrt') == 'std_gp'
    assert name(mode='aug', aug='hfrt') == 'aug_hfrt_none'
    assert name(mode='aug_both', aug='diffaug', penalty='cr') == 'aug_both_diffaug_cr'
    assert name(mode='contrad', aug='simclr') == 'contrad_simclr_L1.0_T0.1'         # (unchanged)
    P = setup(argparse.Namespace(mode='aug_both', penalty='none', aug='diffaug'))
    assert callable(P.train_fn['G']) and callable(P.train_fn['D'])
    with pytest.raises(NotImplementedError):
        name(mode='no_such_mode')


def test_what_keeps_raising():
    _bind_defaults()
    with pytest.raises(NotImplementedError, match='second-order'):
        compute_penalty('gp', D=None, images=None, gen_images=None, lbd=10.0, P=None)
    for mode in ('gaussian', 'color_jitter', 'cutout'):
        with pytest.raises(NotImplementedError):
            get_augment(mode=mode)
    assert isinstance(get_augment(mode='none'), NoAugment) and isinstance(get_augment(mode='hflip'), HorizontalFlipLayer)
    x = torch.rand(2, 3, 4, 4)
    assert get_augment(mode='none')(x) is x
    assert compute_penalty('none', images=x, D=None).shape == (1,)
    with pytest.raises(NotImplementedError):
        DiffAugLayer(policy='cutout,color')                  # stages out of the kernel's order
    with pytest.raises(NotImplementedError):
        HorizontalFlipRandomCrop(max_pixels=4, width=32, padding_mode='zeros')
    with pytest.raises(ValueError):
        HorizontalFlipRandomCrop(max_pixels=8, width=8, padding_mode='reflection')
    with pytest.raises(RuntimeError):                        # no CPU fallback
        get_augment(mode='hfrt')(torch.rand(2, 3, 32, 32))


def test_multi_rank_baselines_stop_at_start_up(monkeypatch):
    from contrad_amd import train_gan, train_stylegan2
    monkeypatch.setenv('WORLD_SIZE', '2')
    gin = os.path.join(config.CONFIG_ROOT, 'gan', 'cifar10', 'c10_b64.gin')
    with pytest.raises(NotImplementedError, match='one GPU'):
        train_gan.main([gin, 'sndcgan', '--mode=std', '--synthetic'])
    with pytest.raises(NotImplementedError, match='one GPU'):
        train_stylegan2.main([os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2',
                              '--mode=aug_both', '--aug=diffaug', '--synthetic'])
