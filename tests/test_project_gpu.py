"""The StyleGAN2 projector (contrad_amd/project.py) on the GPU: ``Generator.synthesize`` with the loss
ends against the float64 synthesis of tests/project_ref64.py (gradients, a three-step trajectory), the fixed point, the
descent, the frozen generator and the two command lines.  Generators: ``Generator(size=8)`` and ``size=16, small32=True`` with
deterministic weights (oracle.stylegan2_oracle.det_fill_g), N = 2.

Tolerances of the whole-network comparisons ((a) and (b)): TOL = 1e-3 of the reference tensor's largest magnitude on the SAME
leaky-relu regions, the tolerance of the other same-region whole-network tests against float64 (tests/test_stylegan2_gstep_gpu.py,
tests/test_recover_gpu.py; DESIGN.md sections 4 and 20).  ``Generator.synthesize`` records the regions its forward ran on
(``_record_regions``) and the float64 synthesis is evaluated on them: leaky-relu's derivative jumps at 0, and a pre-activation
of 3.5e-7 (fp32 summation noise; the 16 x 16 W+ case has one) otherwise changes sides and moves whole rows of the gradient by
1e-3 ... 8e-3 of its maximum, which is no kernel error.  What keeps the imposed regions honest: they may differ from the
reference's own only in units whose float64 pre-activation is below FLIP_PRE = 1e-5 (a 4608-term fp32 dot product of rms 0.5
through five layers is good to about 1e-6), and in at most FLIP_MAX of them.  Observed on the MI355X:
profiles/project_margins.txt."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import project_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
FLIP_PRE, FLIP_MAX = 1e-5, 8
N = 2
DESCENT_STEPS, DESCENT_LR = 8, 0.02       # the float64 loop descends for both images (tests/test_project_ref64_cpu.py runs it)
_cache = {}


def _generator(size, small32):
    """(G on the CPU in eval mode, its float64 state) with deterministic weights; made once per size."""
    key = (size, small32)
    if key not in _cache:
        from contrad_amd.evaluate.gan import freeze
        from contrad_amd.models.gan.stylegan2.generator import Generator
        from oracle import stylegan2_oracle as S
        G = Generator(size=size, small32=small32)
        shapes = S.g_param_shapes(size, small32)
        sd = S.fill_kernels(S.det_fill_g(shapes, seed=777 + size), shapes)
        for k in sd:
            if k.endswith('noise.weight'):
                sd[k] = torch.full_like(sd[k], 0.1)
        G.load_state_dict(sd)
        _cache[key] = (freeze(G), R.state64(G))
    return _cache[key]


def _on_gpu(size, small32):
    key = ('cuda', size, small32)
    if key not in _cache:
        import copy
        _cache[key] = copy.deepcopy(_generator(size, small32)[0]).cuda()
    return _cache[key]


def _inputs(G, space, seed, per_image=True):
    """Seeded CPU float32 (w, maps, target) for N images of G's size."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((N, G.style_dim) if space == 'w' else (N, G.n_latent, G.style_dim), generator=g) * 0.5
    maps = [torch.randn(N if per_image else 1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2), generator=g) for i in range(G.num_layers)]
    target = torch.rand(N, 3, G.size, G.size, generator=g)
    return w, maps, target


def _rel(got, want):
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def descent_case():
    """The inputs of the descent test, all on the CPU: targets painted by the float64 synthesis at latents half a unit from the
    start, one shared noise list, the start at the mean of 64 mapped draws."""
    if 'descent' not in _cache:
        from oracle import stylegan2_oracle as S
        G, sd = _generator(8, False)
        g = torch.Generator().manual_seed(41)
        w_avg = S.mapping(sd, torch.randn(64, G.style_dim, generator=g, dtype=torch.float64)).mean(0, keepdim=True)
        w0 = w_avg.float().repeat(N, 1)
        maps = [torch.randn(1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2), generator=g) for i in range(G.num_layers)]
        w_t = w0.double() + 0.5 * torch.randn(N, G.style_dim, generator=g, dtype=torch.float64)
        with torch.no_grad():
            target = R.synthesis(sd, R.to_latents(w_t, G.n_latent), [m.double() for m in maps], 8).clamp(0, 1).float()
        _cache['descent'] = dict(sd=sd, size=8, n_latent=G.n_latent, target=target.double(), w0=w0, maps=[m.double() for m in maps],
                                 maps32=maps)
    return _cache['descent']


# ---- (a) gradients against float64 ----
@pytest.mark.parametrize('size,small32,space,reg_weight', [(8, False, 'w', 0.0), (8, False, 'wplus', 0.05), (16, True, 'w', 0.05),
                                                          (16, True, 'wplus', 0.0)])
def test_gradients_against_float64(margin, size, small32, space, reg_weight):
    from contrad_amd import project_nodes as PN
    (Gc, sd), G = _generator(size, small32), _on_gpu(size, small32)
    lam = (1.0, 0.5)
    w, maps, target = _inputs(Gc, space, 5 * size)
    wd = w.cuda().requires_grad_()
    md = [m.cuda().requires_grad_() for m in maps]
    lat = wd.unsqueeze(1).repeat(1, G.n_latent, 1) if space == 'w' else wd
    G._record_regions = []
    try:
        x = G.synthesize(lat, md, noise_grad=True)
        masks = R.region_masks(G._record_regions)
    finally:
        G._record_regions = None
    pres = []
    loss64, rows64, regs64, gw64, gmaps64 = R.loss_and_grads(sd, size, Gc.n_latent, target.double(), w.double(), [m.double() for m in maps],
                                                             lam, reg_weight, True, masks=masks, pres=pres)
    flips, worst_pre = R.region_changes(masks, pres)
    print('size %d %s: %d units on the other side of 0 than in float64, largest |pre| among them %.3g' % (size, space, flips, worst_pre))
    assert len(masks) == G.num_layers and flips <= FLIP_MAX and worst_pre < FLIP_PRE
    rows, gx = PN.image_end(x, target.cuda(), lam)
    x.backward(gx)
    regs = torch.stack([PN.noise_reg_(m, m.grad, reg_weight) for m in md])
    name = 'project grads size=%d %s reg_weight=%g/' % (size, space, reg_weight)
    margin(name + 'pix rows', _rel(rows, rows64), TOL)
    margin(name + 'reg rows', _rel(regs, regs64), TOL)
    margin(name + 'd w', _rel(wd.grad, gw64), TOL)
    for i, (m, g64) in enumerate(zip(md, gmaps64)):
        margin(name + 'd noise %d' % i, _rel(m.grad, g64), TOL)
    assert all(p.grad is None for p in G.parameters())


# ---- (b) three steps against the float64 loop ----
@pytest.mark.parametrize('space', ['w', 'wplus'])
def test_three_step_trajectory_against_float64(margin, space):
    from contrad_amd import project
    (Gc, sd), G = _generator(8, False), _on_gpu(8, False)
    lam, w_std = (1.0, 1.0), 1.0
    w0, maps, target = _inputs(Gc, space, 77)
    g = torch.Generator().manual_seed(78)
    gauss = [torch.randn(w0.shape, generator=g) for _ in range(3)]
    proj = project.Projector(G, N, space, 'opt', lam, w_std=w_std)
    proj.set_targets(target.cuda())
    proj.start(w0.cuda(), [m.cuda() for m in maps])
    got, regions = [], []
    for s in range(3):
        G._record_regions = []
        try:
            proj.step(s, 3, gauss=gauss[s].cuda())
            regions.append(R.region_masks(G._record_regions))
        finally:
            G._record_regions = None
        loss, rows, reg = proj.loss_rows()
        got.append((proj.w.detach().clone(), loss, rows, reg, [m.detach().clone() for m in proj.maps]))
    want = R.projector(sd, 8, Gc.n_latent, target.double(), w0, maps, gauss, lam, project.DEFAULT_REG_WEIGHT, project.DEFAULT_LR, True,
                       w_std=w_std, regions=regions)
    for s, (w_s, loss, rows, reg, maps_s) in enumerate(got):
        flips, worst_pre = want[s]['flips']
        assert flips <= FLIP_MAX and worst_pre < FLIP_PRE, (s, flips, worst_pre)
        name = 'project trajectory %s step %d/' % (space, s)
        margin(name + 'w', _rel(w_s, want[s]['w']), TOL)
        margin(name + 'loss', _rel(loss, want[s]['loss']), TOL)
        margin(name + 'pix rows', _rel(rows, want[s]['pix']), TOL)
        margin(name + 'reg', _rel(reg, want[s]['reg'].sum(0)), TOL)
        for i, m in enumerate(maps_s):
            margin(name + 'map %d' % i, _rel(m, want[s]['maps'][i]), TOL)
    assert not np.array_equal(_bits(proj.w), _bits(w0))               # (the steps moved w)


# ---- (c) the fixed point ----
def test_fixed_point():
    from contrad_amd import project
    (Gc, _sd), G = _generator(16, True), _on_gpu(16, True)
    for noise_mode, steps in (('opt', 1), ('fixed', 3)):
        w0, maps, _ = _inputs(Gc, 'w', 9, per_image=(noise_mode == 'opt'))
        w0, maps = w0.cuda(), [m.cuda() for m in maps]
        with torch.no_grad():
            target = G.synthesize(w0.unsqueeze(1).repeat(1, G.n_latent, 1), maps).contiguous()
        proj = project.Projector(G, N, 'w', noise_mode, (1.0, 1.0, 1.0), reg_weight=0.0, noise_factor=0.0, w_std=1.0)
        proj.set_targets(target)
        proj.start(w0, maps)
        for s in range(steps):
            proj.step(s, steps)
            _loss, rows, _reg = proj.loss_rows()
            assert not _bits(rows).any()                              # the residual is exactly 0 at every level
            assert not (proj.gx != 0).any() and not (proj.w.grad != 0).any()
            if noise_mode == 'opt':
                assert all(not (m.grad != 0).any() for m in proj.maps)
        assert np.array_equal(_bits(proj.w), _bits(w0))


# ---- (d) descent ----
def test_descent_from_the_mean_latent():
    from contrad_amd import project
    case, G = descent_case(), _on_gpu(8, False)
    proj = project.Projector(G, N, 'w', 'fixed', (1.0,), reg_weight=0.0, lr0=DESCENT_LR, noise_factor=0.0)
    proj.set_targets(case['target'].float().cuda())
    proj.start(case['w0'].cuda(), [m.cuda() for m in case['maps32']])
    pix = []
    for s in range(DESCENT_STEPS):
        proj.step(s, DESCENT_STEPS, gauss=torch.zeros_like(proj.w))
        pix.append(proj.loss_rows()[1][0].cpu())
    print('pix_opt: first %s last %s' % (pix[0].tolist(), pix[-1].tolist()))
    assert bool((pix[-1] < pix[0]).all())


# ---- (e) the frozen generator ----
def test_frozen_generator():
    import copy
    from contrad_amd import project
    (Gc, _sd), G = _generator(16, True), _on_gpu(16, True)
    w, maps, target = _inputs(Gc, 'wplus', 13)
    w, maps = w.cuda(), [m.cuda() for m in maps]
    Gt = copy.deepcopy(G)
    for p in Gt.parameters():
        p.requires_grad_(True)
    want = Gt(w, input_is_latent=True, noise=maps)                    # eval mode, gradients on: the differentiable path
    assert want.requires_grad
    got = G.synthesize(w, maps)
    assert not got.requires_grad
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(G.synthesize(w, maps)), _bits(want))  # (from the cached tables)
    proj = project.Projector(G, N, 'wplus', 'opt', w_std=1.0)
    proj.set_targets(target.cuda())
    proj.start(w, maps)
    proj.step(0, 2)
    proj.step(1, 2)
    assert all(p.grad is None and not p.requires_grad for p in G.parameters())
    assert not np.array_equal(_bits(proj.w), _bits(w))


# ---- (f) the command lines ----
def test_command_lines(tmp_path):
    import png_reader
    import test_gan_project
    import test_gan_walk
    from contrad_amd import config, latent, ops, recover
    from contrad_amd.evaluate.gan import freeze
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(31)
    G = freeze(get_architecture('stylegan2', (32, 32, 3))[0].cuda())
    run = tmp_path / 'run'
    run.mkdir()
    torch.save(G.state_dict(), str(run / 'gen_ema.pt'))
    shutil.copy(os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), str(run / 'c10_style64.gin'))
    written = []
    for _ in range(2):                                                # same seed, same bytes
        path = test_gan_project.main([str(run / 'gen_ema.pt'), 'stylegan2', '--synthetic', '--n', '2', '--steps', '3', '--seed', '5',
                                      '--rows', '1', '--w_avg_n', '64', '--batch_size', '2', '--save_noise'])
        assert path == str(run / 'project_5.json')
        written.append([open(str(run / ('project_5.' + ext)), 'rb').read() for ext in ('json', 'npz')])
        os.remove(str(run / 'project_5.npz'))
        os.remove(str(run / 'project_5.json'))
    assert written[0] == written[1]
    with open(str(run / 'project_5.npz'), 'wb') as f:
        f.write(written[0][1])
    out = json.loads(written[0][0].decode())
    assert 'provisional' in out['note'] and out['steps'] == 3 and out['train']['n'] == 2 and out['space'] == 'w' and out['noise'] == 'opt'
    outs = [run]
    with np.load(str(outs[0] / 'project_5.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    assert arrays['w'].shape == (2, G.n_latent, 512) and arrays['w'].dtype == np.float32
    assert all(arrays[k].shape == (2,) for k in ('pix', 'pix_opt', 'reg', 'index', 'split'))
    assert [arrays['noise_%d' % i].shape for i in range(G.num_layers)] == [(2, 1, r, r) for r in (4, 8, 8, 16, 16, 32, 32)]
    assert np.all(np.isfinite(arrays['pix'])) and np.all(arrays['pix'] > 0)
    assert png_reader.read_png(str(outs[0] / 'project_5.png')).shape == recover.figure_shape(1, 32, 32)
    # the walk between the two projected codes: the ends of the row are the codes' own images
    paths = test_gan_walk.main([str(outs[0] / 'gen_ema.pt'), 'stylegan2', '--latents', str(outs[0] / 'project_5.npz'), '--steps', '4',
                                '--seed', '5'])
    assert paths == [str(outs[0] / 'walk_5.png')]
    sheet = png_reader.read_png(paths[0])
    assert sheet.shape == (34 + 2, 4 * 34 + 2, 3)
    codes = torch.from_numpy(arrays['w']).cuda()
    with torch.no_grad(), latent.preserved_rng('cuda'):
        noise = latent.shared_noise(G, 5, 'cuda')
        ends = latent.images_of(G, codes[[0, 0, 1, 1]].contiguous(), 'w', noise)
        want = ops.image_grid_u8(ends, nrow=4, padding=2).cpu().numpy()
    assert np.array_equal(sheet[:, :36], want[:, :36]) and np.array_equal(sheet[:, -36:], want[:, -36:])
    assert not np.array_equal(sheet[2:34, 36:68], sheet[2:34, 2:34])
