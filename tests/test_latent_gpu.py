"""contrad_amd/latent.py and the generator's latent methods on the GPU: StyleGAN2 at 32 x 32 with random weights (B = 4) and
SNDCGAN at 32 x 32 for the z-space cases.  The networks are not under test here (their parity modules are); what is, is the
plumbing around them: which latents reach G, the shared noise, the scale, the filter and the pairing of the path length, the
command lines and the training hook.

Observed on the MI355X: profiles/ppl.txt."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import latent_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GINS = {'sndcgan': ('gan', 'cifar10', 'c10_b64.gin'), 'stylegan2': ('gan', 'stylegan2', 'c10_style64.gin')}
B = 4
_nets = {}


def _networks(arch):
    """(G, E) of ``arch`` at 32 x 32 with seeded random weights, on the GPU, frozen; made once."""
    if arch not in _nets:
        from contrad_amd.evaluate.gan import freeze
        from contrad_amd.models.gan import get_architecture
        torch.manual_seed(31)
        G, D = get_architecture(arch, (32, 32, 3))
        _nets[arch] = (freeze(G.cuda()), freeze(D.cuda()))
    return _nets[arch]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _z(seed=0):
    return torch.randn(B, 512, generator=torch.Generator().manual_seed(seed)).cuda()


# ---- the generator's three methods ----
def test_get_latent_is_the_mapping_network_of_forward():
    G, _ = _networks('stylegan2')
    z = _z()
    with torch.no_grad():
        w = G.get_latent(z)
        _img, latents = G(z, return_latents=True)
    assert tuple(w.shape) == (B, 512) and tuple(latents.shape) == (B, G.n_latent, 512)
    assert np.array_equal(_bits(w), _bits(latents[:, 0]))
    with pytest.raises(RuntimeError):
        G.get_latent(z.cpu())


def test_make_noise_has_the_reference_shapes():
    G, _ = _networks('stylegan2')
    noise = G.make_noise()
    assert len(noise) == G.num_layers == 7
    assert [tuple(n.shape) for n in noise] == [(1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)) for i in range(7)]
    assert [n.shape[-1] for n in noise] == [4, 8, 8, 16, 16, 32, 32] and all(n.is_cuda and n.dtype == torch.float32 for n in noise)


def test_mean_latent_is_the_float64_mean_rounded_once():
    G, _ = _networks('stylegan2')
    torch.manual_seed(9)
    got = G.mean_latent(64)
    torch.manual_seed(9)
    z = torch.randn(64, 512, device='cuda')                           # the reference's draw
    with torch.no_grad():
        w = G.get_latent(z)
    want = w.cpu().numpy().astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32)
    assert tuple(got.shape) == (1, 512) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)


# ---- truncation and mixing at one shared noise list ----
def test_truncation_and_mixing_ends_are_bitwise():
    from contrad_amd import latent
    G, _ = _networks('stylegan2')
    z, z2 = _z(1), _z(2)
    torch.manual_seed(3)
    noise = G.make_noise()
    w_avg = G.mean_latent(64)
    with torch.no_grad():
        plain = G(z, noise=noise)
        one = G(latent.truncated(G, z, 1.0, w_avg), input_is_latent=True, noise=noise)
        assert np.array_equal(_bits(one), _bits(plain))               # psi = 1: G(z)
        zero = G(latent.truncated(G, z, 0.0, w_avg), input_is_latent=True, noise=noise)
        centre = G(w_avg.expand(B, -1).contiguous(), input_is_latent=True, noise=noise)
        assert np.array_equal(_bits(zero), _bits(centre))             # psi = 0: the mean's image, B times
        assert np.array_equal(_bits(zero[0]), _bits(zero[B - 1])) and not np.array_equal(_bits(zero), _bits(plain))
        unmixed = G(latent.mixed(G, z, z2, G.n_latent), input_is_latent=True, noise=noise)
        assert np.array_equal(_bits(unmixed), _bits(plain))           # cross = n_latent: unmixed
        other = G(latent.mixed(G, z, z2, 0), input_is_latent=True, noise=noise)
        assert np.array_equal(_bits(other), _bits(G(z2, noise=noise)))
        styles = latent.mixed(G, z, z2, [0, 2, 4, G.n_latent])
        wa, wb = G.get_latent(z), G.get_latent(z2)
        assert np.array_equal(_bits(styles[1, :2]), _bits(wa[1:2].expand(2, -1))) and np.array_equal(_bits(styles[1, 2]), _bits(wb[1]))
        half = latent.truncated(G, z, 0.5, w_avg, cutoff=2)           # the layers behind the cutoff are w itself
        assert np.array_equal(_bits(half[:, 2:]), _bits(wa[:, None].expand(-1, G.n_latent - 2, -1)))
        assert not np.array_equal(_bits(half[:, 0]), _bits(wa))
    with pytest.raises(ValueError):
        latent.truncated(G, z, 0.5, None)
    with pytest.raises(ValueError):
        latent.mixed(G, z, z2, G.n_latent + 1)
    S, _ = _networks('sndcgan')
    with pytest.raises(ValueError, match='no W'):
        latent.truncated(S, torch.zeros(B, 128, device='cuda'), 0.5, w_avg)


def test_pairs_are_eps_apart_on_the_right_path():
    from contrad_amd import latent
    from contrad_amd.evaluate.gan import fixed_latent
    G, _ = _networks('stylegan2')
    S, _ = _networks('sndcgan')
    for net, mode in ((G, 1), (S, 0)):
        x0, x1, t = latent.pairs(net, 6, 11, 'z', 'full', 1e-4)
        z = fixed_latent(net, 12, 11).cpu().numpy()
        a, b = z[:6], z[6:]
        t = t.cpu().numpy()
        assert np.all((0.0 <= t) & (t < 1.0)) and len(np.unique(t)) == 6
        w0, w1 = R.pair(a.astype(np.float64), b.astype(np.float64), t, 1e-4, mode)
        for got, want in ((x0, w0), (x1, w1)):
            assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - want) <= R.pair_bound(want, a, b))
        e0, e1, te = latent.pairs(net, 6, 11, 'z', 'end', 1e-4)
        assert not te.any() and not np.array_equal(_bits(e0), _bits(e1))
    cube = latent.pairs(S, 6, 11)[0].cpu().numpy()
    assert np.abs(cube).max() <= 1.0                                  # lerp stays in the uniform cube
    w0, w1, _t = latent.pairs(G, 6, 11, 'w', 'end', 1e-4)
    with torch.no_grad():
        wa, wb = G.get_latent(fixed_latent(G, 12, 11)[:6]), G.get_latent(fixed_latent(G, 12, 11)[6:])
    assert np.array_equal(_bits(w0), _bits(wa))                       # t = 0 in W: the first endpoint's w
    want = wa.double() + 1e-4 * (wb.double() - wa.double())
    assert float((w1.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    with pytest.raises(ValueError, match='no W'):
        latent.pairs(S, 6, 11, 'w')


# ---- path length ----
@pytest.mark.parametrize('arch,space,sampling', [('stylegan2', 'z', 'full'), ('stylegan2', 'w', 'end'), ('sndcgan', 'z', 'full')])
def test_ppl_of_is_the_oracles_assembly_of_the_devices_rows(margin, arch, space, sampling):
    from contrad_amd import latent
    G, E = _networks(arch)
    n, seed, eps = 128, 5, 1e-4
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    out = latent.ppl_of(G, E, n, seed, space, sampling, eps, batch=32)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert sorted(out) == sorted(['ppl', 'ppl_raw', 'kept', 'n', 'eps', 'space', 'sampling', 'seed', 'note'])
    assert (out['n'], out['eps'], out['space'], out['sampling'], out['seed']) == (n, eps, space, sampling, seed)
    f0, f1 = latent.pair_features(G, E, n, seed, space, sampling, eps, batch=32)
    assert f0.shape[0] == n and tuple(f0.shape) == tuple(f1.shape) and not np.array_equal(_bits(f0), _bits(f1))
    f0, f1 = f0.cpu().numpy(), f1.cpu().numpy()
    ppl, raw, kept, d = R.ppl(f0, f1, eps)
    bound = R.pair_dist_bound(d, f0.shape[1], 1.0 / (eps * eps))
    lo, hi = np.percentile(d, 1, method='lower'), np.percentile(d, 99, method='higher')
    keep = (lo <= d) & (d <= hi)
    print('ppl %s %s/%s: %.6g (raw %.6g, kept %d), yardstick %.6g; mean bound %.3g' % (arch, space, sampling, out['ppl'], out['ppl_raw'],
                                                                                        out['kept'], ppl, bound.mean()))
    assert out['kept'] == kept == int(keep.sum()) and kept in (126, 127, 128) and np.isfinite(ppl) and ppl > 0.0
    sum_slack = n * 2.0 ** -53 * abs(raw)                             # the two means' own float64 sums
    margin('ppl_of %s %s/%s' % (arch, space, sampling), abs(out['ppl'] - ppl), bound[keep].mean() + sum_slack)
    margin('ppl_raw %s %s/%s' % (arch, space, sampling), abs(out['ppl_raw'] - raw), bound.mean() + sum_slack)
    again = latent.ppl_of(G, E, n, seed, space, sampling, eps, batch=32)
    assert again == out                                               # a rerun gives the same bits
    other = latent.ppl_of(G, E, n, seed + 1, space, sampling, eps, batch=32)
    assert other['ppl'] != out['ppl']


def test_ppl_of_refusals():
    from contrad_amd import latent
    G, E = _networks('sndcgan')
    for kw in (dict(n=99), dict(eps=0.0), dict(eps=-1e-4), dict(sampling='middle'), dict(batch=0), dict(space='w')):
        with pytest.raises(ValueError):
            latent.ppl_of(G, E, **dict(dict(n=128, seed=0), **kw))
    G.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            latent.ppl_of(G, E, 128, 0)
    finally:
        G.eval()


# ---- the command lines ----
def _run_dir(tmp_path, arch):
    from contrad_amd import config
    G, E = _networks(arch)
    torch.save(G.state_dict(), str(tmp_path / 'gen.pt'))
    torch.save(E.state_dict(), str(tmp_path / 'dis.pt'))
    shutil.copy(os.path.join(config.CONFIG_ROOT, *GINS[arch]), str(tmp_path / GINS[arch][-1]))
    return str(tmp_path / 'gen.pt'), str(tmp_path / 'dis.pt')


def test_ppl_command_line_writes_the_json(tmp_path):
    import test_ppl
    from contrad_amd import latent
    gen, enc = _run_dir(tmp_path, 'stylegan2')
    path = test_ppl.main([gen, 'stylegan2', '--encoder', enc, '--n', '128', '--space', 'w', '--sampling', 'end', '--batch_size', '32',
                          '--seed', '5'])
    assert path == str(tmp_path / 'ppl_w_5.json')
    with open(path) as f:
        out = json.load(f)
    G, E = _networks('stylegan2')
    assert out == latent.ppl_of(G, E, 128, 5, 'w', 'end', 1e-4, batch=32)
    assert out['eps'] == 1e-4 and 'LPIPS' in out['note']


def test_walk_command_line_writes_the_sheets(tmp_path):
    import png_reader
    import test_gan_walk
    from contrad_amd import latent
    gen, _enc = _run_dir(tmp_path, 'stylegan2')
    paths = test_gan_walk.main([gen, 'stylegan2', '--pairs', '3', '--steps', '5', '--mix', '--cross', '4', '--truncation', '0.7',
                                '--truncation_n', '64', '--seed', '2'])
    assert paths == [str(tmp_path / 'walk_2.png'), str(tmp_path / 'mix_2.png')]
    walk, mix = png_reader.read_png(paths[0]), png_reader.read_png(paths[1])
    assert walk.shape == (3 * 34 + 2, 5 * 34 + 2, 3) and mix.shape == (5 * 34 + 2, 7 * 34 + 2, 3)
    assert not mix[2:34, 2:34].any() and mix[2:34, 36:68].any()      # the corner cell is black, the sources are not
    assert len(np.unique(walk)) > 2
    G, _ = _networks('stylegan2')
    plain = latent.walk_sheet(G, 3, 5, 2).cpu().numpy()               # without truncation: columns 0 and 4 are the endpoints
    from contrad_amd.evaluate.gan import fixed_latent
    from contrad_amd.hostio import to_uint8
    with torch.no_grad(), latent.preserved_rng('cuda'):
        noise = latent.shared_noise(G, 2, 'cuda')
        ends = to_uint8(G(fixed_latent(G, 6, 2), noise=noise)).permute(0, 2, 3, 1).cpu().numpy()
    for p in range(3):                                                # (slerp hands G the normalised z: one grey level at most)
        for col, end in ((0, ends[p]), (4, ends[3 + p])):
            cell = plain[2 + 34 * p:34 + 34 * p, 2 + 34 * col:34 + 34 * col].astype(np.int32)
            assert np.abs(cell - end.astype(np.int32)).max() <= 1
    sgen = tmp_path / 's'
    sgen.mkdir()
    gen, _enc = _run_dir(sgen, 'sndcgan')
    paths = test_gan_walk.main([gen, 'sndcgan', '--pairs', '2', '--steps', '4', '--seed', '2'])
    assert paths == [str(sgen / 'walk_2.png')] and png_reader.read_png(paths[0]).shape == (2 * 34 + 2, 4 * 34 + 2, 3)
    assert not os.path.exists(str(sgen / 'mix_2.png'))


def test_sampling_with_truncation(tmp_path):
    from contrad_amd import latent, sample
    from contrad_amd.hostio import to_uint8
    gen, _enc = _run_dir(tmp_path, 'stylegan2')
    out = sample.main([gen, 'stylegan2', '--n_samples', '6', '--batch_size', '4', '--seed', '3', '--truncation', '0.5',
                       '--truncation_n', '64', '--truncation_cutoff', '4'])
    assert out == str(tmp_path / 'samples_3_n6_psi0.5')
    got = np.load(os.path.join(out, 'samples.npz'))['images']
    G, _ = _networks('stylegan2')
    torch.manual_seed(3)
    with torch.no_grad():
        w_avg = G.mean_latent(64)
        floats = torch.cat([G(latent.truncated(G, G.sample_latent(4), 0.5, w_avg, 4), input_is_latent=True) for _ in range(2)])[:6]
    assert np.array_equal(got, to_uint8(floats).permute(0, 2, 3, 1).contiguous().cpu().numpy())
    plain = sample.main([gen, 'stylegan2', '--n_samples', '6', '--batch_size', '4', '--seed', '3'])
    assert plain == str(tmp_path / 'samples_3_n6')
    assert not np.array_equal(np.load(os.path.join(plain, 'samples.npz'))['images'], got)


# ---- the training hook ----
def test_hook_appends_the_rows_and_leaves_the_checkpoints_bitwise_alone(tmp_path_factory):
    import test_prdc_gpu as TP
    from contrad_amd import features, latent
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.train_gan import main
    plain = TP._run(tmp_path_factory, False, False)
    d = tmp_path_factory.mktemp('ppl_files')
    torch.save(TP._encoder(4)[1].state_dict(), str(d / 'enc.pt'))
    hooked = str(tmp_path_factory.mktemp('ppl_run'))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', hooked, '--ppl_encoder', str(d / 'enc.pt'), '--ppl_n', '128'])
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    assert not [f for f in os.listdir(plain) if f.startswith('ppl_')]
    assert sorted(f for f in os.listdir(hooked) if f.endswith('.csv')) == ['ppl_%d.csv' % TP.EVAL_SEED]
    with open(os.path.join(hooked, 'ppl_%d.csv' % TP.EVAL_SEED)) as f:
        lines = f.read().split()
    assert lines[0] == 'step,ppl,ppl_raw,kept' and len(lines) == 3
    dev = torch.device('cuda', 0)
    E = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[1], str(d / 'enc.pt'), dev)
    for line, (step, name) in zip(lines[1:], ((2, 'gen_2.pt'), (4, 'gen.pt'))):
        G = features.load_frozen(get_architecture('sndcgan', (32, 32, 3))[0], os.path.join(hooked, name), dev)
        out = latent.ppl_of(G, E, 128, TP.EVAL_SEED)
        assert line == latent.csv_line(step, out), (line, out)
        assert np.isfinite(out['ppl']) and out['ppl'] > 0.0
    for bad in (['--ppl_n', '128'], ['--ppl_encoder', str(d / 'enc.pt'), '--ppl_n', '99'], ['--ppl_encoder', str(d / 'enc.pt'), '--ppl_space', 'w']):
        with pytest.raises(ValueError):
            main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', hooked] + bad)
