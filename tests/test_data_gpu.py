"""The real-image data path on the GPU: csrc/data.hip bitwise against ToTensor on the host, the DeviceLoader against the
index plan and replayed flips, and both training loops fed from an npz (``--data``)."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(9, 6, 32, 32), (3, 1, 8, 8), (70, 67, 8, 8), (4, 3, 5, 7), (3, 3, 66, 66), (2, 2, 2, 512)]   # (n, B, H, W)
OFFSETS = [(0, 0), (1, 1), (2, 1), (3, 1), (0, 1), (1, 0)]           # (src bytes off the 4-byte grid, dst floats off the 16-byte grid)
GUARD, SENTINEL = 8, -7.0


def _set(n, H, W, seed):
    x = np.random.RandomState(seed).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    flat = x.reshape(-1)
    flat[:min(256, flat.size)] = np.arange(min(256, flat.size), dtype=np.uint8)       # every byte value where there is room
    return x


def _host(x, idx, flips):
    """The host expression: ToTensor of x[idx], .flip(-1) on the flipped rows."""
    out = torch.from_numpy(x[np.asarray(idx)]).permute(0, 3, 1, 2).float().div(255)
    f = torch.as_tensor(np.asarray(flips, dtype=bool))
    out[f] = out[f].flip(-1)
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _param_blocks(n, B, seed):
    """Two blocks per shape: both hold index 0, index n - 1 and a repeated index as far as B allows, with mixed flips."""
    r = np.random.RandomState(seed).randint(0, n, B)
    a = np.concatenate([[0, n - 1, 0, n - 1], r])[:B]
    b = np.concatenate([[n - 1, 0, n - 1], r[::-1]])[:B]
    return [(a, np.arange(B) % 2 == 0), (b, np.arange(B) % 2 == 1)]


def _on_device(x, src_off, B, dst_off):
    """x in a uint8 buffer ``src_off`` bytes off the allocation's grid; an out view ``dst_off`` floats off it, inside a
    sentinel-filled buffer with guards on both sides."""
    n, H, W, _ = x.shape
    raw = torch.zeros(x.size + 8, dtype=torch.uint8, device=DEV)
    src = raw[src_off:src_off + x.size].view(n, H, W, 3)
    src.copy_(torch.from_numpy(x))
    numel = B * 3 * H * W
    big = torch.full((GUARD + dst_off + numel + GUARD,), SENTINEL, device=DEV)
    out = big[GUARD + dst_off:GUARD + dst_off + numel].view(B, 3, H, W)
    assert src.data_ptr() % 4 == src_off and out.data_ptr() % 16 == 4 * dst_off
    return src, big, out


@pytest.mark.parametrize('src_off,dst_off', OFFSETS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gather_is_bitwise_totensor(shape, src_off, dst_off):
    from contrad_amd import ops
    n, B, H, W = shape
    x = _set(n, H, W, seed=n + B)
    src, big, out = _on_device(x, src_off, B, dst_off)
    for idx, flips in _param_blocks(n, B, seed=H):
        params = torch.tensor(np.stack([idx, flips], 1), dtype=torch.float32, device=DEV)
        big.fill_(SENTINEL)
        got = ops.gather_u8_nchw(src, params, H, W, out=out)
        assert got.data_ptr() == out.data_ptr()
        first = _bits(out)
        assert torch.equal(first, _bits(_host(x, idx, flips))), (shape, src_off, dst_off)
        lo, hi = GUARD + dst_off, GUARD + dst_off + out.numel()
        assert bool((big[:lo] == SENTINEL).all()) and bool((big[hi:] == SENTINEL).all())
        big.fill_(SENTINEL)
        ops.gather_u8_nchw(src, params, H, W, out=out)           # a second call: the same bits
        assert torch.equal(_bits(out), first)


@pytest.mark.parametrize('shape', [(9, 6, 32, 32), (4, 3, 5, 7)], ids=['aligned', 'general'])
def test_gather_clamps_the_index(shape):
    """-1 and n give images 0 and n - 1; so does anything else outside [0, n) -- the kernel never reads outside src."""
    from contrad_amd import ops
    n, _, H, W = shape
    x = _set(n, H, W, seed=3)
    bad = [-1.0, float(n), -1e30, 1e30, float('-inf'), float('inf'), float('nan'), n - 0.5]
    want = [0, n - 1, 0, n - 1, 0, n - 1, 0, n - 1]
    flips = np.arange(len(bad)) % 2 == 1
    params = torch.tensor([[i, float(f)] for i, f in zip(bad, flips)], dtype=torch.float32, device=DEV)
    got = ops.gather_u8_nchw(torch.from_numpy(x).to(DEV), params, H, W)
    assert torch.equal(_bits(got), _bits(_host(x, want, flips)))


def test_gather_without_out_and_argument_checks():
    from contrad_amd import ops
    x = _set(5, 8, 8, seed=1)
    src = torch.from_numpy(x).to(DEV)
    params = torch.tensor([[4, 1], [2, 0]], dtype=torch.float32, device=DEV)
    got = ops.gather_u8_nchw(src, params, 8, 8)
    assert got.shape == (2, 3, 8, 8) and torch.equal(_bits(got), _bits(_host(x, [4, 2], [True, False])))
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src.float(), params, 8, 8)                            # float images
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src.permute(0, 3, 1, 2), params, 8, 8)                # [n, 3, H, W] view
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src, params, 8, 4)                                    # H, W of another set
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src, params.cpu(), 8, 8)
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src, torch.zeros(2, 3, device=DEV), 8, 8)             # not (B, 2)
    with pytest.raises(RuntimeError):
        ops.gather_u8_nchw(src, params, 8, 8, out=torch.empty(2, 8, 8, 3, device=DEV))
    with pytest.raises(NotImplementedError):                                     # 2^24 images: the float index is no longer exact
        ops.gather_u8_nchw(torch.empty(1 << 24, 1, 1, 3, dtype=torch.uint8, device=DEV), params, 1, 1)


# ---- loader ----
def _take(loader, k):
    return [next(loader)[0] for _ in range(k)]


def test_device_loader_follows_the_plan_and_the_seeded_flips():
    from contrad_amd.data import DeviceLoader, index_plan
    n, batch, world = 70, 16, 2
    x = _set(n, 32, 32, seed=11)
    for drop_last, per_epoch in ((False, 3), (True, 2)):             # 35 images per rank: 16 + 16 + 3
        for rank in range(world):
            runs = []
            for _ in range(2):
                torch.manual_seed(123 + rank)
                loader = DeviceLoader(x, batch, rank, world, flip=True, drop_last=drop_last, device=DEV)
                runs.append(_take(loader, 2 * per_epoch))
                assert loader.epoch == 1
            torch.manual_seed(123 + rank)                            # the flips, replayed: one draw per batch
            k = 0
            for epoch in range(2):
                plan = index_plan(n, batch, rank, world, epoch, drop_last)
                assert len(plan) == per_epoch
                for idx in plan:
                    flips = (torch.rand(len(idx)) < 0.5).numpy()
                    want = _bits(_host(x, idx, flips))
                    assert runs[0][k].shape == (len(idx), 3, 32, 32)
                    assert torch.equal(_bits(runs[0][k]), want), (drop_last, rank, epoch, k)
                    assert torch.equal(_bits(runs[1][k]), want)      # the same seed twice
                    k += 1


def test_flip_free_loader_draws_nothing():
    from contrad_amd.data import DeviceLoader, index_plan
    x = _set(70, 8, 8, seed=2)
    torch.manual_seed(9)
    state = torch.get_rng_state()
    loader = DeviceLoader(torch.from_numpy(x).to(DEV), 16, 1, 2, flip=False, drop_last=False)
    got = [next(loader) for _ in range(4)]
    assert torch.equal(torch.get_rng_state(), state)
    plan = index_plan(70, 16, 1, 2, 0, False) + index_plan(70, 16, 1, 2, 1, False)
    for (images, labels), idx in zip(got, plan):
        assert labels is None and torch.equal(_bits(images), _bits(_host(x, idx, np.zeros(len(idx), bool))))
    with pytest.raises(ValueError):
        DeviceLoader(x[:20], 16, 0, 2, flip=False, drop_last=True, device=DEV)     # 10 images per rank: never a full batch


# ---- the loops ----
def _losses(logdir):
    text = open(os.path.join(logdir, 'log.txt')).read()
    assert 'torchvision not available' not in text, text
    rows = re.findall(r'\[Steps\s+(\d+)\] \[G (\S+)\] \[D (\S+)\] \[pen (\S+)\]', text)
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    return [int(r[0]) for r in rows], vals


def test_train_gan_on_an_npz_eager_and_graphed(tmp_path):
    """train_gan.py --data: 128 CIFAR-shaped images, batch 64 -> two epochs in 4 steps; --graph writes the eager run's
    checkpoints bit for bit (the contract tests/test_graph_gpu.py pins for synthetic batches)."""
    from contrad_amd.train_gan import main
    npz = str(tmp_path / 'set.npz')
    np.savez(npz, x_train=_set(128, 32, 32, seed=4))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    states = []
    for tag, extra in (('eager', []), ('graph', ['--graph'])):
        logdir = str(tmp_path / tag)
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--data', npz, '--max_steps', '4', '--print_every', '2',
              '--evaluate_every', '4', '--seed', '5', '--logdir', logdir] + extra)
        steps, vals = _losses(logdir)
        assert steps == [2, 4] and np.isfinite(vals).all(), (steps, vals)
        for name in ('gen.pt', 'dis.pt', 'optim.pt'):
            assert os.path.exists(os.path.join(logdir, name)), name
        states.append({n: torch.load(os.path.join(logdir, n), map_location='cpu') for n in ('gen.pt', 'dis.pt')})
    for name in ('gen.pt', 'dis.pt'):
        a, b = states[0][name], states[1][name]
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
    assert 'drops each epoch' in open(os.path.join(str(tmp_path / 'graph'), 'log.txt')).read()


def test_train_stylegan2_contrad_on_an_npz(tmp_path):
    from contrad_amd.train_stylegan2_contraD import main
    npz = str(tmp_path / 'set.npz')
    np.savez(npz, x_train=_set(16, 32, 32, seed=6), y_train=np.arange(16) % 10)
    gin = os.path.join(ROOT, 'configs', 'gan', 'stylegan2', 'c10_style64.gin')      # cifar10_hflip: the loader flips
    logdir = str(tmp_path / 'run')
    main([gin, 'stylegan2', '--mode=contrad', '--aug=simclr', '--lbd_r1', '0.1', '--d_reg_every', '2', '--data', npz,
          '--batch_size', '8', '--halflife_k', '1', '--ema_start_k', '0', '--print_every', '1', '--max_steps', '2',
          '--evaluate_every', '2', '--seed', '5', '--logdir', logdir])
    steps, vals = _losses(logdir)
    assert steps == [1, 2] and np.isfinite(vals).all(), (steps, vals)
    assert os.path.exists(os.path.join(logdir, 'gen_ema.pt'))


def test_images_of_another_size_are_refused(tmp_path):
    from contrad_amd.train_gan import main
    npz = str(tmp_path / 'small.npz')
    np.savez(npz, x_train=_set(64, 8, 8, seed=1))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    with pytest.raises(ValueError, match=r'\(8, 8, 3\).*\(32, 32, 3\)'):
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--data', npz, '--max_steps', '1', '--logdir',
              str(tmp_path / 'run')])
