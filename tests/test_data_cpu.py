"""Host side of the real-image data path (contrad_amd/data.py, tools/make_image_npz.py, the loops' ``--data`` flag): no GPU."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler
from torch.utils.data.distributed import DistributedSampler

from contrad_amd import _lib, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'make_image_npz.py')


# ---- index plan ----
@pytest.mark.parametrize('n', [7, 64, 70])
@pytest.mark.parametrize('world', [1, 2, 3])
def test_index_plan_is_torchs_samplers(n, world):
    for batch in (16, 64):
        for drop_last in (False, True):
            samplers = [DistributedSampler(range(n), num_replicas=world, rank=r, shuffle=True, seed=0) for r in range(world)]
            for epoch in range(3):
                seen = set()
                for rank, sampler in enumerate(samplers):
                    sampler.set_epoch(epoch)
                    want = list(BatchSampler(sampler, batch, drop_last))
                    got = data.index_plan(n, batch, rank, world, epoch, drop_last)
                    assert len(got) == len(want), (n, world, rank, batch, drop_last, epoch)
                    for g, w in zip(got, want):
                        assert g.dtype == np.int64 and g.tolist() == w
                    # the sampler's share itself (what drop_last=False batches cover)
                    share = data.index_plan(n, batch, rank, world, epoch, False)
                    assert np.concatenate(share).tolist() == list(sampler)
                    seen.update(np.concatenate(share).tolist())
                assert seen == set(range(n)), (n, world, epoch)


def test_index_plan_seed_and_epoch_change_the_order():
    a = np.concatenate(data.index_plan(70, 16, 0, 2, 0, False))
    assert not np.array_equal(a, np.concatenate(data.index_plan(70, 16, 0, 2, 1, False)))
    s = DistributedSampler(range(70), num_replicas=2, rank=0, shuffle=True, seed=5)
    s.set_epoch(2)
    assert np.concatenate(data.index_plan(70, 16, 0, 2, 2, False, seed=5)).tolist() == list(s)
    with pytest.raises(ValueError):
        data.index_plan(70, 16, 2, 2, 0, False)


# ---- reader ----
def _images(n, h=8, w=8, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def test_load_train_npz(tmp_path):
    x = _images(5)
    p = str(tmp_path / 'a.npz')
    np.savez(p, x_train=x)                                       # no labels, no test split
    got = data.load_train_npz(p)
    assert got['y_train'] is None and got['x_train'].dtype == np.uint8 and np.array_equal(got['x_train'], x)
    np.savez(p, x_train=x, y_train=np.arange(5).reshape(5, 1))
    assert data.load_train_npz(p)['y_train'].tolist() == [0, 1, 2, 3, 4]
    np.savez(p, x_train=x.astype(np.float32) / 255)
    with pytest.raises(ValueError, match='x_train'):
        data.load_train_npz(p)
    np.savez(p, x_train=np.ascontiguousarray(x.transpose(0, 3, 1, 2)))   # [n, 3, H, W]
    with pytest.raises(ValueError, match='x_train'):
        data.load_train_npz(p)
    np.savez(p, x_train=x, y_train=np.arange(4))
    with pytest.raises(ValueError, match='y_train'):
        data.load_train_npz(p)
    np.savez(p, x_test=x)
    with pytest.raises(ValueError, match='x_train'):
        data.load_train_npz(p)


# ---- converter ----
def _cifar_rows(seed):
    return np.random.RandomState(seed).randint(0, 256, (5, 3072)).astype(np.uint8)


def _check_rows(x, rows):
    assert x.dtype == np.uint8 and x.shape == (len(rows), 32, 32, 3)
    for c in range(3):
        for i in (0, 1, 17, 31):
            for j in (0, 2, 30, 31):
                assert (x[:, i, j, c] == rows[:, c * 1024 + i * 32 + j]).all()
    assert np.array_equal(x, rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))


def _run_tool(*args):
    r = subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_converter_cifar10_pickles(tmp_path):
    src = tmp_path / 'cifar-10-batches-py'
    src.mkdir()
    rows = {}
    for k, name in enumerate(['data_batch_1', 'data_batch_2', 'test_batch']):
        rows[name] = _cifar_rows(k)
        with open(str(src / name), 'wb') as f:
            pickle.dump({'data': rows[name], 'labels': [(k + i) % 10 for i in range(5)]}, f)
    out = str(tmp_path / 'c10.npz')
    _run_tool('cifar', str(src), out)
    z = np.load(out)
    _check_rows(z['x_train'], np.concatenate([rows['data_batch_1'], rows['data_batch_2']]))
    _check_rows(z['x_test'], rows['test_batch'])
    assert z['y_train'].tolist() == [0, 1, 2, 3, 4, 1, 2, 3, 4, 5] and z['y_test'].tolist() == [2, 3, 4, 5, 6]
    assert z['y_train'].dtype == np.int64
    got = data.load_train_npz(out)                               # the training reader takes the file as written
    assert np.array_equal(got['x_train'], z['x_train']) and got['y_train'].tolist() == z['y_train'].tolist()


def test_converter_cifar100_pickles(tmp_path):
    src = tmp_path / 'cifar-100-python'
    src.mkdir()
    rows = {'train': _cifar_rows(7), 'test': _cifar_rows(8)}
    for name in rows:
        with open(str(src / name), 'wb') as f:
            pickle.dump({'data': rows[name], 'fine_labels': [99, 0, 5, 7, 42], 'coarse_labels': [1] * 5}, f)
    out = str(tmp_path / 'c100.npz')
    _run_tool('cifar', str(src), out)
    z = np.load(out)
    _check_rows(z['x_train'], rows['train'])
    _check_rows(z['x_test'], rows['test'])
    assert z['y_train'].tolist() == [99, 0, 5, 7, 42]


def test_converter_image_folder(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    want = {}
    for split in ('train', 'test'):
        for label, cls in enumerate(['cat', 'dog']):
            d = tmp_path / 'set' / split / cls
            d.mkdir(parents=True)
            for k in range(2):
                img = _images(1, 6, 4, seed=10 * label + k + (100 if split == 'test' else 0))[0]     # H 6, W 4
                Image.fromarray(img).save(str(d / ('%d.png' % k)))
                want.setdefault(split, []).append((label, img))
    out = str(tmp_path / 'f.npz')
    _run_tool('folder', str(tmp_path / 'set'), out)
    z = np.load(out)
    for split in ('train', 'test'):
        assert z['x_' + split].shape == (4, 6, 4, 3) and z['x_' + split].dtype == np.uint8
        assert z['y_' + split].tolist() == [l for l, _ in want[split]]
        for got, (_, img) in zip(z['x_' + split], want[split]):
            assert np.array_equal(got, img)


# ---- parsers ----
def test_parsers_accept_data():
    from contrad_amd import train_gan, train_stylegan2
    assert train_gan.parse_args(['c.gin', 'sndcgan', '--data', 'x.npz']).data == 'x.npz'
    assert train_gan.parse_args(['c.gin', 'sndcgan']).data is None
    assert train_stylegan2.parse_args(['c.gin', 'stylegan2', '--data', 'x.npz']).data == 'x.npz'
    assert train_stylegan2.parse_args(['c.gin', 'stylegan2'], contrad_script=True).data is None


def test_flip_follows_the_reference_transforms():
    from contrad_amd import train_stylegan2
    flipped = sorted(k for k in train_stylegan2.IMAGE_SIZES if data.dataset_flips(k))
    assert flipped == ['afhq_cat', 'afhq_dog', 'afhq_wild', 'cifar100_hflip', 'cifar10_hflip']


# ---- ABI ----
def test_gather_argument_errors_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.lib()
    with pytest.raises(RuntimeError):
        lib.call('contrad_gather_u8_nchw', None, None, None, 4, 4, 8, 8, None)
    buf = torch.zeros(64)                                        # host memory: a valid pointer that must never be used
    p = buf.data_ptr()
    for (B, n, H, W) in ((0, 4, 8, 8), (-1, 4, 8, 8), (4, 0, 8, 8), (4, 4, 0, 8), (4, 4, 8, 0), (4, (1 << 24) + 1, 8, 8)):
        with pytest.raises(RuntimeError):
            lib.call('contrad_gather_u8_nchw', p, p, p, B, n, H, W, None)
