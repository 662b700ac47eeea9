"""The linear-evaluation loop end to end (test_lineval.py at the repository root) on the synthetic learnable set with
a freshly initialised, saved SNDCGAN discriminator: log format, learning, eager / --graph bit equality, checkpoint
round trip.  Every run is a fresh child process under its own time limit, one at a time."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from contrad_amd import lineval
from contrad_amd.evaluate.classifier import test_classifier as run_test_classifier
from contrad_amd.models.gan import get_architecture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, EPOCHS, SIZES, BATCH = 17, 3, ('3000', '1000'), 256           # 3000 = 11 x 256 + 184: a remainder batch per epoch
HEADER = ['epoch', 'time', 'lr', 'train loss', 'train acc', 'test loss', 'test acc']


def _run(logdir, *extra):
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'test_lineval.py'), os.path.join(logdir, 'dis.pt'),
           'sndcgan', '--synthetic', '--synthetic_size', SIZES[0], SIZES[1], '--seed', str(SEED), '--epochs', str(EPOCHS),
           '--batch_size', str(BATCH)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(logdir, 'lin_eval_%d.csv' % SEED)) as f:
        rows = list(csv.reader(f))
    ck = torch.load(os.path.join(logdir, 'lin_eval_%d.pth.tar' % SEED), map_location='cpu')
    init = json.load(open(os.path.join(logdir, 'lin_eval_%d.json' % SEED)))
    return rows, ck, init


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    out = {}
    torch.manual_seed(1)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    for name, extra in (('eager', ()), ('graph', ('--graph',))):
        d = str(tmp_path_factory.mktemp(name))
        torch.save(D.state_dict(), os.path.join(d, 'dis.pt'))
        out[name] = _run(d, *extra)
    return out


def test_log_and_learning(runs, margin):
    rows, ck, init = runs['eager']
    assert rows[0] == HEADER and len(rows) == 1 + EPOCHS
    assert [int(r[0]) for r in rows[1:]] == list(range(EPOCHS)) and all(float(r[2]) == 0.1 for r in rows[1:])
    train_loss = [float(r[3]) for r in rows[1:]]
    assert all(b < a for a, b in zip(train_loss, train_loss[1:])), train_loss
    # the yardstick is inside the run: the untrained head's accuracy on the same test set
    final_acc = float(rows[-1][6])
    margin('lineval untrained / final test accuracy', init['initial test acc'], final_acc)
    assert ck['epoch'] == EPOCHS


def test_eager_and_graph_checkpoints_are_bitwise_equal(runs):
    (_r0, a, _i0), (_r1, b, _i1) = runs['eager'], runs['graph']
    assert list(a['state_dict'].keys()) == list(b['state_dict'].keys())
    for k in a['state_dict']:
        assert torch.equal(a['state_dict'][k], b['state_dict'][k]), k
    assert [r[3:] for r in runs['eager'][0]] == [r[3:] for r in runs['graph'][0]]


def test_checkpoint_reloads_and_reproduces_the_logged_test_loss(runs, margin):
    rows, ck, _ = runs['eager']
    _, D = get_architecture('sndcgan', (32, 32, 3))
    lineval.install_head(D, 10)
    assert list(ck['state_dict'].keys()) == lineval.checkpoint_keys(D)
    D.load_state_dict(ck['state_dict'])
    D = D.to('cuda').eval()
    data = lineval.synthetic_set(SEED, 10, int(SIZES[0]), int(SIZES[1]))
    x, y = torch.from_numpy(data['x_test']).cuda(), torch.from_numpy(data['y_test']).cuda()
    res = run_test_classifier(D, lineval._batches(x, y, BATCH), ['loss', 'error@1'])
    logged = float(rows[-1][5])
    # the CSV keeps four significant digits ('{:.4}')
    margin('lineval reloaded / logged test loss', abs(res['loss'] - logged) / logged, 1e-3)
    assert abs((100 - res['error@1']) - float(rows[-1][6])) < 0.06


def test_reference_format_checkpoint_loads(golden):
    """A file in the reference's format: {'epoch', 'state_dict'} whose head is linear.weight / linear.bias (here the
    head the reference trained in tests/golden/lineval.npz, K = 512 = snresnet18's d_penul)."""
    z = golden('lineval')
    _, D = get_architecture('snresnet18', (32, 32, 3))
    sd = {k: v.clone() for k, v in D.state_dict().items() if not k.startswith('linear.')}
    sd['linear.weight'] = torch.from_numpy(z['c10.state_dict.weight']).float()
    sd['linear.bias'] = torch.from_numpy(z['c10.state_dict.bias']).float()
    lineval.install_head(D, 10)
    D.load_state_dict({'epoch': 7, 'state_dict': sd}['state_dict'])
    D = D.to('cuda').eval()
    X, y = torch.from_numpy(z['c10.X']).float().cuda(), torch.from_numpy(z['c10.y'])
    with torch.no_grad():
        out = D.linear(X)
    W, b = torch.from_numpy(z['c10.state_dict.weight']), torch.from_numpy(z['c10.state_dict.bias'])
    ref = torch.from_numpy(z['c10.X']) @ W.t() + b
    assert ((out.cpu().double() - ref).abs().max() / ref.abs().max()).item() < 5e-6
    assert np.array_equal(out.argmax(1).cpu().numpy(), ref.argmax(1).numpy())
