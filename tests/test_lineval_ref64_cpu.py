"""Linear evaluation without a GPU: the float64 head of tests/linhead_ref64.py reproduces the reference's own
arithmetic (tests/golden/lineval.npz, written by tests/golden/make_golden_lineval.py), and the host-side pieces of
contrad_amd.lineval / contrad_amd.evaluate behave as the reference's do."""
import json
import os

import numpy as np
import pytest
import torch

import linhead_ref64 as R
from contrad_amd import _lib, lineval
from contrad_amd.evaluate import AverageMeter
from contrad_amd.evaluate.classifier import accuracy, error_k
from contrad_amd.models.gan import get_architecture
from contrad_amd.models.gan.base import LinearWrapper

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-12


def _case(golden, C):
    z = golden('lineval')
    return {k[len('c%d.' % C):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c%d.' % C)}


@pytest.mark.parametrize('C', [10, 100])
def test_ref64_reproduces_the_reference_trajectory(golden, C):
    g = _case(golden, C)
    W, b, N = g['W0'], g['b0'], g['X'].shape[0]
    kept = g['logits_iters'].tolist()
    for it in range(len(g['loss'])):
        out = R.head_ref64(g['X'], W, b, g['y'], lr=float(g['lr'][it]))
        if it in kept:
            assert (out['logits'] - g['logits'][kept.index(it)]).abs().max().item() < TOL
        assert abs(out['loss'].item() - g['loss'][it].item()) < TOL
        assert abs(out['hits1'].sum().item() * 100.0 / N - g['acc1'][it].item()) < 1e-5      # (acc@1 went through float32)
        assert abs(out['hits5'].sum().item() * 100.0 / N - g['acc5'][it].item()) < 1e-9
        W, b = out['W'], out['b']
    assert (W - g['state_dict.weight']).abs().max().item() < TOL
    assert (b - g['state_dict.bias']).abs().max().item() < TOL
    assert g['lr'].tolist() == pytest.approx([0.1, 0.1, 0.1, 0.01, 0.01, 0.001, 0.001], rel=1e-12)


@pytest.mark.parametrize('C', [10, 100])
def test_accuracy_and_average_meter_equal_the_fixture(golden, C):
    g = _case(golden, C)
    kept = g['logits_iters'].tolist()
    N = g['X'].shape[0]
    for j, it in enumerate(kept):
        a1, a5 = accuracy(g['logits'][j], g['y'], topk=(1, 5))
        assert a1.shape == (1,) and a5.shape == (1,)
        assert abs(a1.item() - g['acc1'][it].item()) < 1e-5 and abs(a5.item() - g['acc5'][it].item()) < 1e-5
        e1, = error_k(g['logits'][j], g['y'], ks=(1,))
        assert abs(e1.item() - (100.0 - g['acc1'][it].item())) < 1e-5
    m_loss, m_top1, m_top5 = AverageMeter(), AverageMeter(), AverageMeter()
    for it in range(len(g['loss'])):
        m_loss.update(g['loss'][it].item(), N); m_top1.update(g['acc1'][it].item(), N); m_top5.update(g['acc5'][it].item(), N)
    assert [m_loss.average, m_top1.average, m_top5.average] == pytest.approx(g['avg'].tolist(), rel=1e-13)
    assert m_loss.count == N * len(g['loss']) and m_loss.value == g['loss'][-1].item()


def test_strictly_greater_rule_on_exact_ties():
    out = torch.tensor([[1.0, 1.0, 0.5, 0.2, 0.1, 0.0, -1.0], [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.9]])
    a1, a5 = accuracy(out, torch.tensor([1, 5]), topk=(1, 5))
    assert a1.item() == 50.0 and a5.item() == 100.0         # a tie with the maximum is a hit; five equal logits below one
    r = R.head_ref64(torch.eye(2), out.t().contiguous(), torch.zeros(7), torch.tensor([1, 5]))
    assert r['hits1'].tolist() == [1.0, 0.0] and r['hits5'].tolist() == [1.0, 1.0]


def test_linear_wrapper_is_the_reference_head(golden):
    g = _case(golden, 10)
    head = LinearWrapper(512, 10)
    assert list(head.state_dict().keys()) == ['weight', 'bias']
    head.load_state_dict({'weight': g['state_dict.weight'].float(), 'bias': g['state_dict.bias'].float()})
    x = g['X'].float()
    assert torch.equal(head(x, None), torch.nn.functional.linear(x, head.weight, head.bias))
    torch.manual_seed(7); a = LinearWrapper(64, 5)
    torch.manual_seed(7); b = torch.nn.Linear(64, 5)           # nn.Linear's default init from the host RNG
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)


@pytest.mark.parametrize('arch', ['sndcgan', 'snresnet18', 'stylegan2'])
def test_checkpoint_key_list_is_manifest_plus_linear(arch):
    manifest = json.load(open(os.path.join(GOLDEN, 'checkpoint_manifest.json')))
    _, D = get_architecture(arch, (32, 32, 3))
    want = list(D.state_dict().keys())
    if arch in manifest:                                     # (the manifest lists the reference's sndcgan and stylegan2)
        assert want == [k for k, _shape, _dt in manifest[arch]['dis']]
    lineval.install_head(D, 10)
    keys = lineval.checkpoint_keys(D)
    trunk = [k for k in want if not k.startswith('linear.')]
    assert [k for k in keys if not k.startswith('linear.')] == trunk
    assert [k for k in keys if k.startswith('linear.')] == ['linear.weight', 'linear.bias']
    assert tuple(D.state_dict()['linear.weight'].shape) == (10, D.d_penul)
    # a reference-format file ({'epoch', 'state_dict'} with the head under linear.*) loads into a fresh D + head
    _, D2 = get_architecture(arch, (32, 32, 3))
    lineval.install_head(D2, 10)
    D2.load_state_dict({k: v.clone() for k, v in D.state_dict().items()})
    assert torch.equal(D2.linear.weight, D.linear.weight)


def test_npz_reader_and_synthetic_set_are_deterministic(tmp_path):
    a, b, c = lineval.synthetic_set(5, 10, 300, 100), lineval.synthetic_set(5, 10, 300, 100), lineval.synthetic_set(6, 10, 300, 100)
    for k in ('x_train', 'y_train', 'x_test', 'y_test'):
        assert np.array_equal(a[k], b[k])
    assert not np.array_equal(a['x_train'], c['x_train'])
    assert a['x_train'].dtype == np.uint8 and a['x_train'].shape == (300, 32, 32, 3) and a['y_test'].dtype == np.int64
    # learnable: the class means of the training images tell the test images' classes apart
    means = np.stack([a['x_train'][a['y_train'] == k].mean(0) for k in range(10)]).reshape(10, -1)
    d = ((a['x_test'].reshape(100, 1, -1).astype(np.float32) - means[None]) ** 2).sum(2)
    assert (d.argmin(1) == a['y_test']).mean() > 0.9
    path = str(tmp_path / 'set.npz')
    np.savez(path, x_train=a['x_train'], y_train=a['y_train'].astype(np.int32).reshape(-1, 1), x_test=a['x_test'], y_test=a['y_test'])
    r1, r2 = lineval.load_npz(path), lineval.load_npz(path)
    assert np.array_equal(r1['x_train'], a['x_train']) and np.array_equal(r1['y_train'], a['y_train']) and r1['y_train'].dtype == np.int64
    assert all(np.array_equal(r1[k], r2[k]) for k in r1)
    np.savez(path, x_train=a['x_train'].astype(np.float32), y_train=a['y_train'], x_test=a['x_test'], y_test=a['y_test'])
    with pytest.raises(ValueError):
        lineval.load_npz(path)


def test_lr_schedule_and_cli():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, gamma=0.1, milestones=[60, 75, 90])
    for epoch in range(100):
        assert lineval.lr_at(epoch) == pytest.approx(opt.param_groups[0]['lr'], rel=1e-12)
        opt.step(); sched.step()
    P = lineval.parse_args(['run/dis.pt', 'sndcgan'])
    assert (P.n_classes, P.batch_size, P.epochs, P.graph, P.synthetic) == (10, 256, 100, False, False)
    with pytest.raises(SystemExit):
        lineval.parse_args(['run/dis.pt', 'sndcgan', '--world-size', '2'])
    assert lineval.CSV_HEADER == 'epoch,time,lr,train loss,train acc,test loss,test acc'


def test_header_declares_the_head():
    protos = _lib.parse_header()
    for name in ('contrad_linhead_workspace_bytes', 'contrad_linhead_plan', 'contrad_linhead_fwd', 'contrad_linhead_wgrad_sgd'):
        assert name in protos
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.lib()
    assert lib.raw('contrad_abi_version')() == 3
    assert lib.raw('contrad_linhead_workspace_bytes')(256, 8192, 129) < 0
    assert lib.raw('contrad_linhead_workspace_bytes')(256, 8192, 100) >= 4 * 256 * 100
