"""evaluate/gan.py's ``WeightsMonitor`` on the host, a tiny ``torch.nn.Linear`` standing in for the owned network: the csv
files (header once, a resumed run appends), what ``update`` does to the owned network and does not do to the shown one,
and the global random streams, which come back bit for bit whatever ``evaluate()`` draws or raises."""
import os

import numpy as np
import pytest
import torch

from contrad_amd.evaluate.gan import WeightsMonitor

HEAD = 'step,sum,drawn'


class _Sum(WeightsMonitor):
    """``evaluate()``: the sum of the owned weights, after a draw from each global stream."""

    def __init__(self, logdir, fail=False, files=(('sum_%d.csv', HEAD, lambda step, out: '%d,%.6f,%.6f' % (step, out['sum'], out['drawn'])),)):
        self.fail = fail
        net = torch.nn.Linear(3, 2)
        assert net.training and all(p.requires_grad for p in net.parameters())
        super().__init__(str(logdir), 'cpu', 5, net, files, which='D')

    def evaluate(self):
        drawn = float(torch.rand(1)) + float(np.random.rand())
        assert not torch.is_grad_enabled()
        if self.fail:
            raise RuntimeError('evaluate failed')
        return {'sum': float(sum(p.sum() for p in self.net.parameters())), 'drawn': drawn}


def _shown(value):
    shown = torch.nn.Linear(3, 2)
    with torch.no_grad():
        for p in shown.parameters():
            p.fill_(value)
    return shown.train()


def _streams():
    return torch.get_rng_state().clone(), np.random.get_state()


def _same_streams(before, after):
    assert torch.equal(before[0], after[0])
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]


def _lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_header_once_and_a_second_monitor_appends(tmp_path):
    eval_seed = int(np.random.RandomState(5).randint(10000))
    path = str(tmp_path / ('sum_%d.csv' % eval_seed))
    m = _Sum(tmp_path)
    assert m.eval_seed == eval_seed and [f[:2] for f in m.files] == [(path, HEAD)]
    assert _lines(path) == [HEAD]                                       # written on a fresh directory
    m.update(2, _shown(0.5))
    again = _Sum(tmp_path)                                              # a resumed run: the same directory
    assert _lines(path)[0] == HEAD and len(_lines(path)) == 2           # ... does not rewrite the header
    again.update(4, _shown(1.0))
    lines = _lines(path)
    assert lines[0] == HEAD and [ln.split(',')[0] for ln in lines[1:]] == ['2', '4'] and lines.count(HEAD) == 1
    assert [ln.split(',')[1] for ln in lines[1:]] == ['4.000000', '8.000000']     # 8 weights of 0.5, then of 1
    assert os.listdir(str(tmp_path)) == [os.path.basename(path)]


def test_update_loads_the_shown_weights_into_a_frozen_eval_network(tmp_path):
    m = _Sum(tmp_path)
    assert m.D is m.net and not m.net.training and not any(p.requires_grad for p in m.net.parameters())     # frozen at once
    shown = _shown(0.25)
    m.net.train()                                                       # whatever state it is found in
    out = m.update(2, shown)
    assert out['sum'] == 2.0 and m.lines == ['2,2.000000,%.6f' % out['drawn']]
    for name, value in shown.state_dict().items():
        assert torch.equal(m.net.state_dict()[name], value)
    assert not m.net.training and not any(p.requires_grad for p in m.net.parameters())
    assert shown.training and all(p.requires_grad for p in shown.parameters())     # the shown module is only read
    shown.eval()
    m.update(4, shown)
    assert not shown.training
    assert torch.is_grad_enabled()


def test_the_global_streams_come_back_bit_for_bit(tmp_path):
    m, shown = _Sum(tmp_path), _shown(0.5)                              # (a Linear draws its initial weights: built first)
    torch.manual_seed(11); np.random.seed(12)
    before = _streams()
    out = m.update(2, shown)
    _same_streams(before, _streams())
    torch.manual_seed(11); np.random.seed(12)
    assert out['drawn'] == float(torch.rand(1)) + float(np.random.rand())          # evaluate() did draw from both


def test_a_failing_evaluate_restores_the_streams_and_writes_no_row(tmp_path):
    two = (('a_%d.csv', HEAD, lambda step, out: '%d,%.6f,%.6f' % (step, out['sum'], out['drawn'])),
           ('b_%d.csv', 'step,none', lambda step, out: '%d,%s' % (step, out['missing'])))
    m, shown = _Sum(tmp_path, fail=True), _shown(0.5)
    torch.manual_seed(11); np.random.seed(12)
    before = _streams()
    with pytest.raises(RuntimeError, match='evaluate failed'):
        m.update(2, shown)
    _same_streams(before, _streams())
    assert _lines(m.files[0][0]) == [HEAD] and torch.is_grad_enabled()
    m2 = _Sum(tmp_path, files=two)                                      # a line that cannot be formed: no file gets a partial row
    with pytest.raises(KeyError):
        m2.update(2, _shown(0.5))
    assert [_lines(f[0]) for f in m2.files] == [[HEAD], ['step,none']]
