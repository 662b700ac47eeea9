#!/usr/bin/env python
"""Generate tests/golden/lineval.npz: the reference's linear-evaluation arithmetic on seeded features.

Runs ONLY in the build container (imports the read-only reference through _refshim.py).  Per class count (10, 100) it
runs the reference's ``LinearWrapper``, ``CrossEntropyLoss``, ``torch.optim.SGD(lr=0.1)`` + ``MultiStepLR``,
``accuracy`` (top-1; top-5 straight from ``torch.topk``, see run()) and ``AverageMeter`` in float64 for seven iterations across two milestones on a fixed
learnable batch (N = 48, K = 512) and stores inputs, per-iteration loss / acc@1 / acc@5, logits (every iteration at C = 10, first and last at C = 100), the running
averages, the learning rates and the final ``state_dict``.  Data only; the reference never travels.

    python tests/golden/make_golden_lineval.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402

_refshim.install()


def _load(name, rel):
    """Import one reference source file by path (fallback when its package pulls in something the shim lacks)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(_refshim.REFERENCE_ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


try:
    from models.gan.base import LinearWrapper
except Exception:                                   # noqa: BLE001
    LinearWrapper = _load('_ref_base', 'models/gan/base.py').LinearWrapper
try:
    from evaluate import AverageMeter
    from evaluate.classifier import accuracy
except Exception:                                   # noqa: BLE001
    AverageMeter = _load('evaluate', 'evaluate/__init__.py').AverageMeter
    sys.modules['evaluate'] = sys.modules.get('evaluate') or _load('evaluate', 'evaluate/__init__.py')
    accuracy = _load('_ref_classifier', 'evaluate/classifier.py').accuracy

N, K, ITERS, MILESTONES = 48, 512, 7, [3, 5]


def run(C, seed):
    g = torch.Generator().manual_seed(seed)
    # inputs and initial weights are float32-representable float64 (half the bytes after compression: the fixture must
    # stay under the size limit for committed files); everything computed from them is full float64
    X = (torch.randn(N, K, generator=g, dtype=torch.float64).relu() * 4 / K ** 0.5).float().double()
    y = ((X - X.mean(0)) @ torch.randn(C, K, generator=g, dtype=torch.float64).t()).argmax(1)
    torch.manual_seed(seed)
    head = LinearWrapper(K, C).double()              # (drawn in float32, then widened)
    out = {'X': X, 'y': y, 'W0': head.weight.detach().clone(), 'b0': head.bias.detach().clone()}
    opt = torch.optim.SGD(head.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, gamma=0.1, milestones=MILESTONES)
    crit = torch.nn.CrossEntropyLoss()
    m_loss, m_top1, m_top5 = AverageMeter(), AverageMeter(), AverageMeter()
    logits, losses, acc1s, acc5s, lrs = [], [], [], [], []
    for _ in range(ITERS):
        lrs.append(opt.param_groups[0]['lr'])
        o = head(X)
        loss = crit(o, y)
        a1, = accuracy(o, y, topk=(1,))
        # accuracy() cannot run for k > 1 on this torch (its view(-1) of a transposed comparison raises), so acc@5 comes
        # from the torch.topk call it is built on
        a5 = (o.detach().topk(5, 1).indices == y.view(-1, 1)).any(1).double().sum() * (100.0 / N)
        m_loss.update(loss.item(), N); m_top1.update(a1.item(), N); m_top5.update(a5.item(), N)
        opt.zero_grad(); loss.backward(); opt.step(); sched.step()
        logits.append(o.detach().clone()); losses.append(loss.item()); acc1s.append(a1.item()); acc5s.append(a5.item())
    keep = list(range(ITERS)) if C <= 10 else [0, ITERS - 1]         # (size limit: C = 100 keeps the first and last iteration)
    out.update(logits=torch.stack([logits[i] for i in keep]), logits_iters=torch.tensor(keep), loss=torch.tensor(losses, dtype=torch.float64),
               acc1=torch.tensor(acc1s, dtype=torch.float64), acc5=torch.tensor(acc5s, dtype=torch.float64),
               lr=torch.tensor(lrs, dtype=torch.float64),
               avg=torch.tensor([m_loss.average, m_top1.average, m_top5.average], dtype=torch.float64))
    for k, v in head.state_dict().items():
        out['state_dict.' + k] = v.detach().clone()
    return out


def main():
    blob = {}
    for C, seed in ((10, 101), (100, 102)):
        for k, v in run(C, seed).items():
            blob['c%d.%s' % (C, k)] = v.numpy()
    path = os.path.join(HERE, 'lineval.npz')
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
