"""Classifier metrics of the reference's ``evaluate/classifier.py`` (:11-25 accuracy, :28-41 error_k, :154-176
test_classifier) for the linear-evaluation head.

A label counts as a top-k hit when fewer than k logits are strictly greater than its own logit -- what ``torch.topk``
gives the reference whenever the logits of a row are distinct, and the rule the head kernel implements
(csrc/linhead.hip, launch 2).
"""
import torch

from .. import ops
from ..models.gan.base import LinearWrapper


def _hits(output, target, ks):
    own = output.gather(1, target.view(-1, 1))
    above = (output > own).sum(1)
    return [(above < k).sum().float() for k in ks]


def accuracy(output, target, topk=(1,)):
    """Top-k accuracies in percent, one 1-element tensor per k."""
    with torch.no_grad():
        scale = 100.0 / target.size(0)
        return [(h * scale).view(1) for h in _hits(output, target, topk)]


def error_k(output, target, ks=(1,)):
    """Top-k error rates in percent, one scalar tensor per k."""
    with torch.no_grad():
        scale = 100.0 / target.size(0)
        return [100.0 - h * scale for h in _hits(output, target, ks)]


_METRICS = ('loss', 'error@1', 'error@5')


def new_meters(device):
    """The device-resident meter block of the head kernels: float64 {loss sum, top-1 hits, top-5 hits, samples}."""
    return torch.zeros(4, dtype=torch.float64, device=device)


def summarize(meters4):
    """Host values of a meter block: THE device-to-host read of a pass over a loader."""
    loss, h1, h5, n = meters4.cpu().tolist()
    n = max(n, 1.0)
    return {'loss': loss / n, 'error@1': 100.0 - 100.0 * h1 / n, 'error@5': 100.0 - 100.0 * h5 / n,
            'acc@1': 100.0 * h1 / n, 'acc@5': 100.0 * h5 / n, 'count': n}


def test_classifier(cls, data_loader, metrics, augment_fn=None, adversary=None):
    """Mean cross-entropy and top-k error of ``cls`` (a discriminator whose ``linear`` is a LinearWrapper) over
    ``data_loader`` in eval mode: per batch the trunk forward and launches 1 + 2 of the head, the sums kept on the
    device, one read at the end.  Returns {metric: value} like the reference."""
    unknown = [m for m in metrics if m not in _METRICS]
    if unknown:
        raise NotImplementedError('metrics %s (implemented: %s)' % (unknown, list(_METRICS)))
    head = getattr(cls, 'linear', None)
    if not isinstance(head, LinearWrapper):
        raise NotImplementedError('test_classifier evaluates a discriminator with a LinearWrapper head')
    was_training = cls.training
    cls.eval()
    dev = head.weight.device
    meters = new_meters(dev)
    with torch.no_grad():
        for images, labels in data_loader:
            feats = cls.penultimate(images.to(dev))
            ops.linhead_fwd(feats, head.weight, head.bias, y=labels, meters=meters, want_logits=False)
    cls.train(was_training)
    out = summarize(meters)
    return {k: out[k] for k in metrics}


test_classifier.__test__ = False        # (the reference's name; not a pytest case)
