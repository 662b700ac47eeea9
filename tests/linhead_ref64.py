"""Float64 statement of the linear-evaluation head in plain torch (no project kernels): logits, mean cross-entropy,
dlogits, weight / bias gradients, the SGD update and the top-k hit rule.  The yardstick of tests/test_linhead_gpu.py,
tied to the reference's own arithmetic by tests/test_lineval_ref64_cpu.py."""
import torch


def head_ref64(F, W, b, y, lr=None, scale=None):
    """One iteration on features F[N, K], weights W[C, K], bias b[C], labels y[N] (entries outside [0, C) contribute
    loss 0, no hit and zero gradient but still count as samples).  Returns a dict of float64 tensors: logits, loss_rows,
    loss (sum over rows / N), dlogits (times ``scale``, default 1 / N), gradW, gradb, hits1 / hits5 (per-row 0 / 1) and,
    with ``lr``, the updated W and b."""
    F, W, b = F.double(), W.double(), b.double()
    N, C = F.shape[0], W.shape[0]
    scale = 1.0 / N if scale is None else scale
    logits = F @ W.t() + b
    ok = (y >= 0) & (y < C)
    ys = torch.where(ok, y, torch.zeros_like(y))
    m = logits.max(1, keepdim=True).values
    lse = (m + (logits - m).exp().sum(1, keepdim=True).log()).view(N)
    own = logits.gather(1, ys.view(N, 1))
    okd = ok.double()
    loss_rows = (lse - own.view(N)) * okd
    onehot = torch.zeros_like(logits).scatter_(1, ys.view(N, 1), 1.0)
    dlogits = ((logits - lse.view(N, 1)).exp() - onehot) * scale * okd.view(N, 1)
    above = (logits > own).sum(1)
    out = {'logits': logits, 'loss_rows': loss_rows, 'loss': loss_rows.sum() / N, 'dlogits': dlogits,
           'gradW': dlogits.t() @ F, 'gradb': dlogits.sum(0),
           'hits1': ((above < 1) & ok).double(), 'hits5': ((above < 5) & ok).double()}
    if lr is not None:
        out['W'], out['b'] = W - lr * out['gradW'], b - lr * out['gradb']
    return out


def near_tie_rows(logits, y, rel=1e-4):
    """Rows whose top-1 / top-5 verdict an fp32 evaluation may flip: the label's logit differs by less than
    ``rel * max|logit|`` (and by more than 0) from another logit ranked 1, 2, 5 or 6 (1-based, descending)."""
    N, C = logits.shape
    own = logits.gather(1, y.clamp(0, C - 1).view(N, 1))
    srt = logits.sort(1, descending=True).values
    ranks = [r for r in (0, 1, 4, 5) if r < C]
    d = (srt[:, ranks] - own).abs()
    tol = rel * logits.abs().max()
    return ((d > 0) & (d < tol)).any(1)
