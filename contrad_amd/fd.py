"""The number the reference selects by, without its Inception network: the Frechet distance between generated images and
data in the feature space of a FROZEN discriminator, the space of contrad_amd/prdc.py and contrad_amd/kid.py (DESIGN.md
section 19).  The numbers are comparable only between evaluations made with the same encoder file, NEVER with the
Inception-based FID of papers.

    python test_fd.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_fd.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7

Features are ``D.penultimate`` in eval mode with L2-normalised rows (``features.extract_features``).  ``mu`` is the column
mean and ``Sigma = np.cov(rows, rowvar=False)`` (ddof 1), what the reference's ``compute_stats_*`` hand to
``calculate_frechet_distance``, and

    fd = ||mu_r - mu_f||^2 + tr Sigma_r + tr Sigma_f - 2 tr (Sigma_r Sigma_f)^(1/2)                  (not clamped)

No eigen-solver and no d x d covariance is formed.  With centred rows A = (R - mu_r) / sqrt(n_r - 1) and B = (F - mu_f) /
sqrt(n_f - 1), Sigma_r = A^T A and Sigma_f = B^T B, so

    tr (Sigma_r Sigma_f)^(1/2) = the sum of the singular values of A B^T = ||A B^T||_*

and ``M = Fc Rc^T`` is the cross-similarity GEMM of the centred rows on the conv engine.  Its nuclear norm is <U, M> with U
the polar factor of M, which the Newton-Schulz iteration approaches with GEMMs alone:

    X_0 = M / ||M||_F        X <- X (1.5 I - 0.5 X^T X)        estimate_k = <X_k, M>   (from below)

  * every GEMM: ``features.similarities`` in section 15's row chunks; M is kept [p][round_up(q, 4)] with p = max(n_r, n_f),
    q = min, so that the Gram matrix X^T X is the smaller one, q x q; padding columns stay zero;
  * csrc/kid.hip: ``ops.dot_sums`` -- the traces (sum of squares of the centred rows), ||M||_F^2 and every estimate, each
    product exact in float64, sums in float64, into one float64 device table;
  * ``n_iter`` is FIXED (default 60: only singular values below 1.5^-60 = 3e-11 of ||M||_F are not converged by then, and
    they contribute at most q times that); no adaptive stop, so there is ONE device-to-host read, of the table, and two
    runs take the same path.  Every division and the final combination are float64 on the host.

``--prdc_fd`` of the training scripts appends ``step,fd,mean_term,trace_fake,cross_term,tail`` to ``fd_<eval_seed>.csv`` at
every evaluation of the ``--prdc_data`` hook (the same frozen encoder, the same fakes, the real state made once).  It
records only: ``--prdc_best`` gains no choice.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import features, ops

N_ITER = 60
CSV_HEAD = 'step,fd,mean_term,trace_fake,cross_term,tail'
NOTE = ('Frechet distance ||mu_r - mu_f||^2 + tr S_r + tr S_f - 2 tr (S_r S_f)^(1/2) of the column means and np.cov covariances '
        '(ddof 1) of L2-normalised penultimate features of a frozen discriminator; the trace term is the nuclear norm of the '
        'cross-similarity matrix of the centred rows, by a fixed number of Newton-Schulz steps.  Comparable only between '
        'evaluations under one encoder file, never with Inception-based FID.')
TAIL_WARN = 1e-6                                                            # of estimates[-1]: the printed line warns above it
ROW_CHUNK = 4096                                                            # rows centred at a time (a float64 copy of them)


def check_sizes(n_real, n_fake, n_iter=N_ITER, dim=None):
    """The host refusals -> (p, q) = (max, min) of the two set sizes.  A covariance needs two rows; the conv engine takes
    operands below 2^31 elements, and X [p][round_up(q, 4)] is one (as is a bank [dim][round_up(q, 4)])."""
    if int(n_iter) < 1:
        raise ValueError('fd: n_iter must be at least 1, got %r' % (n_iter,))
    if n_real < 2 or n_fake < 2:
        raise ValueError('fd: a covariance (ddof 1) needs two rows of each set (%d real, %d fake)' % (n_real, n_fake))
    p, q = max(int(n_real), int(n_fake)), min(int(n_real), int(n_fake))
    if p * ops.round_up(q, 4) >= 1 << 31 or (dim is not None and int(dim) * ops.round_up(q, 4) >= 1 << 31):
        raise ValueError('fd: %d real and %d fake rows%s make a GEMM operand of 2^31 elements or more, which the conv engine '
                         'does not take' % (n_real, n_fake, '' if dim is None else ' of width %d' % dim))
    return p, q


def _feats(feats, what):
    if not torch.is_tensor(feats) or feats.dtype != torch.float32 or feats.dim() != 2:
        raise RuntimeError('fd: the %s features must be a CUDA float32 (n, d) matrix' % what)
    return feats.shape[0]


def _on_device(feats, what):
    if not feats.is_cuda:
        raise RuntimeError('fd: the %s features must be a CUDA float32 (n, d) matrix' % what)


def centred_rows(rows):
    """(rows - column mean rounded once to fp32, the column mean in float64 [d]) of CUDA fp32 rows [n, d]; the mean is
    accumulated in float64 (a torch reduction: plumbing, once per set)."""
    n = rows.shape[0]
    mu = rows.sum(0, dtype=torch.float64) / n
    out = torch.empty_like(rows)
    for i in range(0, n, ROW_CHUNK):
        out[i:i + ROW_CHUNK].copy_(rows[i:i + ROW_CHUNK].double() - mu)
    return out, mu


def real_state_of(bankT, n):
    """What the hook keeps of a real set between evaluations, from its transposed bank [d][round_up(n, 4)]
    (``features.bank_of`` of the normalised rows): ``bankT`` the centred bank (padding columns zero), ``mu`` the float64
    mean [d], ``sumsq`` a float64 device cell with the sum of squares of the centred rows (tr Sigma_r = sumsq / (n - 1),
    divided on the host with everything else) and ``n``."""
    if not torch.is_tensor(bankT) or bankT.dtype != torch.float32 or bankT.dim() != 2:
        raise RuntimeError('fd: the real bank must be a CUDA float32 [d][round_up(n, 4)] matrix')
    n = int(n)
    if n < 2:
        raise ValueError('fd: a covariance (ddof 1) needs two rows of each set (%d real)' % n)
    if bankT.shape[1] != ops.round_up(n, 4):
        raise RuntimeError('fd: a real bank of %s for %d rows' % (tuple(bankT.shape), n))
    _on_device(bankT, 'real')
    d = bankT.shape[0]
    mu = bankT[:, :n].sum(1, dtype=torch.float64) / n
    centred = features.new_bank(n, d, bankT.device)
    step = max(1, ROW_CHUNK * 64 // n)
    for i in range(0, d, step):
        centred[i:i + step, :n].copy_(bankT[i:i + step, :n].double() - mu[i:i + step, None])
    return SimpleNamespace(bankT=centred, mu=mu, sumsq=ops.dot_sums(centred, centred, n), n=n)


def gemm_rows(q, bankT, out):
    """out[m][n_pad] = q[m][d] bank^T, ``features.chunk_rows_of(n_pad)`` rows per launch (section 15's chunks), into the
    resident ``out``."""
    chunk = features.chunk_rows_of(bankT.shape[1])
    for i in range(0, q.shape[0], chunk):
        features.similarities(q[i:i + chunk], bankT, out[i:i + chunk])
    return out


def newton_schulz_step(X, XT, G, H, Xn, q):
    """One step on X [p][q_pad] -> Xn: XT [q, p] the transposed copy, G [q][q_pad] = X^T X (the bank is X itself), H
    [q_pad][q_pad] = 1.5 I - 0.5 G on the leading q x q block (zero elsewhere; H is symmetric, so it is its own bank), Xn = X H."""
    XT.copy_(X[:, :q].t())
    gemm_rows(XT, X, G)
    torch.mul(G, -0.5, out=H[:q])
    H[:q, :q].diagonal().add_(1.5)
    return gemm_rows(X, H, Xn)


def fd(real_feats, fake_feats, n_iter=N_ITER, normalize=True, real_state=None):
    """The Frechet distance of fake feature rows [n_f, d] from real ones [n_r, d] (CUDA fp32) in the features they come from
    -- comparable only between evaluations under one encoder, never with Inception-based FID.  ``normalize``: L2-normalise
    the rows here (False: the caller did, as ``extract_features`` does).  ``real_state``: ``real_state_of`` of the real set's
    bank (``real_feats`` is then not read and may be None).  ``n_iter``: the fixed number of Newton-Schulz steps.
    ValueError / RuntimeError before any GPU work on fewer than 2 rows of a set, unequal widths, ``n_iter`` < 1, host
    tensors, sizes the conv engine does not take.  Returns fd, mean_term, trace_real, trace_fake, cross_term
    (= tr (Sigma_r Sigma_f)^(1/2); fd subtracts it twice), n_iter, ``estimates`` (of ||Fc Rc^T||_* after each step, not
    yet divided), ``tail`` = estimates[-1] - estimates[-6] (0 if shorter), n_real, n_fake, dim and ``note``."""
    n_f = _feats(fake_feats, 'fake')
    d = fake_feats.shape[1]
    if real_state is None:
        n_r = _feats(real_feats, 'real')
        if real_feats.shape[1] != d:
            raise RuntimeError('fd: real features of width %d, fake ones of width %d' % (real_feats.shape[1], d))
    else:
        n_r = int(real_state.n)
        if real_state.bankT.shape[0] != d or real_state.bankT.shape[1] != ops.round_up(n_r, 4):
            raise RuntimeError('fd: a real bank of %s for %d rows and fake features of width %d'
                               % (tuple(real_state.bankT.shape), n_r, d))
    p, q = check_sizes(n_r, n_f, n_iter, d)                                    # (before any GPU work)
    n_iter = int(n_iter)
    _on_device(fake_feats, 'fake')
    if real_state is None:
        _on_device(real_feats, 'real')
    dev = fake_feats.device
    table = torch.zeros(n_iter + 4, device=dev, dtype=torch.float64)          # estimates, sumsq_r, sumsq_f, mean term, ||M||_F^2
    cell = lambda i: table[n_iter + i:n_iter + i + 1]

    Fc, mu_f = centred_rows(features.normalize_rows(fake_feats) if normalize else fake_feats.contiguous())
    ops.dot_sums(Fc, Fc, d, out=cell(1))
    Rc = None
    if real_state is None:
        Rc, mu_r = centred_rows(features.normalize_rows(real_feats) if normalize else real_feats.contiguous())
        ops.dot_sums(Rc, Rc, d, out=cell(0))
    else:
        mu_r = real_state.mu
        cell(0).copy_(real_state.sumsq)
    cell(2).copy_(((mu_r - mu_f) ** 2).sum().reshape(1))

    # M [p][q_pad]: the rows of the larger set against the bank of the smaller one (||M||_* = ||M^T||_*)
    if n_f >= n_r:
        rows, bank = Fc, (real_state.bankT if real_state is not None else features.bank_of(Rc))
    else:
        rows, bank = (Rc if Rc is not None else real_state.bankT[:, :n_r].t().contiguous()), features.bank_of(Fc)
    q_pad = bank.shape[1]
    M = gemm_rows(rows, bank, torch.empty(p, q_pad, device=dev))
    del rows, bank, Fc, Rc
    ops.dot_sums(M, M, q, out=cell(3))
    fro2 = cell(3)
    scale = torch.where(fro2 > 0, fro2.rsqrt(), torch.zeros_like(fro2)).float()      # a device scalar: no host read
    X = M * scale
    XT, Xn = torch.empty(q, p, device=dev), torch.empty_like(X)
    G, H = torch.empty(q, q_pad, device=dev), torch.zeros(q_pad, q_pad, device=dev)
    for k in range(n_iter):
        newton_schulz_step(X, XT, G, H, Xn, q)
        X, Xn = Xn, X
        ops.dot_sums(X, M, q, out=table[k:k + 1])
    host = table.cpu().numpy()                                                 # the one device-to-host read
    return combine(host[:n_iter], host[n_iter], host[n_iter + 1], host[n_iter + 2], n_r, n_f, d)


def combine(estimates, sumsq_real, sumsq_fake, mean_term, n_real, n_fake, dim):
    """The result dict from what the device table holds, in float64 on the host."""
    est = np.asarray(estimates, np.float64)
    trace_r, trace_f = float(sumsq_real) / (n_real - 1), float(sumsq_fake) / (n_fake - 1)
    cross = float(est[-1]) / math.sqrt(float(n_real - 1) * float(n_fake - 1))
    return {'fd': float(mean_term) + trace_r + trace_f - 2.0 * cross, 'mean_term': float(mean_term), 'trace_real': trace_r,
            'trace_fake': trace_f, 'cross_term': cross, 'n_iter': len(est), 'estimates': est.tolist(),
            'tail': float(est[-1] - est[-6]) if len(est) >= 6 else 0.0, 'n_real': int(n_real), 'n_fake': int(n_fake),
            'dim': int(dim), 'note': NOTE}


def fd_of(encoder, real_u8, fake_u8, n_iter=N_ITER, batch=500):
    """``fd`` of device-resident uint8 [n, H, W, 3] sets through ``encoder`` (on the GPU, in eval mode), ``batch`` images per
    trunk forward.  Comparable only between evaluations under one encoder file, never with Inception-based FID."""
    features.check_u8(fake_u8, 'fake', 'fd')
    features.check_u8(real_u8, 'real', 'fd')
    if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
        raise ValueError('fd: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    check_sizes(real_u8.shape[0], fake_u8.shape[0], n_iter)
    return fd(features.extract_features(encoder, real_u8, batch), features.extract_features(encoder, fake_u8, batch), n_iter,
              normalize=False)


def csv_line(step, out):
    return '%d,%.6f,%.6f,%.6f,%.6f,%.3e' % (step, out['fd'], out['fd_mean_term'], out['fd_trace_fake'], out['fd_cross_term'],
                                            out['fd_tail'])


def line_of(out):
    """The printed line; it warns when the last five steps still moved the estimate by more than TAIL_WARN of it."""
    warn = ''
    if abs(out['tail']) > TAIL_WARN * abs(out['estimates'][-1]):
        warn = '  WARNING: the estimate moved by %.3e over the last 5 of %d steps (more than %.0e of it): raise --n_iter' % (
            out['tail'], out['n_iter'], TAIL_WARN)
    return ('FD (features of this encoder: not an Inception FID): [fd %.6f] = [means %.6f] + [tr real %.6f] + [tr fake %.6f] - 2 '
            '[cross %.6f] after %d steps on %d fake / %d real images%s' % (
                out['fd'], out['mean_term'], out['trace_real'], out['trace_fake'], out['cross_term'], out['n_iter'],
                out['n_fake'], out['n_real'], warn))


def parse_args(argv=None):
    return features.real_fake_parser(
        'Testing script: Frechet distance of the means and covariances of the L2-normalised features of a frozen '
        'discriminator (one process, one GPU), the trace term by a fixed number of Newton-Schulz steps on the conv engine.  '
        'Comparable only between evaluations under one encoder file, never with Inception-based FID',
        'file-name tag and seed of the latents of --gen (default: drawn)',
        after_sizes=(('--n_iter', dict(default=N_ITER, type=int,
                                       help='Newton-Schulz steps, fixed: no adaptive stop (default: %d)' % N_ITER)),)
    ).parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    if P.n_iter < 1:                                                           # (before the sets are read, and any GPU work)
        raise ValueError('--n_iter must be at least 1, got %r' % (P.n_iter,))
    return features.real_fake_main(
        P, 'the Frechet distance runs', lambda n_real, n_fake: check_sizes(n_real, n_fake, P.n_iter),
        lambda E, real, fake, seed: fd_of(E, real, fake, P.n_iter, P.batch_size), line_of, 'fd_%d.json')


if __name__ == '__main__':
    main()
