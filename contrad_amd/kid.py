"""One distance between generated images and data without an Inception network: the kernel distance (KID) of Binkowski
et al. 2018 -- the unbiased MMD^2 under a cubic polynomial kernel, averaged over subsets -- in the feature space of a
FROZEN discriminator, the space of contrad_amd/prdc.py.  An ADDITION of this project: the reference tracks FID, which is
out of scope here (DESIGN.md sections 8, 16 and 17).  The numbers are comparable only between evaluations made with the
same encoder file, NEVER with the Inception-based KID of papers.

    python test_kid.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_kid.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7

Features are ``D.penultimate`` in eval mode with L2-normalised rows (``features.extract_features``), and

    k(a, b) = (gamma a.b + coef0)^3,  gamma = 1, coef0 = 1

(the paper's gamma = 1 / d is meant for unnormalised Inception features; on the unit sphere a.b lies in [-1, 1] and 1 / d
would flatten the cubic to 1 + 3 a.b / d).  With m = min(subset_size, n_r, n_f) and, per subset t, the rows R_t, F_t that
``subset_indices`` draws (S_XY = X Y^T):

    A_t = sum_{i != j} k(S_RR)    B_t = sum_{i != j} k(S_FF)    C_t = sum_{i, j} k(S_FR)       (self pairs left out by index)
    MMD2_t = (A_t + B_t) / (m (m - 1)) - 2 C_t / m^2        kid = mean_t MMD2_t        kid_std = std_t MMD2_t (ddof 0)

  * banks and the row chunks of S: contrad_amd/features.py;
  * csrc/kid.hip: ``kid_sums`` per chunk, every term and every sum in float64, ``self0`` = the chunk's first row, the
    second and later chunks accumulate;
  * the host reads the [n_subsets][3] table of sums once and divides, averages and takes the deviation in float64.  KID
    may be slightly negative (the estimator is unbiased); it is not clamped.

``--prdc_kid`` of the training scripts adds this to every evaluation of the ``--prdc_data`` hook (``prdc.PRDCMonitor``: the
same frozen encoder, the same fakes, the same real set), appended to ``kid_<eval_seed>.csv``; ``--prdc_best kid`` keeps the
``*_best.pt`` files of the evaluation with the SMALLEST value.
"""
import math

import numpy as np
import torch

from . import features, ops

DEGREE = 3
CSV_HEAD = 'step,kid,kid_std'
KERNEL_NOTE = ('k(a, b) = (gamma a.b + coef0)^3 on L2-normalised penultimate features of a frozen discriminator; gamma = 1 '
               'departs from the 1 / d of Binkowski et al. 2018 (unnormalised Inception features): on the unit sphere 1 / d '
               'would flatten the cubic.  Comparable only between evaluations under one encoder file, never with '
               'Inception-based KID.')


def check_sizes(n_real, n_fake, n_subsets=100, subset_size=1000):
    """The host refusals -> m = min(subset_size, n_real, n_fake), the rows of a subset."""
    if int(n_subsets) < 1:
        raise ValueError('kid: n_subsets must be at least 1, got %r' % (n_subsets,))
    if int(subset_size) < 2:
        raise ValueError('kid: subset_size must be at least 2, got %r' % (subset_size,))
    if n_real < 1 or n_fake < 1:
        raise ValueError('kid: empty %s set' % ('real' if n_real < 1 else 'fake'))
    m = min(int(subset_size), int(n_real), int(n_fake))
    if m < 2:
        raise ValueError('kid: a subset needs two rows of each set (%d real, %d fake): the unbiased estimate divides by m (m - 1)'
                         % (n_real, n_fake))
    return m


def check_kernel(gamma, coef0):
    if not (math.isfinite(float(gamma)) and math.isfinite(float(coef0))):
        raise ValueError('kid: gamma and coef0 must be finite, got %r, %r' % (gamma, coef0))


def subset_indices(n_r, n_f, m, n_subsets, seed):
    """(idx_r, idx_f), int64 [n_subsets][m]: per subset, in order, m distinct rows of the real set, then m distinct rows
    of the fake set, from ``np.random.default_rng(seed)``.  Host only."""
    rng = np.random.default_rng(seed)
    idx_r, idx_f = np.empty((n_subsets, m), np.int64), np.empty((n_subsets, m), np.int64)
    for t in range(n_subsets):
        idx_r[t] = rng.choice(n_r, m, replace=False)
        idx_f[t] = rng.choice(n_f, m, replace=False)
    return idx_r, idx_f


def mmd2_of(sums, m):
    """MMD2_t of the [n_subsets][3] table of (A_t, B_t, C_t), in float64."""
    s = np.asarray(sums, np.float64).reshape(-1, 3)
    return (s[:, 0] + s[:, 1]) / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)


def _feats(feats, what):
    if not torch.is_tensor(feats) or feats.dtype != torch.float32 or feats.dim() != 2:
        raise RuntimeError('kid: the %s features must be a CUDA float32 (n, d) matrix' % what)
    return feats.shape[0]


def _on_device(feats, what):
    if not feats.is_cuda:
        raise RuntimeError('kid: the %s features must be a CUDA float32 (n, d) matrix' % what)


def gather_subset(real, real_bankT, fake, idx_r, idx_f):
    """(R_t, F_t, bank of R_t, bank of F_t) for the device index vectors of one subset.  The real set is given as rows
    ``real`` [n_r, d] or, with ``real`` None, as its transposed bank ``real_bankT`` [d][>= n_r]: the same floats either way."""
    m, d = idx_f.numel(), fake.shape[1]
    F_t = fake.index_select(0, idx_f)
    if real is not None:
        R_t = real.index_select(0, idx_r)
        bank_R = features.bank_of(R_t)
    else:
        bank_R = features.new_bank(m, d, fake.device)
        bank_R[:, :m].copy_(real_bankT.index_select(1, idx_r))
        R_t = bank_R[:, :m].t().contiguous()
    return R_t, F_t, bank_R, features.bank_of(F_t)


def block_sum(q, bankT, n, leave_self_out, gamma, coef0, out, S=None):
    """out[0] = sum of k over the similarities of ``q`` to the first ``n`` columns of the bank, pair (i, i) left out with
    ``leave_self_out``."""
    for i, chunk in features.similarity_chunks(q, bankT, S):
        ops.kid_sums(chunk, n, self0=i if leave_self_out else -1, gamma=gamma, coef0=coef0, out=out, accumulate=i > 0)
    return out


def kid(real_feats, fake_feats, n_subsets=100, subset_size=1000, seed=0, normalize=True, gamma=1.0, coef0=1.0,
        real_bank=None):
    """The kernel distance of fake feature rows [n_f, d] from real ones [n_r, d] (CUDA fp32) in the features they come
    from -- comparable only between evaluations under one encoder, never with Inception-based KID.  ``normalize``:
    L2-normalise the rows here (False: the caller did, as ``extract_features`` does).  ``real_bank``: ``(bankT, n_real)``, the
    transposed bank ``features.bank_of`` of the normalised real rows (``real_feats`` is then not read and may be None).
    Returns kid, kid_std, n_subsets, subset_size (the m actually used), n_real, n_fake, gamma, coef0, degree, seed, the
    table ``sums`` of (A_t, B_t, C_t) behind them and ``kernel``, the note on the kernel."""
    n_f = _feats(fake_feats, 'fake')
    if real_bank is None:
        n_r = _feats(real_feats, 'real')
        if real_feats.shape[1] != fake_feats.shape[1]:
            raise RuntimeError('kid: real features of width %d, fake ones of width %d' % (real_feats.shape[1], fake_feats.shape[1]))
    else:
        real_bankT, n_r = real_bank
        if real_bankT.shape[0] != fake_feats.shape[1] or real_bankT.shape[1] < n_r:
            raise RuntimeError('kid: a real bank of %s for %d rows and fake features of width %d'
                               % (tuple(real_bankT.shape), n_r, fake_feats.shape[1]))
    m = check_sizes(n_r, n_f, n_subsets, subset_size)                          # (before any GPU work)
    check_kernel(gamma, coef0)
    n_subsets, gamma, coef0 = int(n_subsets), float(gamma), float(coef0)
    _on_device(fake_feats, 'fake')
    fake = features.normalize_rows(fake_feats) if normalize else fake_feats.contiguous()
    real = real_bankT = None
    if real_bank is None:
        _on_device(real_feats, 'real')
        real = features.normalize_rows(real_feats) if normalize else real_feats.contiguous()
    else:
        real_bankT = real_bank[0]
    dev = fake.device
    idx = torch.from_numpy(np.stack(subset_indices(n_r, n_f, m, n_subsets, seed))).to(dev)      # [2][n_subsets][m]
    table = torch.empty(n_subsets, 3, device=dev, dtype=torch.float64)
    m_pad = ops.round_up(m, 4)
    S = torch.empty(min(features.chunk_rows_of(m_pad), m), m_pad, device=dev)
    for t in range(n_subsets):
        R_t, F_t, bank_R, bank_F = gather_subset(real, real_bankT, fake, idx[0, t], idx[1, t])
        block_sum(R_t, bank_R, m, True, gamma, coef0, table[t, 0:1], S)
        block_sum(F_t, bank_F, m, True, gamma, coef0, table[t, 1:2], S)
        block_sum(F_t, bank_R, m, False, gamma, coef0, table[t, 2:3], S)
    sums = table.cpu().numpy()                                                 # the one device-to-host read
    mmd2 = mmd2_of(sums, m)
    return {'kid': float(mmd2.mean()), 'kid_std': float(mmd2.std()), 'n_subsets': n_subsets, 'subset_size': m,
            'n_real': int(n_r), 'n_fake': int(n_f), 'gamma': gamma, 'coef0': coef0, 'degree': DEGREE, 'seed': int(seed),
            'sums': sums.tolist(), 'kernel': KERNEL_NOTE}


def kid_of(encoder, real_u8, fake_u8, n_subsets=100, subset_size=1000, seed=0, batch=500, gamma=1.0, coef0=1.0):
    """``kid`` of device-resident uint8 [n, H, W, 3] sets through ``encoder`` (on the GPU, in eval mode), ``batch`` images per
    trunk forward.  Comparable only between evaluations under one encoder file, never with Inception-based KID."""
    features.check_u8(fake_u8, 'fake', 'kid')
    features.check_u8(real_u8, 'real', 'kid')
    if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
        raise ValueError('kid: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    check_sizes(real_u8.shape[0], fake_u8.shape[0], n_subsets, subset_size)
    check_kernel(gamma, coef0)
    return kid(features.extract_features(encoder, real_u8, batch), features.extract_features(encoder, fake_u8, batch), n_subsets, subset_size,
               seed, normalize=False, gamma=gamma, coef0=coef0)


def csv_line(step, out):
    return '%d,%.6f,%.6f' % (step, out['kid'], out['kid_std'])


def best_in_csv(path, upto_step):
    """The smallest kid among the rows of a ``kid_<seed>.csv`` with step <= ``upto_step`` (None: no such row)."""
    return features.best_in_csv(path, 1, upto_step, min)


def parse_args(argv=None):
    return features.real_fake_parser(
        'Testing script: kernel distance (KID, cubic kernel, gamma = coef0 = 1) in the L2-normalised features of a frozen '
        'discriminator (one process, one GPU).  Comparable only between evaluations under one encoder file, never with '
        'Inception-based KID',
        'file-name tag, seed of the subsets and of the latents of --gen (default: drawn)',
        after_sizes=(('--n_subsets', dict(default=100, type=int, help='subsets the estimate is averaged over (default: 100)')),
                     ('--subset_size', dict(default=1000, type=int,
                                            help='rows of each set per subset (default: 1000; at most the smaller set)')))
    ).parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    return features.real_fake_main(
        P, 'the kernel distance runs', lambda n_real, n_fake: check_sizes(n_real, n_fake, P.n_subsets, P.subset_size),
        lambda E, real, fake, seed: kid_of(E, real, fake, P.n_subsets, P.subset_size, seed, P.batch_size),
        lambda out: 'KID (cubic kernel, gamma 1, coef0 1, features of this encoder: not an Inception KID): [kid %.6f +- %.6f] '
                    'over %d subsets of %d on %d fake / %d real images' % (
                        out['kid'], out['kid_std'], out['n_subsets'], out['subset_size'], out['n_fake'], out['n_real']),
        'kid_%d.json')


if __name__ == '__main__':
    main()
