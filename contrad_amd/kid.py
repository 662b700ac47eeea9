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

A second kernel, ``kernel='rq'`` (``--kernel rq``), is CHARACTERISTIC where the cubic sees moments up to order 3 only (two
different feature distributions can be at cubic distance 0): the rational-quadratic mixture of Binkowski et al. on the squared
distance u = ||a - b||^2 = 2 - 2 a.b of two UNIT rows (clamped below at 0),

    k(a, b) = sum over alpha in {1/2, 1, 2} of (1 + u / (2 alpha))^-alpha = 1 / sqrt(1 + u) + 1 / (1 + u / 2) + 1 / (1 + u / 4)^2

The alphas are not the paper's {0.2, 0.5, 1, 2, 5}: with these three every term is a fixed number of correctly rounded
float64 operations (square root and division, no pow), so the parity bound is derived, not measured.
The same subsets, gathers, chunks, table and ``mmd2_of``; only the launch differs (``ops.mmd_sums``).  ``intra_class_kid``
(``--intra``) is the mean over classes of the distance between the real and the fake rows of each class, for the labelled
``samples.npz`` of test_gan_sample_cddls.py against the ``y_train`` of tools/make_image_npz.py.

``--prdc_kid`` of the training scripts adds this to every evaluation of the ``--prdc_data`` hook (``prdc.PRDCMonitor``: the
same frozen encoder, the same fakes, the same real set), appended to ``kid_<eval_seed>.csv``; ``--prdc_best kid`` keeps the
``*_best.pt`` files of the evaluation with the SMALLEST value.  ``--prdc_kid_kernel rq`` computes the rational-quadratic
distance instead, appended to ``kid_rq_<eval_seed>.csv`` (never into ``kid_<eval_seed>.csv``), which ``--prdc_best kid`` then tracks.
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
KERNELS = ('poly3', 'rq')
RQ_NOTE = ('k(a, b) = sum over alpha in {1/2, 1, 2} of (1 + u / (2 alpha))^-alpha at u = max(2 - 2 a.b, 0), the squared distance '
           'of L2-normalised penultimate features of a frozen discriminator: the rational-quadratic mixture of Binkowski et al. '
           '2018 with alphas that need square root and division only (theirs: 0.2, 0.5, 1, 2, 5), so every term is a fixed '
           'number of correctly rounded float64 operations.  Comparable only between evaluations under one encoder file, '
           'never with Inception-based KID, whatever the alphas.')
KERNEL_NOTES = {'poly3': KERNEL_NOTE, 'rq': RQ_NOTE}


def check_kernel_name(kernel):
    if kernel not in KERNELS:
        raise ValueError('kid: unknown kernel %r (one of %s)' % (kernel, ', '.join(KERNELS)))


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


def block_sum(q, bankT, n, leave_self_out, gamma, coef0, out, S=None, kernel='poly3'):
    """out[0] = sum of k over the similarities of ``q`` to the first ``n`` columns of the bank, pair (i, i) left out with
    ``leave_self_out``."""
    for i, chunk in features.similarity_chunks(q, bankT, S):
        if kernel == 'poly3':
            ops.kid_sums(chunk, n, self0=i if leave_self_out else -1, gamma=gamma, coef0=coef0, out=out, accumulate=i > 0)
        else:
            ops.mmd_sums(chunk, n, kernel, self0=i if leave_self_out else -1, out=out, accumulate=i > 0)
    return out


def kid(real_feats, fake_feats, n_subsets=100, subset_size=1000, seed=0, normalize=True, gamma=1.0, coef0=1.0,
        real_bank=None, kernel='poly3'):
    """The kernel distance of fake feature rows [n_f, d] from real ones [n_r, d] (CUDA fp32) in the features they come
    from -- comparable only between evaluations under one encoder, never with Inception-based KID.  ``normalize``:
    L2-normalise the rows here (False: the caller did, as ``extract_features`` does).  ``real_bank``: ``(bankT, n_real)``, the
    transposed bank ``features.bank_of`` of the normalised real rows (``real_feats`` is then not read and may be None).
    ``kernel``: one of ``KERNELS``.  'rq' takes the rows as UNIT vectors (u = 2 - 2 a.b is their squared distance only then):
    ``normalize=True``, or the caller's contract with ``normalize=False`` (the hook, ``kid_of``); gamma and coef0 are not read.
    Returns kid, kid_std, n_subsets, subset_size (the m actually used), n_real, n_fake, gamma, coef0, degree, seed, the
    table ``sums`` of (A_t, B_t, C_t) behind them, ``kernel_name`` and ``kernel``, the note on that kernel ('rq' carries no
    gamma, coef0 or degree)."""
    check_kernel_name(kernel)                                                  # (before any GPU work)
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
        block_sum(R_t, bank_R, m, True, gamma, coef0, table[t, 0:1], S, kernel)
        block_sum(F_t, bank_F, m, True, gamma, coef0, table[t, 1:2], S, kernel)
        block_sum(F_t, bank_R, m, False, gamma, coef0, table[t, 2:3], S, kernel)
    sums = table.cpu().numpy()                                                 # the one device-to-host read
    mmd2 = mmd2_of(sums, m)
    out = {'kid': float(mmd2.mean()), 'kid_std': float(mmd2.std()), 'n_subsets': n_subsets, 'subset_size': m,
           'n_real': int(n_r), 'n_fake': int(n_f), 'gamma': gamma, 'coef0': coef0, 'degree': DEGREE, 'seed': int(seed),
           'sums': sums.tolist(), 'kernel': KERNEL_NOTES[kernel], 'kernel_name': kernel}
    if kernel != 'poly3':
        for name in ('gamma', 'coef0', 'degree'):
            del out[name]
    return out


def kid_of(encoder, real_u8, fake_u8, n_subsets=100, subset_size=1000, seed=0, batch=500, gamma=1.0, coef0=1.0, kernel='poly3'):
    """``kid`` of device-resident uint8 [n, H, W, 3] sets through ``encoder`` (on the GPU, in eval mode), ``batch`` images per
    trunk forward.  Comparable only between evaluations under one encoder file, never with Inception-based KID."""
    check_kernel_name(kernel)
    features.check_u8(fake_u8, 'fake', 'kid')
    features.check_u8(real_u8, 'real', 'kid')
    if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
        raise ValueError('kid: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    check_sizes(real_u8.shape[0], fake_u8.shape[0], n_subsets, subset_size)
    check_kernel(gamma, coef0)
    return kid(features.extract_features(encoder, real_u8, batch), features.extract_features(encoder, fake_u8, batch), n_subsets, subset_size,
               seed, normalize=False, gamma=gamma, coef0=coef0, kernel=kernel)


# ---- intra-class ----
def class_rows(real_labels, fake_labels, n_real, n_fake, n_classes):
    """The host refusals of the intra-class distance -> per class c in order, (rows of the real set, rows of the fake set)
    as int64 arrays.  ValueError on label arrays that are not one integer per row, a label outside [0, n_classes), or a
    class with fewer than two rows on either side."""
    n_classes = int(n_classes)
    if n_classes < 1:
        raise ValueError('kid: n_classes must be at least 1, got %r' % (n_classes,))
    rows = []
    for labels, n, what in ((real_labels, n_real, 'real'), (fake_labels, n_fake, 'fake')):
        y = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
        if y.ndim != 1 or y.dtype.kind not in 'iu' or len(y) != n:
            raise ValueError('kid: the %s labels must be one integer per row (%d rows), got %s %s' % (what, n, y.dtype, y.shape))
        y = y.astype(np.int64)
        if len(y) and (y.min() < 0 or y.max() >= n_classes):
            raise ValueError('kid: a %s label outside [0, %d): %d' % (what, n_classes, y.min() if y.min() < 0 else y.max()))
        rows.append([np.flatnonzero(y == c) for c in range(n_classes)])
    for c in range(n_classes):
        if len(rows[0][c]) < 2 or len(rows[1][c]) < 2:
            raise ValueError('kid: class %d has %d real and %d fake rows: the unbiased estimate needs two of each'
                             % (c, len(rows[0][c]), len(rows[1][c])))
    return list(zip(rows[0], rows[1]))


def intra_of(per_class):
    """(kid_intra, kid_intra_std): the plain mean of the class values and their population deviation, in float64."""
    v = np.asarray([c['kid'] for c in per_class], np.float64)
    return float(v.mean()), float(v.std())


def intra_class_kid(real_feats, real_labels, fake_feats, fake_labels, n_classes, n_subsets=100, subset_size=1000, seed=0,
                    kernel='poly3', normalize=True):
    """The intra-class kernel distance of labelled feature rows: for each class c in order, ``kid`` of the fake rows of
    class c from the real rows of class c, with the same ``seed`` for every class and m_c = min(subset_size, n_r_c, n_f_c);
    ``kid_intra`` is the plain mean of the class values, ``kid_intra_std`` their population deviation over classes (not an
    error bar of the mean).  Labels: one integer per row, host arrays or tensors.  ValueError before any GPU work on a
    label outside [0, n_classes), a class with fewer than 2 rows on either side, label arrays of another length than the
    features, an unknown kernel.  Returns kid_intra, kid_intra_std, n_classes, ``classes`` (the dict of ``kid`` per
    class), seed, ``kernel_name`` and ``kernel``, the note."""
    check_kernel_name(kernel)
    n_f, n_r = _feats(fake_feats, 'fake'), _feats(real_feats, 'real')
    rows = class_rows(real_labels, fake_labels, n_r, n_f, n_classes)
    for r, f in rows:
        check_sizes(len(r), len(f), n_subsets, subset_size)
    _on_device(fake_feats, 'fake')
    _on_device(real_feats, 'real')
    dev = fake_feats.device
    per_class = [kid(real_feats.index_select(0, torch.from_numpy(r).to(dev)), fake_feats.index_select(0, torch.from_numpy(f).to(dev)),
                     n_subsets, subset_size, seed, normalize=normalize, kernel=kernel) for r, f in rows]
    mean, std = intra_of(per_class)
    return {'kid_intra': mean, 'kid_intra_std': std, 'n_classes': len(rows), 'classes': per_class, 'seed': int(seed),
            'kernel': KERNEL_NOTES[kernel], 'kernel_name': kernel}


def intra_class_kid_of(encoder, real_u8, real_labels, fake_u8, fake_labels, n_classes, n_subsets=100, subset_size=1000, seed=0,
                       batch=500, kernel='poly3'):
    """``intra_class_kid`` of device-resident uint8 [n, H, W, 3] sets through ``encoder``: every image is encoded once."""
    check_kernel_name(kernel)
    features.check_u8(fake_u8, 'fake', 'kid')
    features.check_u8(real_u8, 'real', 'kid')
    if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
        raise ValueError('kid: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    class_rows(real_labels, fake_labels, real_u8.shape[0], fake_u8.shape[0], n_classes)
    return intra_class_kid(features.extract_features(encoder, real_u8, batch), real_labels, features.extract_features(encoder, fake_u8, batch),
                           fake_labels, n_classes, n_subsets, subset_size, seed, kernel, normalize=False)


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
                                            help='rows of each set per subset (default: 1000; at most the smaller set)')),
                     ('--kernel', dict(default='poly3', choices=KERNELS,
                                       help='poly3: the cubic kernel (default, kid_<seed>.json); rq: the rational-quadratic mixture '
                                            'over alpha = 1/2, 1, 2 on the squared distance of the unit rows, a characteristic '
                                            'kernel (kid_rq_<seed>.json)')),
                     ('--intra', dict(action='store_true',
                                      help='the intra-class distance: the mean over classes of the distance between the real and the '
                                           'fake images of each class (kid_intra_<seed>.json / kid_intra_rq_<seed>.json).  Needs '
                                           '--fake with the labels of test_gan_sample_cddls.py and --real with y_train; not with --gen')),
                     ('--n_classes', dict(default=None, type=int,
                                          help='with --intra: the number of classes (default: the largest label of y_train + 1)')))
    ).parse_args(argv)


def json_name(kernel, intra=False):
    """``kid_<seed>.json`` for the default kernel as ever; ``kid_rq_``, ``kid_intra_``, ``kid_intra_rq_`` for the others."""
    return 'kid_%s%s%%d.json' % ('intra_' if intra else '', '' if kernel == 'poly3' else kernel + '_')


def load_labels(path, key, n=None):
    """int64 [n] labels ``key`` of an npz, the first ``n`` of them (``features.load_images`` takes the same rows)."""
    with np.load(path) as z:
        if key not in z:
            raise ValueError('%s holds no %s: --intra needs the labels of both sets' % (path, key))
        y = np.asarray(z[key])
    if y.ndim != 1 or y.dtype.kind not in 'iu':
        raise ValueError('%s: %s must be one integer per image, got %s %s' % (path, key, y.dtype, y.shape))
    return y[:n].astype(np.int64)


def main(argv=None):
    P = parse_args(argv)
    check_kernel_name(P.kernel)
    what = 'cubic kernel, gamma 1, coef0 1' if P.kernel == 'poly3' else 'rational-quadratic kernel, alpha 1/2, 1, 2'
    if not P.intra:
        if P.n_classes is not None:
            raise ValueError('--n_classes does nothing without --intra')
        return features.real_fake_main(
            P, 'the kernel distance runs', lambda n_real, n_fake: check_sizes(n_real, n_fake, P.n_subsets, P.subset_size),
            lambda E, real, fake, seed: kid_of(E, real, fake, P.n_subsets, P.subset_size, seed, P.batch_size, kernel=P.kernel),
            lambda out: 'KID (%s, features of this encoder: not an Inception KID): [kid %.6f +- %.6f] '
                        'over %d subsets of %d on %d fake / %d real images' % (
                            what, out['kid'], out['kid_std'], out['n_subsets'], out['subset_size'], out['n_fake'], out['n_real']),
            json_name(P.kernel))
    if P.gen or not P.fake:                                                    # (before the sets are read, and any GPU work)
        raise ValueError('--intra needs --fake FILE.npz with the labels test_gan_sample_cddls.py writes: images sampled here '
                         'from --gen have no classes')
    y_real, y_fake = load_labels(P.real, 'y_train', P.n_real), load_labels(P.fake, 'labels', P.n_fake)
    n_classes = int(y_real.max()) + 1 if P.n_classes is None and len(y_real) else P.n_classes

    def sizes(n_real, n_fake):
        for r, f in class_rows(y_real, y_fake, n_real, n_fake, n_classes):
            check_sizes(len(r), len(f), P.n_subsets, P.subset_size)
    return features.real_fake_main(
        P, 'the kernel distance runs', sizes,
        lambda E, real, fake, seed: intra_class_kid_of(E, real, y_real, fake, y_fake, n_classes, P.n_subsets, P.subset_size, seed,
                                                       P.batch_size, P.kernel),
        lambda out: 'intra-class KID (%s, features of this encoder: not an Inception KID): [kid_intra %.6f, deviation over '
                    'classes %.6f] over %d classes: %s' % (what, out['kid_intra'], out['kid_intra_std'], out['n_classes'],
                                                          ' '.join('%.6f' % c['kid'] for c in out['classes'])),
        json_name(P.kernel, intra=True))


if __name__ == '__main__':
    main()
