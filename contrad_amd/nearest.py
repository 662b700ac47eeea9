"""The memorisation check next to the sample-quality numbers of contrad_amd/prdc.py and contrad_amd/kid.py: a generator that
replays its training set gets the best value of every one of them.  In the feature space of the same FROZEN discriminator
this module finds the nearest training images of generated samples, shows them as a figure and counts how many samples
are suspiciously close to one training image -- the authenticity score of Alaa et al. 2022 ("How Faithful is your
Synthetic Data?").  An ADDITION of this project: the reference has nothing of the kind.

    python test_nearest.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz --holdout
    python test_nearest.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7 --k 8 --rows 16

Features are ``D.penultimate`` in eval mode with L2-normalised rows (``features.extract_features``); every comparison is
made on the fp32 similarities the conv engine writes (prdc.py's rule).  With R the n_r real rows, F the n_f fake rows:

    t1[i]  = the largest S_RR[i][l], l != i,  nn1[i] that l          (self left out by index: a duplicate of i elsewhere counts)
    i*(j)  = the first column of fake j's neighbour order in S_FR,   s_j = S_FR[j][i*(j)]
    authentic_j = s_j < t1[i*(j)]                                    (strict; a NaN compares false)
    authenticity = #authentic / n_f

A fake is NOT authentic when it lies at least as close to its nearest training image as that image lies to its own nearest
other training image.  The number has no absolute scale: fresh real images (``--holdout``: ``x_test`` in place of the fakes)
score well below 1, and a perfect generator scores about what they score.  It is comparable only between evaluations
under one encoder file.  Alaa et al. compare Euclidean distances; on unit rows ||a - b||^2 = 2 - 2 a.b, so both orders agree.

  * banks and the row chunks of S: contrad_amd/features.py;
  * csrc/knn.hip: ``knn_select`` per chunk, with ``self0`` = the chunk's first row for the real-against-real pass (the
    leave-self-out argument of the select kernel); callers here have no labels and pass a cached zero vector with one class;
  * ``authenticity`` reads the device once.

``--prdc_auth`` of the training scripts appends ``step,authenticity,nearest_mean`` to ``auth_<eval_seed>.csv`` at every
evaluation of the ``--prdc_data`` hook (``prdc.PRDCMonitor``: the same encoder, fakes and real bank).  It records only: it
is no ``--prdc_best`` choice, because it is not a quantity to maximise.
"""
import os
from pathlib import Path

import numpy as np
import torch

from . import features, hostio, ops

CSV_HEAD = 'step,authenticity,nearest_mean'
NOTE = ('authenticity = the share of fakes with s_j < t1[i*(j)]: s_j the similarity of fake j to its nearest real i*(j), t1[i] the '
        'similarity of real i to its nearest OTHER real (self left out by index), on L2-normalised penultimate features of a '
        'frozen discriminator.  Comparable only between evaluations under one encoder file.  It has no absolute scale: read it '
        'against holdout_authenticity (--holdout: held-out real images in place of the fakes), not against 1.  Not the Euclidean '
        'version of Alaa et al. 2022; on unit rows the two orders agree.')

_ZERO_LABELS = {}


def _zero_labels(n, device):
    """The label vector of a caller without labels: int64 zeros [n], one cached vector per device (the last bank size)."""
    key = (device.type, device.index)
    if key not in _ZERO_LABELS or _ZERO_LABELS[key].numel() != n:
        _ZERO_LABELS[key] = torch.zeros(n, device=device, dtype=torch.int64)
    return _ZERO_LABELS[key]


def _rows(feats, what, normalize):
    if not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2:
        raise RuntimeError('nearest: the %s features must be a CUDA float32 (n, d) matrix' % what)
    if feats.shape[0] < 1:
        raise ValueError('nearest: empty %s set' % what)
    return features.normalize_rows(feats) if normalize else feats.contiguous()


def check_k(k, n, leave_self_out=False):
    """The refusals of k against a bank of ``n`` columns (``leave_self_out``: a row has n - 1 neighbours)."""
    remain = n - 1 if leave_self_out else n
    if int(k) < 1:
        raise ValueError('nearest: k must be at least 1, got %r' % (k,))
    if int(k) > remain:
        raise ValueError('nearest: k = %d above the %d columns that remain of a bank of %d%s'
                         % (k, remain, n, ' with the row itself left out' if leave_self_out else ''))
    if int(k) > ops.KNN_MAX_K:
        raise ValueError('nearest: k = %d above the kernel limit %d' % (k, ops.KNN_MAX_K))


def neighbours(rows, bankT, n, k, leave_self_out=False, S=None):
    """(idx int32 [M, k], val fp32 [M, k]): per row of ``rows`` [M, d] the first k of the ``n`` bank columns in the neighbour
    order (value descending, column ascending; contrad_knn_select's contract) and the very similarities.  ``bankT``: the
    transposed bank [d][round_up(n, 4)].  ``leave_self_out``: ``rows`` are the bank's own rows (M == n) and row i leaves
    column i out, by index.  ``S``: a buffer for the chunks of S (its rows are the chunk size).  Every refusal comes before
    any GPU work."""
    if not torch.is_tensor(rows) or not torch.is_tensor(bankT) or rows.dim() != 2 or bankT.dim() != 2:
        raise RuntimeError('nearest: rows [M, d] and a transposed bank [d][round_up(n, 4)] expected')
    n, k = int(n), int(k)
    M, d = rows.shape
    if n < 1 or tuple(bankT.shape) != (d, ops.round_up(n, 4)):
        raise RuntimeError('nearest: a bank of %s for %d columns and rows of width %d' % (tuple(bankT.shape), n, d))
    if leave_self_out and M != n:
        raise ValueError('nearest: leave_self_out takes the rows of the bank itself (%d rows, %d bank columns)' % (M, n))
    check_k(k, n, leave_self_out)
    for t, what in ((rows, 'rows'), (bankT, 'bank')):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError('nearest: the %s must be a CUDA float32 matrix' % what)
    dev = rows.device
    idx = torch.empty(M, k, device=dev, dtype=torch.int32)
    val = torch.empty(M, k, device=dev)
    labels = _zero_labels(n, dev)
    for i, Sc in features.similarity_chunks(rows.contiguous(), bankT, S):
        m = Sc.shape[0]
        ci, cv, _, _ = ops.knn_select(Sc, n, labels, 1, k, 1.0, self0=i if leave_self_out else -1)
        idx[i:i + m].copy_(ci)
        val[i:i + m].copy_(cv)
    return idx, val


def real_state_of(real_feats, normalize=True, bankT=None):
    """``(bankT, t1 fp32 [n_r], nn1 int32 [n_r])`` of a real set of at least two rows: its bank, the largest similarity of
    each real to ANOTHER real and that real's index -- what ``authenticity`` needs of it, for a caller whose real set does
    not change.  ``bankT``: the bank ``features.bank_of`` of the same (normalised) rows, where the caller keeps one."""
    rows = _rows(real_feats, 'real', normalize)
    n = rows.shape[0]
    if n < 2:
        raise ValueError('nearest: the real set needs at least 2 rows (%d): a row is compared with the others' % n)
    if bankT is None:
        bankT = features.bank_of(rows)
    idx, val = neighbours(rows, bankT, n, 1, leave_self_out=True)
    return bankT, val[:, 0].contiguous(), idx[:, 0].contiguous()


def verdicts(fake_rows, real_state):
    """(i* int32 [n_f], s fp32 [n_f], authentic bool [n_f]) of normalised fake rows against ``real_state_of``'s state, on
    the device."""
    bankT, t1, _ = real_state
    n_r = t1.numel()
    if bankT.shape[0] != fake_rows.shape[1] or bankT.shape[1] != ops.round_up(n_r, 4):
        raise RuntimeError('nearest: a real bank of %s for %d rows and fake features of width %d'
                           % (tuple(bankT.shape), n_r, fake_rows.shape[1]))
    idx, val = neighbours(fake_rows, bankT, n_r, 1)
    i_star, s = idx[:, 0].contiguous(), val[:, 0].contiguous()
    return i_star, s, s < t1.index_select(0, i_star.long())            # strict, on the two fp32 values; a NaN: False


def authenticity(real_feats, fake_feats, real_state=None, normalize=True):
    """The authenticity of fake feature rows [n_f, d] against real ones [n_r, d] (CUDA fp32): the share of fakes that are NOT
    closer to their nearest real than that real is to its own nearest other real (the module docstring has the formula).
    ``normalize``: L2-normalise the rows here (False: the caller did, as ``extract_features`` does; the rows must be UNIT
    rows).  ``real_state``: ``real_state_of`` of the same real set (``real_feats`` is then not read and may be None).
    Returns authenticity, n_authentic, nearest_mean (the float64 mean of s_j), real_nearest_mean (that of t1), n_real,
    n_fake and ``note``.  The number is comparable only under one encoder file; it is to be read against the value of
    held-out real images (``--holdout``), not against 1; it is not Alaa et al.'s Euclidean version, though on unit rows
    the two orders agree.  One device-to-host read."""
    fake = _rows(fake_feats, 'fake', normalize)
    if real_state is None:
        real_state = real_state_of(real_feats, normalize)
    _, s, authentic = verdicts(fake, real_state)
    t1 = real_state[1]
    n_r, n_f = t1.numel(), fake.shape[0]
    stats = torch.stack([authentic.sum().double(), s.double().sum(), t1.double().sum()])
    n_auth, s_sum, t_sum = stats.tolist()                                      # the one device-to-host read
    n_auth = int(n_auth)
    return {'authenticity': n_auth / n_f, 'n_authentic': n_auth, 'nearest_mean': s_sum / n_f, 'real_nearest_mean': t_sum / n_r,
            'n_real': n_r, 'n_fake': n_f, 'note': NOTE}


def real_state_of_images(encoder, real_u8, batch=500):
    features.check_u8(real_u8, 'real', 'nearest')
    return real_state_of(features.extract_features(encoder, real_u8, batch), normalize=False)


def authenticity_of(encoder, real_u8, fake_u8, batch=500, real_state=None):
    """``authenticity`` of device-resident uint8 [n, H, W, 3] sets through ``encoder`` (on the GPU, in eval mode), ``batch``
    images per trunk forward.  ``real_state``: ``real_state_of_images`` of the real set (``real_u8`` is then not read)."""
    features.check_u8(fake_u8, 'fake', 'nearest')
    if real_state is None:
        features.check_u8(real_u8, 'real', 'nearest')
        if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
            raise ValueError('nearest: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
        if real_u8.shape[0] < 2:
            raise ValueError('nearest: the real set needs at least 2 images (%d)' % real_u8.shape[0])
        real_state = real_state_of_images(encoder, real_u8, batch)
    return authenticity(None, features.extract_features(encoder, fake_u8, batch), real_state=real_state, normalize=False)


def most_similar(s, rows):
    """The ``rows`` indices of the host vector ``s`` with the largest values, in that order; a tie keeps the lower index, a
    NaN comes last."""
    s = np.asarray(s, np.float64)
    return np.argsort(-np.where(np.isnan(s), -np.inf, s), kind='stable')[:rows].astype(np.int64)


def check_retrieval(k, rows, n_real, n_fake):
    check_k(k, n_real)
    if not 1 <= int(rows) <= n_fake:
        raise ValueError('nearest: rows = %r outside [1, %d] (the fakes)' % (rows, n_fake))


def retrieval(real_feats, fake_feats, k, rows, normalize=True, real_bank=None):
    """For the ``rows`` fakes that lie closest to a real (the largest s_j; a tie keeps the lower fake index):
    ``(fake_rows int64 [rows], idx int32 [rows, k], val fp32 [rows, k])``, their indices and their k nearest reals in rank
    order, on the device.  The selection reads the ``s`` vector once and sorts it on the host (stable, so the tie rule is
    exact); the second, small pass finds the k neighbours of the chosen fakes.  ``real_bank``: ``(bankT, n_real)`` of the
    normalised real rows (``real_feats`` is then not read and may be None)."""
    k, rows = int(k), int(rows)
    if not torch.is_tensor(fake_feats) or fake_feats.dim() != 2:
        raise RuntimeError('nearest: the fake features must be a CUDA float32 (n, d) matrix')
    n_r = int(real_bank[1]) if real_bank is not None else (real_feats.shape[0] if torch.is_tensor(real_feats) and real_feats.dim() == 2 else 0)
    check_retrieval(k, rows, n_r, fake_feats.shape[0])                         # (before any GPU work)
    fake = _rows(fake_feats, 'fake', normalize)
    bankT = real_bank[0] if real_bank is not None else features.bank_of(_rows(real_feats, 'real', normalize))
    _, s = neighbours(fake, bankT, n_r, 1)
    chosen = torch.from_numpy(most_similar(s[:, 0].cpu().numpy(), rows)).to(fake.device)      # the one read of s
    idx, val = neighbours(fake.index_select(0, chosen), bankT, n_r, k)
    return chosen, idx, val


def retrieval_grid(real_u8, fake_u8, fake_rows, idx):
    """The figure: a uint8 canvas with one line per chosen fake -- the fake, then its k nearest reals in rank order --
    laid out by ``ops.image_grid_u8(..., nrow=k + 1)`` on the gathered images.  ``fake_rows`` [rows], ``idx`` [rows, k]:
    ``retrieval``'s."""
    features.check_u8(real_u8, 'real', 'nearest')
    features.check_u8(fake_u8, 'fake', 'nearest')
    if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
        raise ValueError('nearest: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
    if idx.dim() != 2 or fake_rows.dim() != 1 or idx.shape[0] != fake_rows.numel() or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise RuntimeError('nearest: fake_rows [rows] and idx [rows, k] expected, got %s and %s' % (tuple(fake_rows.shape), tuple(idx.shape)))
    rows, k = idx.shape
    _, h, w, c = fake_u8.shape
    dev = fake_u8.device
    cells = torch.empty(rows, k + 1, c, h, w, device=dev)
    features.to_float_nchw(fake_u8, fake_rows.to(dev).long(), cells[:, 0])
    near = features.to_float_nchw(real_u8, idx.to(dev).long().reshape(-1), torch.empty(rows * k, c, h, w, device=dev))
    cells[:, 1:].copy_(near.view(rows, k, c, h, w))
    return ops.image_grid_u8(cells.view(rows * (k + 1), c, h, w), nrow=k + 1)


def csv_line(step, out):
    return '%d,%.6f,%.6f' % (step, out['authenticity'], out['nearest_mean'])


def parse_args(argv=None):
    return features.real_fake_parser(
        'Testing script: the memorisation check in the L2-normalised features of a frozen discriminator (one process, one '
        'GPU): the authenticity of the fakes (the share that is NOT closer to its nearest training image than that image is '
        'to its own nearest other training image) and a figure of the fakes closest to a training image next to their '
        'nearest training images.  Comparable only between evaluations under one encoder file; read it against --holdout, '
        'not against 1',
        'file-name tag and seed of the latents of --gen (default: drawn)',
        before_sizes=(('--k', dict(default=8, type=int, help='nearest training images shown per fake (default: 8)')),
                      ('--rows', dict(default=16, type=int,
                                      help='lines of the figure: the fakes with the most similar nearest training image '
                                           '(default: 16; 0: no png)'))),
        after_sizes=(('--holdout', dict(action='store_true',
                                        help='also report holdout_authenticity: the same number for x_test of --real in place '
                                             'of the fakes, the yardstick (a perfect generator scores about this)')),)
    ).parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    if P.rows < 0:
        raise ValueError('--rows must be at least 0, got %r' % (P.rows,))
    held = features.load_images(P.real, 'x_test') if P.holdout else None       # (ValueError without x_test: before the encoder)

    def sizes(n_real, n_fake):
        if n_real < 2:
            raise ValueError('nearest: the real set needs at least 2 images (%d)' % n_real)
        if P.rows:
            check_retrieval(P.k, P.rows, n_real, n_fake)

    def evaluate(E, real, fake, seed):
        if held is not None and tuple(held.shape[1:]) != tuple(real.shape[1:]):
            raise ValueError('%s: x_test holds %s images, x_train %s' % (P.real, tuple(held.shape[1:]), tuple(real.shape[1:])))
        state = real_state_of_images(E, real, P.batch_size)
        fake_feats = features.extract_features(E, fake, P.batch_size)
        out = authenticity(None, fake_feats, real_state=state, normalize=False)
        if held is not None:
            h = authenticity_of(E, None, torch.from_numpy(held).to(real.device), P.batch_size, real_state=state)
            out.update({'holdout_authenticity': h['authenticity'], 'holdout_nearest_mean': h['nearest_mean'], 'n_holdout': h['n_fake']})
        out.update({'k': P.k, 'rows': P.rows})
        if P.rows:
            chosen, idx, val = retrieval(None, fake_feats, P.k, P.rows, normalize=False, real_bank=(state[0], out['n_real']))
            canvas = retrieval_grid(real, fake, chosen, idx)
            out.update({'fakes': chosen.tolist(), 'nearest': idx.tolist(), 'similarity': val.tolist()})
            hostio.write_png(os.path.join(Path(P.fake or P.gen).parent, 'nearest_%d.png' % seed), canvas.cpu().numpy())
        return out

    def line(out):
        text = 'nearest (features of this encoder): [authenticity %.4f] [nearest %.4f, real to real %.4f] on %d fake / %d real images' % (
            out['authenticity'], out['nearest_mean'], out['real_nearest_mean'], out['n_fake'], out['n_real'])
        if 'holdout_authenticity' in out:
            text += ' [holdout authenticity %.4f on %d held-out images]' % (out['holdout_authenticity'], out['n_holdout'])
        return text
    return features.real_fake_main(P, 'the memorisation check runs', sizes, evaluate, line, 'nearest_%d.json')


if __name__ == '__main__':
    main()
