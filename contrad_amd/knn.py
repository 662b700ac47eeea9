"""Weighted k-nearest-neighbour evaluation of a discriminator's penultimate features (Wu et al. 2018; k = 200,
temperature 0.1 is the usual setting of SimCLR-family code bases).  An ADDITION of this project: the reference has no kNN
evaluator.  It is the cheap per-checkpoint probe next to the 100-epoch linear evaluation: one
eval-mode trunk forward per image, one similarity GEMM, one select-and-vote launch per chunk of queries.

    python test_knn.py <run>/dis.pt sndcgan --n_classes 10 --data cifar10.npz
    python test_knn.py <run>/dis.pt sndcgan --synthetic --k 200 --temp 0.1
    python test_knn.py <run>/dis.pt sndcgan --n_classes 3 --data afhq.npz --loo     # + leave-one-out on the training split alone

  * features, the transposed bank and the row chunks of ``S``: contrad_amd/features.py;
  * per chunk csrc/knn.hip reads ``S`` back five times (four radix digits and the compaction) while it is still cached;
  * ``knn_accuracy`` reads the device once, at the end;
  * ``loo_accuracy`` (``--loo``) classifies every image of ONE labelled set by the others: the select kernel leaves the
    query's own column out of its own bank by index (``self0``), so a set without a test split has
    a kNN accuracy too.

``--knn_data`` of the training scripts runs ``knn_accuracy`` at every ``--evaluate_every`` through ``KNNMonitor``
(evaluate/gan.py's ``WeightsMonitor``: a discriminator of its own, so that the training trajectory does not move by a bit).
"""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import features, ops
from .evaluate.gan import WeightsMonitor, own_network
from .hooks import Hook
from .lineval import load_npz, synthetic_set
from .models.gan import get_architecture


def check_labels(y, n_classes, what='labels'):
    """Host-side range check of a label array (as lineval.main does before it uploads)."""
    y = np.asarray(y)
    if y.size and (int(y.min()) < 0 or int(y.max()) >= n_classes):
        raise ValueError('%s in [%d, %d] with n_classes %d' % (what, int(y.min()), int(y.max()), n_classes))


class KNNClassifier(object):
    """Weighted kNN vote against a bank of ``n`` labelled feature rows.  ``bank_feats``: CUDA fp32 [n, d], or with
    ``transposed=True`` the [d][round_up(n, 4)] bank itself (``features.new_bank`` filled by ``features.extract_features``;
    kept, not copied).  ``normalize``: L2-normalise bank and query rows here (False: the caller did, as
    ``extract_features`` does).
    ``k`` is clamped to the bank size."""

    def __init__(self, bank_feats, bank_labels, n_classes, k=200, temp=0.1, normalize=True, transposed=False):
        if not torch.is_tensor(bank_feats) or not bank_feats.is_cuda or bank_feats.dtype != torch.float32 \
                or bank_feats.dim() != 2:
            raise RuntimeError('knn: the bank must be a CUDA float32 matrix')
        if not float(temp) > 0:
            raise ValueError('knn: temp must be positive, got %r' % (temp,))
        if int(k) < 1:
            raise ValueError('knn: k must be at least 1, got %r' % (k,))
        if not 1 <= int(n_classes) <= ops.KNN_MAX_CLASSES:
            raise ValueError('knn: n_classes = %r outside [1, %d]' % (n_classes, ops.KNN_MAX_CLASSES))
        dev = bank_feats.device
        if not torch.is_tensor(bank_labels) or not bank_labels.is_cuda:      # host labels are checked before the upload
            check_labels(np.asarray(bank_labels), n_classes, 'bank labels')
            bank_labels = torch.as_tensor(np.asarray(bank_labels), dtype=torch.int64).to(dev)
        self.labels = bank_labels.to(torch.int64).contiguous()
        self.n = self.labels.numel()
        if self.n < 1:
            raise ValueError('knn: empty bank')
        if transposed:
            if normalize:
                raise ValueError('knn: a transposed bank is taken as it is (normalize=False)')
            if bank_feats.shape[1] != ops.round_up(self.n, 4) or not bank_feats.is_contiguous():
                raise RuntimeError('knn: a transposed bank of %d rows is a contiguous [d][%d] matrix'
                                   % (self.n, ops.round_up(self.n, 4)))
            self.bankT = bank_feats
        else:
            if bank_feats.shape[0] != self.n:
                raise RuntimeError('knn: %d labels for %d bank rows' % (self.n, bank_feats.shape[0]))
            self.bankT = features.bank_of(features.normalize_rows(bank_feats) if normalize else bank_feats)
        self.d, self.n_pad = self.bankT.shape
        self.n_classes, self.normalize = int(n_classes), bool(normalize)
        self.k = min(int(k), self.n)
        if self.k > ops.KNN_MAX_K:
            raise ValueError('knn: k = %d above the kernel limit %d' % (self.k, ops.KNN_MAX_K))
        self.inv_temp = 1.0 / float(temp)
        self.chunk_rows = features.chunk_rows_of(self.n_pad)

    def predict(self, feats, neighbours=False, leave_self_out=False):
        """(pred int32 [M], scores [M, n_classes]) of the query rows ``feats`` [M, d]; with ``neighbours`` also
        (idx int32 [M, k], val [M, k]).  ``leave_self_out``: ``feats`` are the bank's own rows in the bank's order (M == n)
        and row i does not vote for itself -- column i is left out by index (csrc/knn.hip's ``self0``), k is clamped to
        n - 1."""
        if not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 \
                or feats.shape[1] != self.d:
            raise RuntimeError('knn: queries must be a CUDA float32 [M, %d] matrix' % self.d)
        M, dev = feats.shape[0], feats.device
        k = self.k
        if leave_self_out:
            if M != self.n:
                raise ValueError('knn: leave_self_out takes the rows of the bank itself (%d rows, a bank of %d)' % (M, self.n))
            if self.n < 2:
                raise ValueError('knn: leave_self_out needs a bank of at least 2 rows')
            k = min(k, self.n - 1)
        q = features.normalize_rows(feats) if self.normalize else feats.contiguous()
        pred = torch.empty(M, device=dev, dtype=torch.int32)
        scores = torch.empty(M, self.n_classes, device=dev)
        idx = torch.empty(M, k, device=dev, dtype=torch.int32) if neighbours else None
        val = torch.empty(M, k, device=dev) if neighbours else None
        for i, Sc in features.similarity_chunks(q, self.bankT, chunk_rows=self.chunk_rows):
            m = Sc.shape[0]
            ci, cv, cs, cp = ops.knn_select(Sc, self.n, self.labels, self.n_classes, k, self.inv_temp,
                                            self0=i if leave_self_out else -1)
            pred[i:i + m].copy_(cp)
            scores[i:i + m].copy_(cs)
            if neighbours:
                idx[i:i + m].copy_(ci)
                val[i:i + m].copy_(cv)
        return (pred, scores, idx, val) if neighbours else (pred, scores)


def to_device(data, n_classes, device):
    """The four arrays of ``lineval.load_npz`` / ``lineval.synthetic_set`` on the device, labels range-checked on the host."""
    out = {}
    for split in ('train', 'test'):
        check_labels(data['y_' + split], n_classes, 'y_' + split)
        out['x_' + split] = torch.from_numpy(np.ascontiguousarray(data['x_' + split])).to(device)
        out['y_' + split] = torch.from_numpy(np.asarray(data['y_' + split]).astype(np.int64)).to(device)
    return out


def knn_accuracy(D, data, n_classes, k=200, temp=0.1, batch=500):
    """Top-1 accuracy (percent) of the weighted kNN vote: bank = the training split, queries = the test split, both as
    ``D``'s normalised penultimate features.  ``data``: the dict of ``lineval.load_npz`` / ``lineval.synthetic_set`` (numpy),
    or the result of ``to_device`` (kept by a caller that evaluates repeatedly).  ``D``: on the GPU, in eval mode."""
    dev = next(D.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError('kNN evaluation runs on the MI355X HIP path only (no CPU fallback)')
    if not torch.is_tensor(data['x_train']):
        data = to_device(data, n_classes, dev)
    n_train, n_test = data['x_train'].shape[0], data['x_test'].shape[0]
    if n_train < 1 or n_test < 1:
        raise ValueError('knn_accuracy: empty split (%d training, %d test images)' % (n_train, n_test))
    bankT = features.extract_features(D, data['x_train'], batch, bankT=features.new_bank(n_train, D.d_penul, dev))
    clf = KNNClassifier(bankT, data['y_train'], n_classes, k=k, temp=temp, normalize=False, transposed=True)
    pred, _ = clf.predict(features.extract_features(D, data['x_test'], batch))
    hits = (pred.long() == data['y_test']).sum()
    return {'acc@1': 100.0 * int(hits.item()) / n_test, 'n_test': n_test}       # the one device-to-host read


def loo_accuracy(D, x_u8, y, n_classes, k=200, temp=0.1, batch=500):
    """Leave-one-out top-1 accuracy (percent) of the weighted kNN vote on ONE labelled set (no test split, as AFHQ has none):
    every image is classified by the others, its own column left out of its row by index; k is clamped to n - 1.  ``x_u8``:
    device-resident uint8 [n, H, W, 3]; ``y``: its labels (host array, range-checked here, or a CUDA tensor).  ``D``: on the
    GPU, in eval mode."""
    features.check_u8(x_u8, 'given', 'knn.loo_accuracy')
    n, dev = x_u8.shape[0], x_u8.device
    if n < 2:
        raise ValueError('knn.loo_accuracy: %d image: leave-one-out needs at least 2' % n)
    if not torch.is_tensor(y):
        check_labels(y, n_classes, 'labels')
        y = torch.from_numpy(np.asarray(y).astype(np.int64)).to(dev)
    feats = features.extract_features(D, x_u8, batch)
    clf = KNNClassifier(feats, y, n_classes, k=k, temp=temp, normalize=False)
    pred, _ = clf.predict(feats, leave_self_out=True)
    hits = (pred.long() == clf.labels).sum()
    return {'acc@1': 100.0 * int(hits.item()) / n, 'n': n, 'k': min(clf.k, n - 1)}      # the one device-to-host read


class KNNMonitor(WeightsMonitor):
    """``--knn_data`` on rank 0: the kNN accuracy of the training discriminator's weights at every evaluation, appended
    as ``step,acc@1`` to ``knn_<eval_seed>.csv`` (evaluate/gan.py's ``WeightsMonitor``).  The uint8 sets go to the device
    once, here."""

    def __init__(self, logdir, architecture, image_size, device, seed, data_path, n_classes=None, k=200, temp=0.1, batch=500,
                 P=None):
        data = load_npz(data_path)
        for split in ('train', 'test'):
            if tuple(data['x_' + split].shape[1:]) != tuple(image_size):
                raise ValueError('%s: x_%s holds %s images, the discriminator takes %s'
                                 % (data_path, split, tuple(data['x_' + split].shape[1:]), tuple(image_size)))
        if n_classes is None:
            n_classes = int(max(data['y_train'].max(), data['y_test'].max())) + 1
        self.n_classes, self.k, self.temp, self.batch = n_classes, k, temp, batch
        self.data = to_device(data, n_classes, device)
        super().__init__(logdir, device, seed, own_network('D', architecture, image_size, device, P),
                         [('knn_%d.csv', 'step,acc@1', lambda step, out: '%d,%.4f' % (step, out['acc@1']))], which='D')

    def evaluate(self):
        return knn_accuracy(self.D, self.data, self.n_classes, self.k, self.temp, self.batch)


# ---- the training scripts' hook: ordinary defaults (the attributes are on every parsed namespace), --knn_k alone passes ----
HOOK = Hook(
    flags=(('knn_data', None, dict(type=str, help='npz with x_train, y_train, x_test, y_test: rank 0 appends the weighted-kNN accuracy of D\'s '
                                                  'penultimate features to knn_<seed>.csv at every evaluate_every; the training trajectory is unchanged')),
           ('knn_k', 200, dict(type=int, help='with --knn_data: neighbours (default: 200)')),
           ('knn_temp', 0.1, dict(type=float, help='with --knn_data: vote temperature (default: 0.1)'))),
    switch='knn_data', shown='D', suppressed=False,
    build=lambda H, run: KNNMonitor(*run.head, H.knn_data, k=H.knn_k, temp=H.knn_temp, P=run.P),
    log_lines=lambda monitor, step, out: ['[Steps %7d] [kNN Acc@1 %.3f]' % (step, out['acc@1'])])
add_hook_arguments = HOOK.add_arguments


def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: weighted kNN evaluation (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (discriminator) model checkpoint')
    parser.add_argument('architecture', type=str, help='Architecture')
    parser.add_argument('--n_classes', type=int, default=10, help='Number of classes (default: 10)')
    parser.add_argument('--data', default=None, type=str, help='npz with x_train, y_train, x_test, y_test')
    parser.add_argument('--synthetic', action='store_true', help='seeded learnable set instead of a dataset')
    parser.add_argument('--synthetic_size', default=(50000, 10000), type=int, nargs=2, metavar=('TRAIN', 'TEST'))
    parser.add_argument('--synthetic_image', default=32, type=int, help='side of the synthetic images (default: 32)')
    parser.add_argument('--k', default=200, type=int, help='neighbours (default: 200; clamped to the bank size)')
    parser.add_argument('--temp', default=0.1, type=float, help='vote temperature (default: 0.1)')
    parser.add_argument('--batch_size', default=500, type=int, help='images per trunk forward (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help='file-name tag and seed of --synthetic (default: drawn)')
    parser.add_argument('--loo', action='store_true',
                        help='also the leave-one-out accuracy on the training split alone (every image classified by the '
                             'others, k clamped to n - 1): the probe for a labelled set without a test split; adds the key '
                             '"loo" to the json')
    return parser.parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('kNN evaluation runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.synthetic:
        data = synthetic_set(seed, P.n_classes, P.synthetic_size[0], P.synthetic_size[1], size=P.synthetic_image)
    elif P.data:
        data = load_npz(P.data)
    else:
        raise RuntimeError('no dataset reader is installed here: pass --data FILE.npz (x_train, y_train, x_test, '
                           'y_test) or --synthetic')
    image_size = tuple(data['x_train'].shape[1:])                          # the image size comes from the data
    D = features.load_frozen(get_architecture(P.architecture, image_size)[1], P.model_path, dev)
    out = knn_accuracy(D, data, P.n_classes, P.k, P.temp, P.batch_size)
    out.update({'k': min(P.k, len(data['y_train'])), 'temp': P.temp, 'n_train': int(len(data['y_train']))})
    print('kNN (k %d, T %g): [Acc@1 %.3f] on %d test images, bank of %d' % (
        out['k'], P.temp, out['acc@1'], out['n_test'], out['n_train']), flush=True)
    if P.loo:
        out['loo'] = loo_accuracy(D, torch.from_numpy(np.ascontiguousarray(data['x_train'])).to(dev), data['y_train'], P.n_classes,
                                  P.k, P.temp, P.batch_size)
        print('kNN leave-one-out (k %d, T %g): [Acc@1 %.3f] on the %d training images' % (
            out['loo']['k'], P.temp, out['loo']['acc@1'], out['loo']['n']), flush=True)
    path = os.path.join(Path(P.model_path).parent, 'knn_%d.json' % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    return path


if __name__ == '__main__':
    main()
