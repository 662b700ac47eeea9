"""Weighted k-nearest-neighbour evaluation of a discriminator's penultimate features (Wu et al. 2018; k = 200,
temperature 0.1 is the usual setting of SimCLR-family code bases).  An ADDITION of this project: the reference has no kNN
evaluator.  It is the cheap per-checkpoint probe next to the 100-epoch linear evaluation: one
eval-mode trunk forward per image, one similarity GEMM, one select-and-vote launch per chunk of queries.

    python test_knn.py <run>/dis.pt sndcgan --n_classes 10 --data cifar10.npz
    python test_knn.py <run>/dis.pt sndcgan --synthetic --k 200 --temp 0.1

  * features: ``D.penultimate`` under ``no_grad`` in eval mode (no power iteration, no augmentation), rows L2-normalised
    by ``contrad_l2norm_fwd`` (x / max(||x||, 1e-12), F.normalize's rule);
  * the bank is kept transposed, [d][n_pad] with n_pad = round_up(n, 4) and zero padding columns: the packed weight
    layout of the conv engine, so ``S = Q bank^T`` is ``ops.conv2d_fwd`` on a (m, 1, 1, d) input;
  * queries go through in row chunks of about 64 MB of ``S``: the GEMM writes a chunk, csrc/knn.hip reads it back five
    times (four radix digits and the compaction) while it is still cached;
  * ``knn_accuracy`` reads the device once, at the end.

``--knn_data`` of the training scripts runs ``knn_accuracy`` at every ``--evaluate_every`` through ``KNNMonitor``, which
follows evaluate/gan.py's ``Monitor``: a discriminator of its own, so that the training trajectory does not move by a bit.
"""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import ops
from .evaluate.gan import eval_seed_of, preserved_rng
from .lineval import _to_float_nchw, load_npz, synthetic_set
from .models.gan import get_architecture

S_CHUNK_FLOATS = 1 << 24          # one chunk of S: 64 MB
MAX_CHUNK_ROWS = 512


def check_labels(y, n_classes, what='labels'):
    """Host-side range check of a label array (as lineval.main does before it uploads)."""
    y = np.asarray(y)
    if y.size and (int(y.min()) < 0 or int(y.max()) >= n_classes):
        raise ValueError('%s in [%d, %d] with n_classes %d' % (what, int(y.min()), int(y.max()), n_classes))


def normalize_rows(feats):
    """x / max(||x||_2, 1e-12) per row of a CUDA fp32 (n, d) matrix (contrad_l2norm_fwd)."""
    if feats.dim() != 2:
        raise RuntimeError('knn: features must be an (n, d) matrix, got %s' % (tuple(feats.shape),))
    if feats.stride(-1) != 1:
        feats = feats.contiguous()
    return ops.l2norm_fwd(feats)[0]


def new_bank(n, d, device):
    """The transposed bank [d][round_up(n, 4)], zero-filled (the padding columns stay zero)."""
    return torch.zeros(d, ops.round_up(n, 4), device=device, dtype=torch.float32)


def extract_features(D, x_u8, batch, bankT=None):
    """Normalised penultimate features of the device-resident uint8 set ``x_u8`` [n, H, W, 3], ``batch`` images per
    forward.  Returns them as [n, d]; with ``bankT`` (``new_bank(n, d, device)``) writes column i of the bank per image
    instead and returns ``bankT``.  ``D`` must be in eval mode (the caller's business: this function touches no mode)."""
    if D.training:
        raise RuntimeError('knn.extract_features: D must be in eval mode (train mode runs a power iteration per call)')
    if not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise RuntimeError('knn.extract_features: images must be a CUDA uint8 [n, H, W, 3] tensor')
    n, h, w, c = x_u8.shape
    dev = x_u8.device
    if batch < 1:
        raise ValueError('knn.extract_features: batch must be at least 1, got %r' % (batch,))
    rows = None
    buf = torch.empty(min(batch, n), c, h, w, device=dev)
    with torch.no_grad():
        for i in range(0, n, batch):
            m = min(batch, n - i)
            x = _to_float_nchw(x_u8, torch.arange(i, i + m, device=dev), buf[:m])
            z = normalize_rows(D.penultimate(x).reshape(m, -1))
            if bankT is not None:
                bankT[:, i:i + m].copy_(z.t())
                continue
            if rows is None:
                rows = torch.empty(n, z.shape[1], device=dev)
            rows[i:i + m].copy_(z)
    return bankT if bankT is not None else rows


class KNNClassifier(object):
    """Weighted kNN vote against a bank of ``n`` labelled feature rows.  ``bank_feats``: CUDA fp32 [n, d], or with
    ``transposed=True`` the [d][round_up(n, 4)] bank itself (``new_bank`` + ``extract_features``; kept, not copied).
    ``normalize``: L2-normalise bank and query rows here (False: the caller did, as ``extract_features`` does).
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
            self.bankT = new_bank(self.n, bank_feats.shape[1], dev)
            self.bankT[:, :self.n].copy_((normalize_rows(bank_feats) if normalize else bank_feats).t())
        self.d, self.n_pad = self.bankT.shape
        self.n_classes, self.normalize = int(n_classes), bool(normalize)
        self.k = min(int(k), self.n)
        if self.k > ops.KNN_MAX_K:
            raise ValueError('knn: k = %d above the kernel limit %d' % (self.k, ops.KNN_MAX_K))
        self.inv_temp = 1.0 / float(temp)
        self.chunk_rows = max(1, min(MAX_CHUNK_ROWS, S_CHUNK_FLOATS // self.n_pad))

    def similarities(self, q, out):
        """out[m][n_pad] = q[m][d] bank^T on the conv engine (a linear layer whose packed weight is the bank)."""
        m = q.shape[0]
        ops.conv2d_fwd(q.view(m, 1, 1, self.d), self.bankT, None, self.n_pad, 1, 1, 1, 0, out=out.view(m, 1, 1, self.n_pad))
        return out

    def predict(self, feats, neighbours=False):
        """(pred int32 [M], scores [M, n_classes]) of the query rows ``feats`` [M, d]; with ``neighbours`` also
        (idx int32 [M, k], val [M, k])."""
        if not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 \
                or feats.shape[1] != self.d:
            raise RuntimeError('knn: queries must be a CUDA float32 [M, %d] matrix' % self.d)
        M, dev = feats.shape[0], feats.device
        q = normalize_rows(feats) if self.normalize else feats.contiguous()
        pred = torch.empty(M, device=dev, dtype=torch.int32)
        scores = torch.empty(M, self.n_classes, device=dev)
        idx = torch.empty(M, self.k, device=dev, dtype=torch.int32) if neighbours else None
        val = torch.empty(M, self.k, device=dev) if neighbours else None
        S = torch.empty(min(self.chunk_rows, max(M, 1)), self.n_pad, device=dev)
        for i in range(0, M, self.chunk_rows):
            m = min(self.chunk_rows, M - i)
            Sc = self.similarities(q[i:i + m], S[:m])
            ci, cv, cs, cp = ops.knn_select(Sc, self.n, self.labels, self.n_classes, self.k, self.inv_temp)
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
    bankT = extract_features(D, data['x_train'], batch, bankT=new_bank(n_train, D.d_penul, dev))
    clf = KNNClassifier(bankT, data['y_train'], n_classes, k=k, temp=temp, normalize=False, transposed=True)
    pred, _ = clf.predict(extract_features(D, data['x_test'], batch))
    hits = (pred.long() == data['y_test']).sum()
    return {'acc@1': 100.0 * int(hits.item()) / n_test, 'n_test': n_test}       # the one device-to-host read


class KNNMonitor(object):
    """``--knn_data`` on rank 0: the kNN accuracy of the training discriminator's weights at every evaluation, appended
    as ``step,acc@1`` to ``knn_<eval_seed>.csv``.  Like evaluate/gan.py's ``Monitor`` it owns its module (built inside
    ``preserved_rng``, always in eval mode, never requiring grad) and loads the training D's state dict at each
    evaluation: D's mode, u / v, packed-weight caches and captured graphs are not touched, the random streams not read."""

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
        self.data = to_device(data, n_classes, device)                     # the uint8 sets go to the device once
        self.device = device
        self.path = os.path.join(logdir, 'knn_%d.csv' % eval_seed_of(seed))
        with preserved_rng(device):                                        # the constructors draw the initial weights
            _, D = get_architecture(architecture, image_size, P=P)
        self.D = D.to(device).eval()
        for p in self.D.parameters():
            p.requires_grad_(False)
        if not os.path.exists(self.path):                                  # (a resumed run appends to its file)
            with open(self.path, 'w') as f:
                f.write('step,acc@1\n')

    def update(self, step, discriminator):
        with torch.no_grad(), preserved_rng(self.device):
            self.D.load_state_dict(discriminator.state_dict())
            self.D.eval()
            out = knn_accuracy(self.D, self.data, self.n_classes, self.k, self.temp, self.batch)
        with open(self.path, 'a') as f:
            f.write('%d,%.4f\n' % (step, out['acc@1']))
        return out


def add_hook_arguments(parser):
    """The three flags of the training scripts."""
    parser.add_argument('--knn_data', default=None, type=str,
                        help='npz with x_train, y_train, x_test, y_test: rank 0 appends the weighted-kNN accuracy of D\'s '
                             'penultimate features to knn_<seed>.csv at every evaluate_every; the training trajectory is unchanged')
    parser.add_argument('--knn_k', default=200, type=int, help='with --knn_data: neighbours (default: 200)')
    parser.add_argument('--knn_temp', default=0.1, type=float, help='with --knn_data: vote temperature (default: 0.1)')


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
    _, D = get_architecture(P.architecture, image_size)
    D.load_state_dict(torch.load(P.model_path, map_location='cpu'))
    D = D.to(dev).eval()
    for p in D.parameters():
        p.requires_grad_(False)
    out = knn_accuracy(D, data, P.n_classes, P.k, P.temp, P.batch_size)
    out.update({'k': min(P.k, len(data['y_train'])), 'temp': P.temp, 'n_train': int(len(data['y_train']))})
    print('kNN (k %d, T %g): [Acc@1 %.3f] on %d test images, bank of %d' % (
        out['k'], P.temp, out['acc@1'], out['n_test'], out['n_train']), flush=True)
    path = os.path.join(Path(P.model_path).parent, 'knn_%d.json' % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    return path


if __name__ == '__main__':
    main()
