"""Linear evaluation of a trained discriminator's penultimate features: the reference's ``test_lineval.py`` on the
MI355X path.  Same CLI (``model_path architecture --n_classes --batch_size``), same recipe (D in eval mode, a fresh
``LinearWrapper(d_penul, n_classes)`` head, SGD lr 0.1 without momentum, MultiStepLR 60 / 75 / 90 x 0.1, 100 epochs,
RandomResizedCrop(scale 0.2 - 1) + flip on the training images), same files next to the checkpoint
(``lin_eval_<seed>.csv`` with ``epoch,time,lr,train loss,train acc,test loss,test acc`` and ``lin_eval_<seed>.pth.tar``
holding ``{'epoch', 'state_dict'}`` after every epoch).

One training iteration is the crop + flip kernel, the eval-mode trunk forward and the three launches of
csrc/linhead.hip; loss and accuracy sums stay on the device and are read once per epoch.  ``--graph`` replays that
iteration from a hipGraph captured once per batch shape (the full batch and the epoch's remainder); the learning rate
is read from device memory, so the same graph serves every milestone.  Eager and ``--graph`` runs write bitwise-equal
checkpoints.

Declared deviation: the reference augments uint8 images with PIL in loader workers; here the whole set lives on the
device as uint8 and the crop is the project's RandomResizeCropLayer parameterisation (bilinear ``grid_sample``
semantics on floats).  Same distribution family, not the same pixels.

Data: ``--data FILE.npz`` with ``x_train`` uint8 [n, 32, 32, 3], ``y_train``, ``x_test``, ``y_test`` (the arrays of the
CIFAR python pickles), or ``--synthetic``: a seeded learnable set (class-dependent colour pattern + noise).
"""
import json
import os
import time
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import config, ops
from .augment import SimCLRAugment
from .captured import EagerFirst, capture
from .evaluate.classifier import new_meters, summarize, test_classifier
from .features import to_float_nchw
from .hostio import THROTTLE, upload, upload_into
from .models.gan import get_architecture
from .models.gan.base import LinearWrapper

CSV_HEADER = 'epoch,time,lr,train loss,train acc,test loss,test acc'
MILESTONES, GAMMA, BASE_LR = (60, 75, 90), 0.1, 0.1
LIN_DATASETS = {'cifar10': 10, 'cifar10_hflip': 10, 'cifar100': 100, 'cifar100_hflip': 100}


def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: Linear evaluation (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (discriminator) model checkpoint')
    parser.add_argument('architecture', type=str, help='Architecture')
    parser.add_argument('--n_classes', type=int, default=10, help='Number of classes (default: 10)')
    parser.add_argument('--batch_size', default=256, type=int, help='Batch size (default: 256)')
    # additions
    parser.add_argument('--data', default=None, type=str, help='npz with x_train, y_train, x_test, y_test')
    parser.add_argument('--synthetic', action='store_true', help='seeded learnable set instead of a dataset')
    parser.add_argument('--synthetic_size', default=(50000, 10000), type=int, nargs=2, metavar=('TRAIN', 'TEST'))
    parser.add_argument('--seed', default=None, type=int, help='RNG seed and file-name tag (default: drawn)')
    parser.add_argument('--epochs', default=100, type=int)
    parser.add_argument('--graph', action='store_true', help='replay the training iteration from captured hipGraphs')
    return parser.parse_args(argv)


def load_npz(path):
    """The four arrays of an image-classification set, validated: images uint8 [n, H, W, 3], labels int64 [n]."""
    out = {}
    with np.load(path) as z:
        for split in ('train', 'test'):
            x, y = np.asarray(z['x_' + split]), np.asarray(z['y_' + split]).reshape(-1)
            if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
                raise ValueError('%s: x_%s must be uint8 [n, H, W, 3], got %s %s' % (path, split, x.dtype, x.shape))
            if len(y) != len(x):
                raise ValueError('%s: %d labels for %d images in %s' % (path, len(y), len(x), split))
            out['x_' + split], out['y_' + split] = x, y.astype(np.int64)
    return out


def synthetic_set(seed, n_classes, n_train=50000, n_test=10000, size=32, noise=0.2):
    """A learnable stand-in for CIFAR: every class has a random 4 x 4 colour pattern (blown up to size x size); an
    image is its class's pattern plus Gaussian pixel noise.  Deterministic in ``seed``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cell = size // 4
    patterns = rng.uniform(0.15, 0.85, (n_classes, 4, 4, 3)).astype(np.float32)
    patterns = patterns.repeat(cell, axis=1).repeat(cell, axis=2)
    out = {}
    for split, n in (('train', n_train), ('test', n_test)):
        y = rng.integers(0, n_classes, n).astype(np.int64)
        x = np.empty((n, size, size, 3), np.uint8)
        for i in range(0, n, 8192):
            yy = y[i:i + 8192]
            v = patterns[yy] + noise * rng.standard_normal((len(yy), size, size, 3), dtype=np.float32)
            x[i:i + 8192] = np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)
        out['x_' + split], out['y_' + split] = x, y
    return out


def lr_at(epoch):
    """MultiStepLR(milestones 60 / 75 / 90, gamma 0.1) on lr 0.1, in the scheduler's own chained arithmetic."""
    lr = BASE_LR
    for m in MILESTONES:
        if epoch >= m:
            lr = lr * GAMMA
    return lr


def checkpoint_keys(D):
    """Key list of the ``state_dict`` lin-eval saves: D's keys with ``linear.weight`` / ``linear.bias`` as the head."""
    return list(D.state_dict().keys())


def install_head(D, n_classes):
    """``model.linear = LinearWrapper(model.d_penul, n_classes)`` (nn.Linear's default init from the host torch RNG)."""
    D.linear = LinearWrapper(D.d_penul, n_classes)
    return D.linear


def save_checkpoint(D, epoch, path):
    torch.save({'epoch': epoch, 'state_dict': D.state_dict()}, path)


class HeadStep(object):
    """One training iteration at a fixed batch size on static buffers: crop + flip, eval-mode trunk forward, launches
    1 - 3 of the head.  The eager form runs the body; with ``graph=True`` the body is captured at the second use of
    this batch size (the first runs eagerly: first-use allocations and module loads must not land in a capture) and
    replayed afterwards.  Both forms run the same launches on the same buffers, hence the same bits."""

    def __init__(self, D, aug, n, image_size, meters, lr_dev, graph):
        h, w, c = image_size
        dev = meters.device
        self.D, self.aug, self.n, self.use_graph = D, aug, n, graph
        self.images = torch.zeros(n, c, h, w, device=dev)
        self.labels = torch.zeros(n, dtype=torch.int64, device=dev)
        self.params = torch.zeros(n, ops.AUG_NPARAM, device=dev)
        self.dlogits = torch.zeros(n, D.linear.out_features, device=dev)
        self.meters, self.lr = meters, lr_dev
        self.graph, self.first, self._scratch = None, EagerFirst(), {}

    def _body(self):
        head = self.D.linear
        with torch.no_grad():
            x = ops.simclr_augment(self.images, self.params, -1, self.aug.r_c is not None)
            feats = self.D.penultimate(x)
            ops.linhead_fwd(feats, head.weight, head.bias, y=self.labels, dlogits=self.dlogits, meters=self.meters,
                            want_logits=False)
            ops.linhead_wgrad_sgd(feats, self.dlogits, head.weight, head.bias, lr=self.lr)

    def __call__(self, x_u8, y_dev, idx):
        to_float_nchw(x_u8, idx, self.images)
        self.labels.copy_(y_dev.index_select(0, idx))
        P, _cf, _ = self.aug.sample(self.n, self.images.shape[2], self.images.shape[3])     # (column 15: the colour-op order)
        upload_into(P, self.params)
        if not self.use_graph or not self.first.may_capture():
            return self._body()
        if self.graph is None:
            self.graph, _ = capture(self._body, (self.D,), self._scratch)
        self.graph.replay()


def _batches(x_u8, y_dev, batch):
    """Unshuffled float NCHW batches of a device-resident uint8 set (the test loader)."""
    n = x_u8.shape[0]
    for i in range(0, n, batch):
        idx = torch.arange(i, min(i + batch, n), device=x_u8.device)
        yield x_u8.index_select(0, idx).permute(0, 3, 1, 2).float().div_(255.0), y_dev.index_select(0, idx)


def train_epoch(steps, x_u8, y_dev, batch, D, aug, image_size, meters, lr_dev, graph):
    """One pass over the training set in a fresh host permutation (torch RNG, as DataLoader(shuffle=True) draws it)."""
    n = x_u8.shape[0]
    if n >= 1 << 24:
        raise NotImplementedError('the shuffle is handed over as floats: fewer than 2^24 images')
    perm = upload(torch.randperm(n).float().view(n, 1), x_u8.device).view(n).long()
    meters.zero_()
    for i in range(0, n, batch):
        idx = perm[i:i + batch]
        m = idx.numel()
        if m not in steps:
            steps[m] = HeadStep(D, aug, m, image_size, meters, lr_dev, graph)
        THROTTLE.begin()                          # the host stays at most one iteration ahead (hostio.py)
        steps[m](x_u8, y_dev, idx)
        THROTTLE.end()
    return summarize(meters)                      # the epoch's one device-to-host read


def _dataset_name(logdir):
    gins = sorted(Path(logdir).glob('*.gin'))
    if not gins:
        return None
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'), str(gins[0])])
    return config.get_bindings('options').get('dataset')


def main(argv=None):
    P = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('linear evaluation runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    logdir = Path(P.model_path).parent
    dataset = _dataset_name(logdir)
    if dataset is not None and dataset not in LIN_DATASETS:
        raise NotImplementedError("linear evaluation of dataset '%s' (implemented: %s)" % (dataset, sorted(LIN_DATASETS)))
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    torch.manual_seed(seed); np.random.seed(seed)
    if P.synthetic:
        data = synthetic_set(seed, P.n_classes, *P.synthetic_size)
    elif P.data:
        data = load_npz(P.data)
    else:
        raise RuntimeError('no dataset reader is installed here: pass --data FILE.npz (x_train, y_train, x_test, '
                           'y_test) or --synthetic')
    image_size = tuple(data['x_train'].shape[1:])
    x_train, y_train = torch.from_numpy(data['x_train']).to(dev), torch.from_numpy(data['y_train']).to(dev)
    x_test, y_test = torch.from_numpy(data['x_test']).to(dev), torch.from_numpy(data['y_test']).to(dev)
    if int(data['y_train'].max()) >= P.n_classes or int(data['y_test'].max()) >= P.n_classes:
        raise ValueError('labels up to %d with --n_classes %d' % (int(data['y_train'].max()), P.n_classes))

    _, D = get_architecture(P.architecture, image_size)
    D.load_state_dict(torch.load(P.model_path, map_location='cpu'))
    D.eval()
    install_head(D, P.n_classes)
    D.to(dev)
    for p in D.parameters():
        p.requires_grad_(False)
    aug = SimCLRAugment(scale=(0.2, 1.0), p_jitter=0.0, p_gray=0.0)

    logfile = os.path.join(logdir, 'lin_eval_%d.csv' % seed)
    save_path = os.path.join(logdir, 'lin_eval_%d.pth.tar' % seed)
    with open(logfile, 'w') as f:
        f.write(CSV_HEADER + '\n')
    meters, lr_dev = new_meters(dev), torch.zeros(1, device=dev)
    init = test_classifier(D, _batches(x_test, y_test, P.batch_size), ['loss', 'error@1'])
    print('untrained head: [Loss %.3f] [Err@1 %.3f]' % (init['loss'], init['error@1']), flush=True)
    with open(os.path.join(logdir, 'lin_eval_%d.json' % seed), 'w') as f:
        json.dump({'initial test loss': init['loss'], 'initial test acc': 100 - init['error@1']}, f)
    steps = {}
    for epoch in range(P.epochs):
        before = time.time()
        lr = lr_at(epoch)
        lr_dev.fill_(lr)
        train_out = train_epoch(steps, x_train, y_train, P.batch_size, D, aug, image_size, meters, lr_dev, P.graph)
        test_out = test_classifier(D, _batches(x_test, y_test, P.batch_size), ['loss', 'error@1'])
        with open(logfile, 'a') as f:
            f.write('{},{:.8},{:.4},{:.4},{:.4},{:.4},{:.4}\n'.format(
                epoch, time.time() - before, lr, train_out['loss'], train_out['acc@1'], test_out['loss'],
                100 - test_out['error@1']))
        print('Epoch %d: train [Loss %.4f] [Acc@1 %.3f] [Acc@5 %.3f]   test [Loss %.3f] [Err@1 %.3f]' % (
            epoch, train_out['loss'], train_out['acc@1'], train_out['acc@5'], test_out['loss'], test_out['error@1']),
            flush=True)
        save_checkpoint(D, epoch + 1, save_path)
    return save_path


if __name__ == '__main__':
    main()
