"""Real-image batches for the training loops without torchvision: the whole training set lives on the device as uint8
[n, H, W, 3] (150 MB for CIFAR), and a batch is ONE launch of csrc/data.hip (gather by index, flip, NHWC -> NCHW,
``/ 255``) driven by a (batch, 2) float block of host draws -- 4 KB at batch 512, one 64 KB piece of ``hostio.upload``
at most, instead of the 6.3 MB float batch the reference's ``images.cuda(non_blocking=True)`` ships per step.

What is kept from the reference's loaders (train_gan.py / train_stylegan2.py of this package, which mirror it):
  * the ORDER: ``index_plan`` is ``DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=seed)``
    after ``set_epoch(epoch)``, batched by ``BatchSampler(..., batch, drop_last)``, index for index;
  * the PIXELS: bit-equal to ``ToTensor`` (``x.float().div(255)``), flipped rows bit-equal to its ``.flip(-1)``.

Declared deviation: the reference flips in loader workers, each with its own RNG stream, so its flips are not
reproducible from the seed.  Here they come from the main process's torch CPU generator: one ``torch.rand(m) < 0.5`` per
batch, drawn BEFORE the step's own draws (latents, augmentation parameters); a loader without flip draws nothing.  Same
distribution (every image mirrored with probability 1/2, independently), reproducible runs.

File format: the ``.npz`` that ``test_lineval.py --data`` reads (tools/make_image_npz.py writes it); only ``x_train``
(and ``y_train`` when present) are read here.
"""
import numpy as np
import torch

from . import ops
from .hostio import upload


def load_train_npz(path):
    """``{'x_train': uint8 [n, H, W, 3], 'y_train': int64 [n] or None}`` of an image-set npz, validated."""
    with np.load(path) as z:
        if 'x_train' not in z.files:
            raise ValueError('%s: no array x_train (found %s)' % (path, sorted(z.files)))
        x = np.asarray(z['x_train'])
        if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3 or x.shape[0] == 0:
            raise ValueError('%s: x_train must be uint8 [n, H, W, 3] with n > 0, got %s %s' % (path, x.dtype, x.shape))
        y = None
        if 'y_train' in z.files:
            y = np.asarray(z['y_train']).reshape(-1)
            if len(y) != len(x):
                raise ValueError('%s: y_train has %d labels for the %d images of x_train' % (path, len(y), len(x)))
            y = y.astype(np.int64)
    return {'x_train': np.ascontiguousarray(x), 'y_train': y}


def index_plan(n, batch, rank, world, epoch, drop_last, seed=0):
    """The index arrays (int64) rank ``rank`` of ``world`` iterates in epoch ``epoch``: torch's DistributedSampler
    (shuffle, seed ``seed``, its own drop_last False) under a BatchSampler(batch, drop_last).  Pure host code."""
    n, batch, rank, world = int(n), int(batch), int(rank), int(world)
    if n <= 0 or batch <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError('index_plan: n %d, batch %d, rank %d of %d' % (n, batch, rank, world))
    g = torch.Generator()
    g.manual_seed(int(seed) + int(epoch))
    perm = torch.randperm(n, generator=g).numpy()
    per_rank = -(-n // world)
    total = per_rank * world
    if total > n:                                       # padded by the head of the permutation (repeated if need be)
        perm = np.concatenate([perm, np.resize(perm, total - n)])
    mine = perm[rank:total:world].astype(np.int64)
    stop = (per_rank // batch) * batch if drop_last else per_rank
    return [mine[i:i + batch].copy() for i in range(0, stop, batch)]


class DeviceLoader(object):
    """Endless iterator over ``(images, None)`` like the loops' other loaders: float NCHW batches of a device-resident
    uint8 set, in the order of ``index_plan``.  ``x``: uint8 [n, H, W, 3] as a numpy array or a tensor; it goes to
    ``device`` once, here.  Every rank holds the whole set and takes its sampler share."""

    def __init__(self, x, batch, rank=0, world=1, flip=False, drop_last=False, device=None):
        x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[0] == 0:
            raise ValueError('DeviceLoader: uint8 [n, H, W, 3] images expected, got %s %s' % (x.dtype, tuple(x.shape)))
        if x.shape[0] >= ops.GATHER_MAX_N:
            raise NotImplementedError('the indices are handed over as floats: fewer than 2^24 images (got %d)' % x.shape[0])
        if device is None:
            device = x.device if x.is_cuda else torch.device('cuda', torch.cuda.current_device())
        self.x = x.to(device).contiguous()
        self.n, self.h, self.w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        self.batch, self.rank, self.world = int(batch), int(rank), int(world)
        self.flip, self.drop_last = bool(flip), bool(drop_last)
        self.epoch, self._plan, self._pos = 0, None, 0
        if not index_plan(self.n, self.batch, self.rank, self.world, 0, self.drop_last):
            raise ValueError('DeviceLoader: %d images give rank %d of %d no full batch of %d (drop_last)' % (
                self.n, self.rank, self.world, self.batch))

    def __iter__(self):
        return self

    def __next__(self):
        if self._plan is None or self._pos >= len(self._plan):      # the epoch advances when its plan is exhausted
            if self._plan is not None:
                self.epoch += 1
            self._plan = index_plan(self.n, self.batch, self.rank, self.world, self.epoch, self.drop_last)
            self._pos = 0
        idx = self._plan[self._pos]
        self._pos += 1
        block = torch.zeros(len(idx), 2)
        block[:, 0] = torch.from_numpy(idx).float()
        if self.flip:                                               # the loader's only use of the torch CPU generator
            block[:, 1] = (torch.rand(len(idx)) < 0.5).float()
        return ops.gather_u8_nchw(self.x, upload(block, self.x.device), self.h, self.w), None


# datasets.py:10,57,99,115,131 of the reference: dataset -> (H, W, C).  The training scripts drive subsets of it.
IMAGE_SIZES = {'cifar10': (32, 32, 3), 'cifar100': (32, 32, 3), 'cifar10_hflip': (32, 32, 3),
               'cifar100_hflip': (32, 32, 3), 'celeba128': (128, 128, 3), 'afhq_cat': (512, 512, 3),
               'afhq_dog': (512, 512, 3), 'afhq_wild': (512, 512, 3)}
# what train_gan drives (and the cDDLS sampler, on its checkpoints); the others run through the StyleGAN2 scripts
TRAIN_GAN_IMAGE_SIZES = {k: IMAGE_SIZES[k] for k in ('cifar10', 'cifar100', 'cifar10_hflip')}


def dataset_flips(name):
    """The dataset names whose reference transform has RandomHorizontalFlip (datasets.py: ``*_hflip``, ``afhq_*``)."""
    return name.endswith('hflip') or name.startswith('afhq_')


def loader_for(path, dataset, image_size, batch, rank, world, drop_last, device):
    """The ``--data FILE.npz`` loader of a training loop: checks the images against the dataset's size, turns the flip on
    for the names the reference flips."""
    x = load_train_npz(path)['x_train']
    if tuple(x.shape[1:]) != tuple(image_size):
        raise ValueError("%s: x_train holds %s images, dataset '%s' is %s" % (path, tuple(x.shape[1:]), dataset,
                                                                            tuple(image_size)))
    return DeviceLoader(x, batch, rank, world, flip=dataset_flips(dataset), drop_last=drop_last, device=device)
