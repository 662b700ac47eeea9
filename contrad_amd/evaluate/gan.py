"""Counterpart of the reference's ``evaluate/gan.py`` (:15-82): ``ImageGrid`` and ``FixedSampleGeneration`` with the
reference's interface (``update`` / ``value`` / ``summary`` / ``reset``, the ``volatile`` flag), and the ``Monitor`` that
drives them from the three training loops behind ``--monitor`` (train_gan.py:192-209 of the reference).

A grid is a uint8 (rows, columns, 3) numpy array -- the file's pixels, not the reference's float canvas -- made on the device
by ``ops.image_grid_u8`` (csrc/imagegrid.hip: make_grid and save_image's quantisation in one launch; the D2H copy is the
uint8 canvas).  FID (``FIDScore``) stays out of scope: DESIGN.md section 8.

Monitoring never moves the training trajectory (tests/test_monitor_gpu.py: bitwise-equal checkpoints with and without it):
  * the monitor samples from a generator module of its OWN that loads the training generator's state dict at each
    evaluation, stays in eval mode and never requires grad -- the training modules' modes, packed-weight caches and
    captured graphs are not touched;
  * the fixed latents come from a ``torch.Generator`` seeded with ``eval_seed``, and ``eval_seed`` from
    ``np.random.RandomState(P.seed)``: the global streams are not read;
  * everything else that draws (building the module, StyleGAN2's per-layer noise, the augmentation preview) runs inside
    ``preserved_rng``: torch CPU, torch CUDA and numpy states saved before, restored after;
  * the real batch of the preview is the one the step drew (``LastBatch``), cloned at evaluation time only.
"""
import contextlib
import os

import numpy as np
import torch

from .. import ops
from ..hostio import apng_bytes, write_png

N_FIXED = 16          # evaluate/gan.py:51,58 of the reference: 16 latents, nrow = 4
N_GRID = 64           # evaluate/gan.py:22: images[:64], make_grid's default nrow = 8


def _grid(images, nrow):
    return ops.image_grid_u8(images.detach().contiguous().float(), nrow=nrow).cpu().numpy()


@contextlib.contextmanager
def preserved_rng(device=None):
    """Run the body without a trace in the global random streams: the torch CPU state, the CUDA state of ``device`` (when
    it is a CUDA device) and numpy's global state are saved before and restored after."""
    cpu, npy = torch.get_rng_state(), np.random.get_state()
    cuda = torch.cuda.get_rng_state(device) if device is not None and torch.device(device).type == 'cuda' else None
    try:
        yield
    finally:
        torch.set_rng_state(cpu)
        np.random.set_state(npy)
        if cuda is not None:
            torch.cuda.set_rng_state(cuda, device)


def fixed_latent(G, n, seed, generator=None):
    """``n`` latents of ``G``'s prior (G.sample_latent's distribution) from a torch.Generator of their own, on G's device.
    ``generator``: the caller's CPU generator, already seeded, to go on drawing from behind the latents."""
    g = torch.Generator(device='cpu').manual_seed(int(seed)) if generator is None else generator
    dev = next(G.parameters()).device
    if hasattr(G, 'style_dim'):                                    # StyleGAN2: N(0, 1)
        return torch.randn(n, G.style_dim, generator=g).to(dev)
    if hasattr(G, 'nz'):                                           # SNDCGAN: U(-1, 1)
        return torch.empty(n, G.nz).uniform_(-1, 1, generator=g).to(dev)
    raise NotImplementedError('fixed latents for %s' % type(G).__name__)


class _GridHistory(object):
    def __init__(self, volatile=False):
        self._images = []
        self._steps = []
        self.volatile = volatile

    def _push(self, step, img_grid):
        self._images.append(img_grid)
        self._steps.append(step)
        if self.volatile:
            self._images = self._images[-1:]
            self._steps = self._steps[-1:]
        return img_grid

    @property
    def value(self):
        if len(self._images) > 0:
            return self._images[-1]
        raise ValueError()

    def summary(self):
        return self._images


class ImageGrid(_GridHistory):
    """Grid of the first 64 images of a batch, 8 per row."""

    def update(self, step, images):
        return self._push(step, _grid(images[:N_GRID], 8))

    def reset(self):
        self._images = []
        self._steps = []


class FixedSampleGeneration(_GridHistory):
    """Grid (4 per row) of ``G`` at 16 fixed latents.  ``seed``: the latents come from a generator of their own (the
    monitor's way); without it they are ``G.sample_latent(16)`` from the global stream, as in the reference."""

    def __init__(self, G, volatile=False, seed=None):
        super().__init__(volatile)
        self._G = G
        self._seed = seed
        self._latent = G.sample_latent(N_FIXED) if seed is None else fixed_latent(G, N_FIXED, seed)

    def update(self, step):
        with torch.no_grad():
            return self._push(step, _grid(self._G(self._latent), 4))

    def reset(self):
        # evaluate/gan.py:80 of the reference draws 64 latents here (update() then still lays them out 4 per row)
        self._latent = self._G.sample_latent(N_GRID) if self._seed is None else fixed_latent(self._G, N_GRID, self._seed)
        self._images = []
        self._steps = []


class LastBatch(object):
    """Pass-through iterator around a loader that remembers the last item it handed out (``.last``, None before the
    first): the monitor previews the batch the step already drew instead of drawing one more."""

    def __init__(self, loader):
        self._it = iter(loader)
        self.last = None

    def __iter__(self):
        return self

    def __next__(self):
        self.last = next(self._it)
        return self.last


def eval_seed_of(seed):
    """The tag of a run's monitoring files (the reference's ``P.eval_seed``, train_gan.py:283), drawn from a stream of its
    own so that the global numpy stream is not read."""
    return int(np.random.RandomState(int(seed)).randint(10000))


def freeze(module):
    """``module`` in eval mode with gradients off on every parameter."""
    module.eval()
    for p in module.parameters():
        p.requires_grad_(False)
    return module


def own_network(which, architecture, image_size, device, P=None):
    """A network of a monitor's own: the ``'G'`` or ``'D'`` of ``get_architecture``, built inside ``preserved_rng`` (the
    constructors draw the initial weights), on ``device``, frozen.  The monitor loads the shown weights into it at each
    evaluation, so the training modules' modes, packed-weight caches and captured graphs are not touched."""
    from ..models.gan import get_architecture
    with preserved_rng(device):
        net = get_architecture(architecture, image_size, P=P)['GD'.index(which)]
    return freeze(net.to(device))


def load_x_train(path, image_size, who):
    """``x_train`` of the npz at ``path`` (``features.load_images``), refused unless its images have the run's
    ``image_size``.  ``who``: 'generator makes' or 'discriminator takes'."""
    from .. import features
    x = features.load_images(path, 'x_train')
    if tuple(x.shape[1:]) != tuple(image_size):
        raise ValueError('%s: x_train holds %s images, the %s %s' % (path, tuple(x.shape[1:]), who, tuple(image_size)))
    return x


def frozen_encoder(architecture, image_size, path, device):
    """A monitor's yardstick: the discriminator of ``architecture`` (built inside ``preserved_rng``: the constructors draw
    the initial weights) with the checkpoint at ``path``, loaded once and frozen."""
    from .. import features
    from ..models.gan import get_architecture
    with preserved_rng(device):
        E = get_architecture(architecture, image_size)[1]
    return features.load_frozen(E, path, device)


class WeightsMonitor(object):
    """"Evaluate these weights, append a row": what every monitor of the training scripts is.  It owns the eval seed, a
    frozen ``network`` of its own (``own_network``; also reachable as ``.G`` / ``.D`` when ``which`` says so) and its csv
    ``files``: ``(name with %d for the eval seed, header, line_of(step, out))`` each, kept as ``(path, header, line_of)``;
    a header is written only where the file does not exist yet, so a resumed run appends.  A subclass checks its arguments
    and computes its fixed state BEFORE it calls this constructor (a refusal leaves no file behind) and gives ``evaluate()``.

    ``update`` is the one place that upholds "monitoring never moves the training trajectory" (module docstring): the shown
    module is only read (its mode, packed-weight caches and captured graphs are not touched) and the global random streams
    come back as they were, whatever ``evaluate()`` draws or raises."""

    def __init__(self, logdir, device, seed, network, files=(), which=None):
        self.logdir, self.device, self.eval_seed = logdir, device, eval_seed_of(seed)
        self.net = freeze(network)
        if which is not None:
            setattr(self, which, self.net)
        self.files = [(os.path.join(logdir, name % self.eval_seed), head, line_of) for name, head, line_of in files]
        for path, head, _ in self.files:
            if not os.path.exists(path):
                with open(path, 'w') as f:
                    f.write(head + '\n')

    @contextlib.contextmanager
    def showing(self, shown):
        """The body sees ``shown``'s weights in the owned network, in eval mode, under ``no_grad`` and ``preserved_rng``."""
        with torch.no_grad(), preserved_rng(self.device):
            self.net.load_state_dict(shown.state_dict())
            self.net.eval()
            yield

    def evaluate(self):
        raise NotImplementedError

    def update(self, step, shown):
        """One evaluation of ``shown``'s weights -> ``evaluate()``'s result, one line appended per file (``self.lines``;
        none if ``evaluate()`` or a ``line_of`` raises)."""
        with self.showing(shown):
            out = self.evaluate()
        self.lines = [line_of(step, out) for _, _, line_of in self.files]
        for (path, _, _), line in zip(self.files, self.lines):
            with open(path, 'a') as f:
                f.write(line + '\n')
        return out


class Monitor(WeightsMonitor):
    """``--monitor`` on rank 0: image grids, no csv.  ``architecture`` / ``image_size`` / ``P``: what ``get_architecture``
    built the training generator from; ``device``: where it lives.  ``last_batch``: () -> the (images, labels) of the step
    just finished (``LastBatch.last``), for an ``update`` that is not handed one."""

    def __init__(self, logdir, architecture, image_size, device, seed, no_gif=False, P=None, delay_ms=500, last_batch=None):
        super().__init__(logdir, device, seed, own_network('G', architecture, image_size, device, P), which='G')
        self.no_gif, self.delay_ms, self.P, self.last_batch = bool(no_gif), delay_ms, P, last_batch
        self.fixed_gen = FixedSampleGeneration(self.G, volatile=self.no_gif, seed=self.eval_seed)
        self.image_grid = ImageGrid(volatile=self.no_gif)
        self._deflated = []                                        # apng_bytes: compressed frames so far

    def _path(self, name):
        return os.path.join(self.logdir, name)

    def update(self, step, generator, batch=None, augment_fn=None):
        """One evaluation: ``generator``: the module whose weights are shown (G, or g_ema in the StyleGAN2 loops);
        ``batch``: the (images, labels) of the step just finished (default: ``last_batch()``); ``augment_fn``: the run's
        (default: ``P.augment_fn``)."""
        if batch is None and self.last_batch is not None:
            batch = self.last_batch()
        with self.showing(generator):
            torch.cuda.manual_seed(self.eval_seed)                 # StyleGAN2's per-layer noise: the same at every evaluation
            grid = self.fixed_gen.update(step)
            if self.no_gif:
                write_png(self._path('fixed_gen_%d.png' % self.eval_seed), grid)
            else:
                sub = self._path('progress_%d' % self.eval_seed)
                os.makedirs(sub, exist_ok=True)
                write_png(os.path.join(sub, 'step_%d.png' % step), grid)
                with open(self._path('training_progress_%d.png' % self.eval_seed), 'wb') as f:
                    f.write(apng_bytes(self.fixed_gen.summary(), self.delay_ms, deflated=self._deflated))
            if batch is not None:
                images = batch[0].clone()
                aug_grid = self.image_grid.update(step, (augment_fn or self.P.augment_fn)(images))
                write_png(self._path('real_augment_%d.png' % self.eval_seed), aug_grid)
