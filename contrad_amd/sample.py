"""Random sampling from a generator checkpoint: the reference's ``test_gan_sample.py`` on the MI355X path.  Same CLI
(``model_path architecture --n_samples --batch_size``), same loop (:89-99): ``G.eval()``, per batch
``G.sample_latent(batch_size)`` with the FULL batch size (on the last batch too) and ``G(z)`` under no_grad, image
``index = i * batch_size + j`` up to ``n_samples``; same output tree ``<logdir>/samples_<tag>_n<N>/<index>.png`` -- the
folder the reference's FID tooling reads -- plus one ``samples.npz`` (``images``: uint8 [N, H, W, 3], the input format of
common FID tools).  The dataset, hence the image size, comes from the ``*.gin`` next to the checkpoint.

Additions: ``--seed`` (the tag, and ``torch.manual_seed(tag)`` before the first draw; without it the tag is
``np.random.randint(10000)`` as in the reference) and ``--grid K`` (also writes ``grid.png`` of the first K samples).

The image side is one launch per batch (``ops.images_u8``, csrc/imagegrid.hip: quantisation and NCHW -> NHWC) and a D2H copy
of the uint8 batch, a quarter of the float one; the PNG deflate runs on a small host thread pool (zlib releases the GIL).
``--truncation PSI`` (StyleGAN2 only; with ``--truncation_n`` draws behind ``G.mean_latent`` and ``--truncation_cutoff L``)
samples at ``w_avg + PSI (w - w_avg)`` through ``latent.truncated`` and adds ``_psi<PSI>`` to the folder tag; w_avg is drawn
after the seed and before the first batch.  Without the flag nothing else is drawn and the output is what it was.

Any state dict the generator accepts works (gen.pt, gen_best.pt, gen_ema.pt) for all four names of ``get_architecture``.
"""
import math
import os
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import latent, ops
from .features import load_frozen
from .hostio import write_png

PNG_WORKERS = 8          # (fixed: a machine's CPU count says nothing about this process's share of it)


def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: Random sampling from G (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (generator) model checkpoint')
    parser.add_argument('architecture', type=str, help='Architecture')
    parser.add_argument('--n_samples', default=10000, type=int, help='Number of samples to generate (default: 10000)')
    parser.add_argument('--batch_size', default=500, type=int, help='Batch size (default: 500)')
    # additions
    parser.add_argument('--seed', default=None, type=int, help='RNG seed and directory tag (default: drawn)')
    parser.add_argument('--grid', default=0, type=int, metavar='K', help='also write grid.png of the first K samples')
    latent.add_truncation_arguments(parser)
    return parser.parse_args(argv)


def image_size_of(logdir):
    """Image size of the dataset named by the first ``*.gin`` in ``logdir`` (as cddls.load_networks reads it)."""
    from .lineval import _dataset_name
    from .data import IMAGE_SIZES
    dataset = _dataset_name(logdir)
    if dataset is None:
        raise RuntimeError('%s holds no *.gin file naming the dataset' % logdir)
    if dataset not in IMAGE_SIZES:
        raise NotImplementedError("sampling for dataset '%s' (implemented: %s)" % (dataset, sorted(IMAGE_SIZES)))
    return IMAGE_SIZES[dataset]


def load_generator(model_path, architecture, dev):
    from .models.gan import get_architecture
    return load_frozen(get_architecture(architecture, image_size_of(Path(model_path).parent))[0], model_path, dev)


def main(argv=None):
    P = parse_args(argv)
    if P.n_samples <= 0 or P.batch_size <= 0 or P.grid < 0:
        raise ValueError('--n_samples and --batch_size must be positive, --grid non-negative')
    latent.check_truncation_arguments(P)                           # (refused before the GPU is opened)
    if not torch.cuda.is_available():
        raise RuntimeError('sampling runs on the MI355X HIP path only (no CPU fallback)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    G = load_generator(P.model_path, P.architecture, dev)          # (the constructors draw: before the seed, as the reference)

    tag = int(np.random.randint(10000)) if P.seed is None else P.seed
    torch.manual_seed(tag)
    subdir = os.path.join(str(Path(P.model_path).parent), 'samples_%d_n%d' % (tag, P.n_samples))
    w_avg = None
    if P.truncation is not None:
        subdir += '_psi%g' % P.truncation
        w_avg = G.mean_latent(P.truncation_n)
    os.makedirs(subdir, exist_ok=True)
    print('Sampling in %s' % subdir, flush=True)

    n_batches = int(math.ceil(P.n_samples / P.batch_size))
    n_grid = min(P.grid, P.n_samples)
    kept, head, pending = [], [], []
    with ThreadPoolExecutor(max_workers=PNG_WORKERS) as pool:
        for i in range(n_batches):
            offset = i * P.batch_size
            keep = min(P.batch_size, P.n_samples - offset)
            with torch.no_grad():
                if w_avg is None:
                    samples = G(G.sample_latent(P.batch_size)).contiguous()
                else:
                    styles = latent.truncated(G, G.sample_latent(P.batch_size), P.truncation, w_avg, P.truncation_cutoff)
                    samples = G(styles, input_is_latent=True).contiguous()
                u8 = ops.images_u8(samples).cpu().numpy()[:keep]
                if sum(h.shape[0] for h in head) < n_grid:         # the float images of the grid stay on the device
                    head.append(samples[:n_grid - sum(h.shape[0] for h in head)].clone())
            for f in pending:                                      # the previous batch's files: written while G ran
                f.result()
            pending = [pool.submit(write_png, os.path.join(subdir, '%d.png' % (offset + j)), u8[j]) for j in range(keep)]
            kept.append(u8)
        for f in pending:
            f.result()
    np.savez(os.path.join(subdir, 'samples.npz'), images=np.concatenate(kept))
    if n_grid > 0:
        write_png(os.path.join(subdir, 'grid.png'), ops.image_grid_u8(torch.cat(head)).cpu().numpy())
    return subdir


if __name__ == '__main__':
    main()
