"""GAN losses with reals and fakes augmented -- counterpart of training/gan/aug_both.py (``--mode=aug_both``, the
DiffAugment baseline): D sees augment([reals | fakes]) in the D-step and augment(fakes), with the gradient flowing through
the augmentation into G, in the G-step."""
import torch

from .contrad import _GanGLoss
from .std import d_loss_and_penalty

D_LOSSES = ('nonsat', 'wgan', 'hinge')           # aug_both.py:15-22 (no lsgan)


def loss_D_fn(P, D, options, images, gen_images):
    assert images.size(0) == gen_images.size(0)
    gen_images = gen_images.detach()
    all_images = torch.cat([images, gen_images], dim=0)
    return d_loss_and_penalty(P, D, options, images, gen_images, all_images, D(P.augment_fn(all_images)), D_LOSSES)


def loss_G_fn(P, D, options, images, gen_images):
    """aug_both.py:36-43: 'nonsat' -> softplus(-d), anything else -> -d (means)."""
    kind = 'nonsat' if options['loss'] == 'nonsat' else 'wgan'
    return _GanGLoss.apply(D(P.augment_fn(gen_images)), kind)
