"""GAN losses with augmented reals -- counterpart of training/gan/aug.py (``--mode=aug``): the discriminator sees
augment(reals) and the plain fakes; the generator step is that of ``std``.  The penalty is computed on the un-augmented
batch, as in the reference (aug.py:27-30)."""
import torch

from .std import D_LOSSES, d_loss_and_penalty, loss_G_fn  # noqa: F401  (loss_G_fn: aug.py:39-48 == std.py:39-48)


def loss_D_fn(P, D, options, images, gen_images):
    gen_images = gen_images.detach()
    all_images = torch.cat([P.augment_fn(images), gen_images], dim=0)
    return d_loss_and_penalty(P, D, options, images, gen_images, all_images, D(all_images), D_LOSSES)
