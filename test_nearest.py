#!/usr/bin/env python
"""Entry point of the memorisation check (contrad_amd/nearest.py): the authenticity of generated images (the share that is
NOT closer to its nearest training image than that image is to its own nearest other training image) in the L2-normalised
features of a frozen discriminator checkpoint, and a figure of the fakes closest to a training image next to their nearest
training images, with the shape of test_prdc.py's command line.  Comparable only between evaluations under one encoder
file; read the number against ``--holdout`` (held-out real images in place of the fakes), not against 1.

    python test_nearest.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz --holdout
    python test_nearest.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7 --k 8 --rows 16
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.nearest import main  # noqa: E402

if __name__ == '__main__':
    main()
