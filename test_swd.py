#!/usr/bin/env python
"""Entry point of the sliced Wasserstein distance (SWD, Karras et al. 2018) of generated images from real ones on
Laplacian-pyramid patches (contrad_amd/swd.py).  It reads uint8 images alone -- no encoder checkpoint, no architecture unless
it samples -- and reports one value per resolution level (x 1e3) and their average: the one number of this project that is
comparable across encoders, architectures and repositories that share the definition.

    python test_swd.py --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_swd.py --real cifar10.npz --gen <run>/gen.pt --gen_arch sndcgan --n 16384 --seed 7
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.swd import main  # noqa: E402

if __name__ == '__main__':
    main()
