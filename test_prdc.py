#!/usr/bin/env python
"""Entry point of the precision / recall / density / coverage evaluation of generated images in the features of a frozen
discriminator checkpoint (contrad_amd/prdc.py), with the shape of test_knn.py's command line:

    python test_prdc.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_prdc.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.prdc import main  # noqa: E402

if __name__ == '__main__':
    main()
