#!/usr/bin/env python
"""Entry point of the label-free contrastive diagnostics of a discriminator checkpoint (contrad_amd/contrast.py): NT-Xent,
the rank of the positive, alignment and uniformity on two held-out views, with the shape of test_knn.py's command line:

    python test_contrast.py logs/gan/c10_b512/sndcgan/<run>/dis.pt sndcgan --data celeba.npz --aug simclr --temp 0.1
    python test_contrast.py <run>/dis.pt sndcgan --synthetic --n 2000 --batch_size 512 --t 2
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.contrast import main  # noqa: E402

if __name__ == '__main__':
    main()
