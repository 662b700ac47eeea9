#!/usr/bin/env python
"""Entry point of the weighted kNN evaluation of a discriminator checkpoint (contrad_amd/knn.py), with the shape of
test_lineval.py's command line:

    python test_knn.py logs/gan/c10_b512/sndcgan/<run>/dis.pt sndcgan --n_classes 10 --data cifar10.npz
    python test_knn.py <run>/dis.pt sndcgan --synthetic --k 200 --temp 0.1
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.knn import main  # noqa: E402

if __name__ == '__main__':
    main()
