#!/usr/bin/env python
"""Entry point of the Frechet distance (column means and np.cov covariances; the trace term by a fixed number of Newton-Schulz
steps on the conv engine) of generated images from real ones in the L2-normalised features of a frozen discriminator
checkpoint (contrad_amd/fd.py), with the shape of test_prdc.py's command line.  The numbers are comparable only between
evaluations under one encoder file, never with the Inception-based FID of papers.

    python test_fd.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_fd.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7 [--n_iter 60]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.fd import main  # noqa: E402

if __name__ == '__main__':
    main()
