#!/usr/bin/env python
"""Entry point with the reference's command line (test_lineval.py:29-40):

    python test_lineval.py logs/gan/c10_b512/sndcgan/<run>/dis.pt sndcgan --n_classes 10 --batch_size 256 --data cifar10.npz
    python test_lineval.py <run>/dis.pt sndcgan --synthetic --graph --epochs 3
"""
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from contrad_amd.lineval import main
    main()
