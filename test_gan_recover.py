#!/usr/bin/env python
"""Entry point of latent recovery (contrad_amd/recover.py; an addition of this project):

    python test_gan_recover.py <run>/gen.pt sndcgan --data cifar10.npz --n 1000 --holdout --graph
    python test_gan_recover.py <run>/gen.pt sndcgan --synthetic --n 64 --steps 50 --lambda_feat 1 --dis <run>/dis.pt
"""
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from contrad_amd.recover import main
    main()
