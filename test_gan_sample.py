#!/usr/bin/env python
"""Entry point with the reference's command line (test_gan_sample.py:24-34):

    python test_gan_sample.py logs/gan/c10_b512/sndcgan/<run>/gen.pt sndcgan --n_samples 10000 --batch_size 500
    python test_gan_sample.py <run>/gen_ema.pt stylegan2 --n_samples 64 --batch_size 32 --seed 1 --grid 64
"""
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from contrad_amd.sample import main
    main()
