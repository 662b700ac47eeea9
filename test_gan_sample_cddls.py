#!/usr/bin/env python
"""Entry point with the reference's command line (test_gan_sample_cddls.py:27-48):

    python test_gan_sample_cddls.py logs/gan/c10_b512/sndcgan/<run> <run>/lin_eval_<seed>.pth.tar sndcgan --lbd 1.0
    python test_gan_sample_cddls.py <run> <run>/lin_eval_<seed>.pth.tar sndcgan --graph --log_energy --seed 1
"""
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from contrad_amd.cddls import main
    main()
