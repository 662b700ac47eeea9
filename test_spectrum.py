#!/usr/bin/env python
"""Entry point of the radial power spectrum of generated images against real ones (contrad_amd/spectrum.py): the azimuthally
averaged power of the luma, the standard check for up-sampling artefacts (Durall et al. 2020).  It reads uint8 images alone -- no
encoder checkpoint, no architecture unless it samples -- and reports the log-spectral distance, the level of the high band and
the three Nyquist points in dB, next to the noise floor of the real set.

    python test_spectrum.py --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz --figure
    python test_spectrum.py --real cifar10.npz --gen <run>/gen.pt --gen_arch sndcgan --n_fake 16384 --seed 7
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.spectrum import main  # noqa: E402

if __name__ == '__main__':
    main()
