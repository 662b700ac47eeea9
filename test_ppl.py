#!/usr/bin/env python
"""Entry point of the perceptual path length (contrad_amd/latent.py; Karras et al. 2019, 2020): how far the image moves, in the
penultimate features of a frozen discriminator, per step of eps in the latent -- the one metric of the StyleGAN papers that
needs no real data.  The number is comparable only under one encoder file, never with LPIPS-based PPL.

    python test_ppl.py <run>/gen.pt sndcgan --encoder <enc>/dis.pt --n 10000 --seed 7
    python test_ppl.py <run>/gen_ema.pt stylegan2 --encoder <enc>/dis.pt --space w --sampling end
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.latent import ppl_main as main  # noqa: E402

if __name__ == '__main__':
    main()
