#!/usr/bin/env python
"""Entry point of the latent walks (contrad_amd/latent.py): an interpolation sheet walk_<seed>.png (one row per pair of fixed
latents, columns at equal steps of t, one noise list) and, for StyleGAN2, a style-mixing sheet mix_<seed>.png (sources A down
the side, B along the top, one crossover layer), optionally truncated.

    python test_gan_walk.py <run>/gen.pt sndcgan --pairs 8 --steps 9 --seed 7
    python test_gan_walk.py <run>/gen_ema.pt stylegan2 --mix --cross 4 --truncation 0.7
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.latent import walk_main as main  # noqa: E402

if __name__ == '__main__':
    main()
