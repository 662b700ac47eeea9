#!/usr/bin/env python
"""Entry point of the StyleGAN2 projector (contrad_amd/project.py; an addition of this project): real
images into W / W+ and the noise maps under a pixel-pyramid loss, and the train-against-held-out statistics of the errors.

    python test_gan_project.py <run>/gen_ema.pt stylegan2 --data afhq.npz --n 100 --holdout --noise fixed
    python test_gan_project.py <run>/gen_ema.pt stylegan2 --synthetic --n 8 --steps 200 --space wplus --level_weights 1 1 1
    python test_gan_walk.py <run>/gen_ema.pt stylegan2 --latents <run>/project_<seed>.npz --latent_rows 0 3 5
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrad_amd.project import main  # noqa: E402

if __name__ == '__main__':
    main()
