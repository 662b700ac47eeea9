"""Counterpart of training/gan/__init__.py:4-29: ``setup(P)`` resolves ``--mode`` to the loss functions."""
from importlib import import_module

BASELINE_MODES = ('std', 'aug', 'aug_both')       # single-rank only (train_gan.py / train_stylegan2.py refuse WORLD_SIZE > 1)


def setup(P):
    if P.mode == 'std':
        P.filename = f"{P.mode}_{P.penalty}"
        if 'cr' in P.penalty:
            P.filename += f'_{P.aug}'
    elif P.mode in ('aug', 'aug_both'):
        P.filename = f"{P.mode}_{P.aug}_{P.penalty}"
    elif P.mode == 'contrad':
        P.filename = f"{P.mode}_{P.aug}_L{P.lbd_a}_T{P.temp}"
    elif P.mode == 'simclr_only':
        P.filename = f"{P.mode}_{P.aug}_T{P.temp}"
    else:
        raise NotImplementedError("training mode '%s'" % P.mode)
    mod = import_module('.' + P.mode, __package__)
    P.train_fn = {"G": mod.loss_G_fn, "D": mod.loss_D_fn}
    return P
