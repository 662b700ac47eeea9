"""Training loop of the reference's ``train_gan.py`` on the MI355X path: same CLI
(``<gin_config> <architecture> --mode=contrad --aug=simclr [--use_warmup --temp --lbd_a --resume ...]``), same step
ordering (train_gan.py:141-179: warm-up, set_grad toggling, D-step, G-step), same checkpoint files
(gen.pt / dis.pt / optim.pt, :211-225), one process per GPU.

Differences by design: data parallelism is ``contrad_amd.engine`` (packed RCCL embedding all-gather inside the loss,
flat gradient all-reduce folded into the fused Adam) instead of DistributedDataParallel; the per-step ``dist.barrier()``
of the reference (:227) is dropped (the all-reduce already synchronises); FID / GIF / tensorboard side paths are out
of scope -- losses are logged to stdout / log.txt; ``--monitor`` writes the reference's fixed-latent
and augmented-real image grids as PNG / animated PNG (contrad_amd/evaluate/gan.py; off by default).  ``--knn_data FILE.npz`` logs the weighted
kNN accuracy of D's features at every evaluation (contrad_amd/knn.py; an addition, off by default); ``--prdc_data FILE.npz --prdc_encoder FILE.pt`` logs
precision / recall / density / coverage of the generator in a frozen encoder's features (contrad_amd/prdc.py; an addition, off by default).  With it ``--prdc_kid`` adds the kernel distance (KID)
of the same features to ``kid_<seed>.csv`` (contrad_amd/kid.py; ``--prdc_best kid`` keeps the checkpoints of its minimum).  Datasets: ``--data FILE.npz`` keeps the uint8
training set on the device and gathers every batch there (contrad_amd/data.py: the reference's sampler order, ToTensor's
pixels, no torchvision); ``--synthetic`` (default when neither it nor torchvision is there) feeds uniform-random
CIFAR-shaped batches; otherwise torchvision CIFAR-10/100 as the reference.

This module holds what the script does differently from the StyleGAN2 ones (its flags, option defaults, warm-up, loaders,
log directory and ``train_step``, which calls the eager steps of engine.py); everything else of ``main()`` is
contrad_amd/train_driver.py.
"""
import functools
import os

import torch

from . import config, engine, train_driver
from .data import TRAIN_GAN_IMAGE_SIZES as IMAGE_SIZES
from .engine import GraphedDStep, GraphedGStep, sample_generator, set_grad
from .hostio import THROTTLE


def parse_args(argv=None):
    accepted = 'accepted for CLI compatibility'
    parser = train_driver.make_parser('Training script: ContraD on MI355X (one process per GPU).', [
        'gin_config', 'architecture', '--mode',
        ('--penalty', dict(help='none | cr | bcr | gp (std / aug / aug_both)')),
        '--aug', '--use_warmup', '--temp', '--lbd_a',
        ('--no_fid', dict(help=accepted + ' (FIDs are never tracked here)')),
        '--no_gif',
        ('--n_eval_avg', dict(help=accepted)),
        '--print_every', '--evaluate_every', '--save_every', '--comment', '--resume', '--finetune',
        ('--workers', dict(default=0)),
        # train_gan.py:79-82 (NODE count / node rank of the reference's mp.spawn launch): accepted; this build is one
        # process per GPU of ONE node and takes rank / world size from the launcher's environment (RANK / WORLD_SIZE)
        ('--world-size', dict(default=1, type=int, help=accepted + ' (nodes; single-node build)')),
        ('--rank', dict(default=0, type=int, help=accepted + ' (node rank)')),
        ('--port', dict(default=40404)),
        '--synthetic', '--data', '--max_steps', '--logdir', '--seed',
        ('--graph', dict(help='replay the D- and G-step from captured hipGraphs (simclr pipeline; with several ranks the '
                              'RCCL collectives are captured too)')),
        ('--monitor', dict(help=train_driver.monitor_help('fixed latents')))])
    return parser.parse_args(argv)


def _update_warmup(optimizer, cur_step, warmup, lr):
    """train_gan.py:88-93."""
    if warmup > 0:
        ratio = min(1., (cur_step + 1) / warmup)
        for group in optimizer.param_groups:
            group['lr'] = ratio * lr


@config.configurable('options')
def get_options_dict(dataset=config.REQUIRED, loss=config.REQUIRED, batch_size=64, fid_size=10000, max_steps=200000,
                     warmup=0, n_critic=1, lr=2e-4, lr_d=None, beta=(.5, .999), lbd=10., lbd2=10.):
    """train_gan.py:103-121."""
    if lr_d is None:
        lr_d = lr
    return {"dataset": dataset, "batch_size": batch_size, "fid_size": fid_size, "loss": loss, "max_steps": max_steps,
            "warmup": warmup, "n_critic": n_critic, "lr": lr, "lr_d": lr_d, "beta": beta, "lbd": lbd, "lbd2": lbd2}


def _synthetic_loader(batch, image_size, device, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    h, w, c = image_size
    while True:
        yield torch.rand(batch, c, h, w, generator=g).to(device, non_blocking=True), None


def _dataset_loader(name, batch, rank, world, workers):
    import torchvision
    import torchvision.transforms as T
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    root = os.environ.get('DATA_DIR', './data')
    cls = torchvision.datasets.CIFAR100 if name == 'cifar100' else torchvision.datasets.CIFAR10
    tf = [T.RandomHorizontalFlip()] if name.endswith('hflip') else []
    ds = cls(root, train=True, download=False, transform=T.Compose(tf + [T.ToTensor()]))
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank)
    loader = DataLoader(ds, shuffle=False, pin_memory=True, num_workers=workers, batch_size=batch, sampler=sampler)
    epoch = 0
    while True:
        for images, targets in loader:
            yield images.cuda(non_blocking=True), targets
        epoch += 1
        sampler.set_epoch(epoch)


NOT_CONTRAD = "--graph captures the ContraD critic iteration (--mode contrad), not '%s'"


class GraphedCritic(engine.GraphedCritic):
    """``--graph``: the critic iteration of ``train_step`` replayed from ONE captured hipGraph (engine.GraphedDStep) and
    the generator step from a second one (engine.GraphedGStep)."""

    def __init__(self):
        super().__init__(functools.partial(GraphedDStep, warmup=0), GraphedGStep, NOT_CONTRAD)


def train_step(P, opt, G, D, opt_G, opt_D, loader, step, reducers, graphed=None):
    """One iteration of train_gan.py:141-179.  ``loader`` yields (images, labels); a fresh real batch is drawn for
    every critic iteration (train_gan.py:153-155) and the last one feeds the G-step.  Returns the loss tensors (no
    host sync)."""
    THROTTLE.begin()                          # host stays at most one step ahead of the GPU (hostio.py)
    G.train(); D.train()
    if P.use_warmup:
        _update_warmup(opt_G, step, opt["warmup"], opt["lr"])
        _update_warmup(opt_D, step, opt["warmup"], opt["lr_d"])
    red_G, red_D = reducers
    set_grad(G, False); set_grad(D, True)
    for _ in range(opt['n_critic']):
        images, _labels = next(loader)
        done = graphed(P, opt, G, D, opt_D, images) if graphed is not None else None
        d_loss, aux = done if done is not None else engine.d_step(P, G, D, opt_D, opt, images, red_D)
    set_grad(G, True); set_grad(D, False)
    g_loss = graphed.generator(P, opt, G, D, opt_G, images) if graphed is not None else None
    if g_loss is None:
        g_loss = P.train_fn["G"](P, D, opt, images, sample_generator(G, images.size(0)))
        engine.optimizer_step(opt_G, g_loss, G, red_G)
    THROTTLE.end()
    # detached: a loss that keeps last iteration's autograd graph (and its AccumulateGrad nodes) alive would tie the next
    # D-step to the stream that graph ran on -- which breaks a hipGraph capture
    return {'G_loss': g_loss.detach(), 'D_loss': d_loss.detach(), 'D_penalty': aux['penalty'].detach(),
            'D_real': aux['d_real'].detach(), 'D_gen': aux['d_gen'].detach()}


def _logdir(P):
    return f'logs/gan/{P.gin_stem}/{P.architecture}/{P.filename}{P.comment}'


SCRIPT = train_driver.Script(
    get_options=get_options_dict, image_sizes=IMAGE_SIZES, logdir=_logdir, synthetic_loader=_synthetic_loader,
    dataset_loader=_dataset_loader, make_critic=GraphedCritic, not_contrad=NOT_CONTRAD, data_keeps_partial_batch=True,
    dataset_hint=" (train_gan.py drives %s; the StyleGAN2 high-resolution configs run through "
                 "train_stylegan2_contraD.py)" % sorted(IMAGE_SIZES))


def main(argv=None):
    run = train_driver.build_run(parse_args(argv), SCRIPT)
    return train_driver.run_loop(run, lambda step: train_step(run.P, run.options, run.G, run.D, run.opt_G, run.opt_D,
                                                              run.loader, step, run.reducers, run.graphed))


if __name__ == '__main__':
    main()
