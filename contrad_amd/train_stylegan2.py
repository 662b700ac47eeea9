"""Training loops of the reference's ``train_stylegan2.py`` and ``train_stylegan2_contraD.py`` on the MI355X path.

Same CLI (``<gin_config> <architecture> --mode=contrad --aug=simclr[_hq] --lbd_r1 .. [--no_lazy --d_reg_every
--style_mix --halflife_k --ema_start_k --halflife_lr --use_warmup --resume --finetune ...]``), same step ordering
(train_stylegan2.py:147-233 / train_stylegan2_contraD.py:182-246): LR warm-up / decay -> EMA ``accumulate`` -> G-step
FIRST -> D-step with the lazy R1 penalty ``(0.5*lbd_r1) * r1 * d_reg_every`` every ``d_reg_every`` steps (``--no_lazy``
=> every step) -> extra critic iterations; same checkpoint files (gen.pt / dis.pt / gen_ema.pt / optim.pt).

The two scripts differ exactly where the reference's do:
  * ``train_stylegan2``        : the D-step re-uses the G-step's fake batch (detached) and makes ONE 3N-image D call
                                 through ``P.train_fn["D"]`` (train_stylegan2.py:184-212);
  * ``train_stylegan2_contraD``: fresh fakes under no_grad, fakes (N) and the two real views (2N) in SEPARATE D calls
                                 (G_D.forward, train_stylegan2_contraD.py:117-164).
The reference parallelises the second one with ``nn.DataParallel(G_D)`` (parameters re-broadcast on every forward, outputs
gathered on GPU 0).  Here both are one process per GPU: per-rank batch = batch_size / world, the embeddings travel in
ONE packed RCCL all-gather inside the loss, parameter gradients in flat all-reduces folded into the fused Adam -- the
global loss of the DataParallel formulation, without the per-step parameter broadcast.
FID / GIF / tensorboard side paths are out of scope; ``--monitor`` writes the reference's image
grids from ``g_ema`` as PNG / animated PNG (contrad_amd/evaluate/gan.py; off by default).  ``--knn_data FILE.npz`` logs the weighted kNN accuracy
of D's features at every evaluation (contrad_amd/knn.py; an addition, off by default); ``--prdc_data FILE.npz --prdc_encoder FILE.pt`` logs
precision / recall / density / coverage of the generator in a frozen encoder's features (contrad_amd/prdc.py; an addition, off by default).  With it ``--prdc_kid`` adds the kernel distance (KID)
of the same features to ``kid_<seed>.csv`` (contrad_amd/kid.py; ``--prdc_best kid`` keeps the checkpoints of its minimum).

This module holds what the two scripts do differently from train_gan (their flags, option defaults, schedules, EMA,
loaders, log directory and ``train_iteration``, whose D-steps are engine.d_step_stylegan2 / d_step_stylegan2_contrad);
everything else of ``main()`` is contrad_amd/train_driver.py.
"""
import functools
import os

import torch

from . import config, engine, ops, train_driver
from .data import IMAGE_SIZES                   # every dataset of the table
from .engine import GraphedSG2DStep, GraphedSG2GStep, _sg2_fakes, set_grad
from .hostio import THROTTLE
from .training.gan.contrad import _GanGLoss


def parse_args(argv=None, contrad_script=False):
    parser = train_driver.make_parser(
        'Training script: StyleGAN2%s on MI355X (one process per GPU).' % (' + ContraD' if contrad_script else ''), [
            'gin_config', 'architecture', '--mode',
            ('--penalty', dict(help='none | cr | bcr (std / aug / aug_both)')),
            '--aug', '--use_warmup',
            ('--workers', dict(default=8)),
            '--temp', '--lbd_a',
            # StyleGAN2 options (train_stylegan2.py:61-75)
            ('--no_lazy', dict(action='store_true', help='Do not use lazy regularization')),
            ('--d_reg_every', dict(type=int, default=16)),
            ('--lbd_r1', dict(type=float, default=10)),
            ('--style_mix', dict(default=0.9, type=float)),
            ('--halflife_k', dict(default=20, type=int)),
            ('--ema_start_k', dict(default=None, type=int)),
            ('--halflife_lr', dict(default=0, type=int)),
            '--no_fid', '--no_gif', '--n_eval_avg', '--print_every', '--evaluate_every', '--save_every', '--comment',
            '--resume', '--finetune',
            ('--port', dict(default=40405)),
            '--synthetic', '--data', '--max_steps',
            ('--batch_size', dict(default=None, type=int, help='override options.batch_size (global)')),
            '--logdir', '--seed',
            ('--graph', dict(help='replay the D- and G-step from captured hipGraphs (collectives included; the ContraD '
                                  'script, whose D-step draws its own fakes)')),
            ('--monitor', dict(help=train_driver.monitor_help('g_ema at fixed latents')))])
    return parser.parse_args(argv)


def _update_warmup(optimizer, cur_step, warmup, lr):
    """train_stylegan2.py:86-91."""
    if warmup > 0:
        ratio = min(1., (cur_step + 1) / (warmup + 1e-8))
        for group in optimizer.param_groups:
            group['lr'] = ratio * lr


def _update_lr(optimizer, cur_step, batch_size, halflife_lr, lr, mult=1.0):
    """train_stylegan2.py:94-103."""
    if halflife_lr > 0 and (cur_step > 0) and (cur_step % 1000 == 0):
        ratio = (cur_step * batch_size) / halflife_lr
        lr_w = (0.5 ** ratio) * lr * mult
        for group in optimizer.param_groups:
            group['lr'] = lr_w
        return lr_w
    return None


@config.configurable('options')
def get_options_dict(dataset=config.REQUIRED, loss=config.REQUIRED, batch_size=32, fid_size=10000, max_steps=800000,
                     warmup=0, n_critic=1, lr=0.002, lr_d=None, beta=(.0, .99), lbd=10., lbd2=10.):
    """train_stylegan2.py:126-144."""
    if lr_d is None:
        lr_d = lr
    return {"dataset": dataset, "batch_size": batch_size, "fid_size": fid_size, "loss": loss, "max_steps": max_steps,
            "warmup": warmup, "n_critic": n_critic, "lr": lr, "lr_d": lr_d, "beta": beta, "lbd": lbd, "lbd2": lbd2}


@torch.no_grad()
def accumulate(model_dst, model_src, decay=0.999):
    """utils.accumulate (utils.py:130-143): dst = decay * dst + (1 - decay) * src for the parameters (one fused axpby
    launch per tensor), buffers copied."""
    params_dst = dict(model_dst.named_parameters())
    params_src = dict(model_src.named_parameters())
    for k, p in params_dst.items():
        ops.axpby_(p.data, params_src[k].data, decay, 1.0 - decay)
        torch.autograd.graph.increment_version(p)
    buf_src = dict(model_src.named_buffers())
    for k, b in model_dst.named_buffers():
        b.copy_(buf_src[k])


def sample_generator(G, num_samples, style_mix=0.9, enable_grad=True):
    """_sample_generator (train_stylegan2.py:116-123)."""
    with torch.set_grad_enabled(enable_grad):
        return _sg2_fakes(G, num_samples, style_mix)     # z, mixing latent and per-layer noise in one device draw


def loss_G_nonsat(d_gen):
    """_loss_G_fn (train_stylegan2_contraD.py:112-114)."""
    return _GanGLoss.apply(d_gen, 'nonsat')


# train_stylegan2_contraD.py calls G_D.forward WITHOUT its style_mix argument (:207,218 -> the default 0.9 of :128): the
# ``--style_mix`` flag only names the log directory there (:349).  Reproduced as is.
CONTRAD_SCRIPT_STYLE_MIX = 0.9

NOT_CONTRAD = "--graph captures the ContraD D-step (--mode contrad), not '%s'"


class GraphedCritic(engine.GraphedCritic):
    """``--graph`` for train_stylegan2_contraD.py: its D-step (fresh fakes, two D calls, lazy R1) is exactly
    engine.d_step_stylegan2_contrad, so it is replayed from engine.GraphedSG2DStep (the lazy-R1 steps run eagerly inside
    it), and its generator step from engine.GraphedSG2GStep."""

    def __init__(self):
        super().__init__(functools.partial(GraphedSG2DStep, contrad_script=True, style_mix=CONTRAD_SCRIPT_STYLE_MIX, warmup=0),
                         functools.partial(GraphedSG2GStep, style_mix=CONTRAD_SCRIPT_STYLE_MIX), NOT_CONTRAD)


def train_iteration(P, opt, G, D, g_ema, opt_G, opt_D, loader, step, reducers, contrad_script, graphed=None):
    """One iteration of train_stylegan2.py:147-233 (contrad_script False) / train_stylegan2_contraD.py:182-246 (True).
    Returns the loss tensors (no host sync)."""
    THROTTLE.begin()
    red_G, red_D = reducers
    style_mix = CONTRAD_SCRIPT_STYLE_MIX if contrad_script else P.style_mix
    d_step = engine.d_step_stylegan2_contrad if contrad_script else engine.d_step_stylegan2
    if P.use_warmup:
        _update_warmup(opt_G, step, opt["warmup"], opt["lr"])
        _update_warmup(opt_D, step, opt["warmup"], opt["lr_d"])
    lr_note = None
    if (not P.use_warmup) or step > opt["warmup"]:
        cur_lr_g = _update_lr(opt_G, step, opt["global_batch_size"], P.halflife_lr, opt["lr"])
        cur_lr_d = _update_lr(opt_D, step, opt["global_batch_size"], P.halflife_lr, opt["lr_d"])
        if cur_lr_d and cur_lr_g:
            lr_note = (cur_lr_g, cur_lr_d)
    do_ema = (step * opt['global_batch_size']) > (P.ema_start_k * 1000)
    accumulate(g_ema, G, P.accum if do_ema else 0)

    G.train(); D.train()
    images, _labels = next(loader)
    N = images.size(0)
    out = {}

    # ---- generator step first ----
    set_grad(G, True); set_grad(D, False)
    g_loss = graphed.generator(P, opt, G, D, opt_G, images) if graphed is not None else None
    if g_loss is None:
        gen_images = sample_generator(G, N, style_mix=style_mix, enable_grad=True)
        if contrad_script:      # G_D.forward(train_G=True): D(augment(G(z)), sg_linear=False, ...) -> d_gen
            d_gen, _aux = D(P.augment_fn(gen_images), sg_linear=False, projection=True, projection2=True)
            g_loss = loss_G_nonsat(d_gen)
        else:
            g_loss = P.train_fn["G"](P, D, opt, images, gen_images)
        engine.optimizer_step(opt_G, g_loss, G, red_G)
    out['G_loss'] = g_loss.detach()

    # ---- discriminator step: train_stylegan2 feeds it the generator step's fakes, the ContraD script draws fresh ones ----
    set_grad(G, False); set_grad(D, True)
    done = graphed(P, opt, G, D, opt_D, images, step) if graphed is not None else None
    d_loss, aux = done if done is not None else d_step(P, G, D, opt_D, opt, images, step, red_D, style_mix,
                                                       fakes=None if contrad_script else gen_images.detach())
    if 'r1' in aux:
        out['D_r1'] = aux['r1'].detach()
    for _ in range(opt['n_critic'] - 1):        # the extra critic iterations: fresh batch, fresh fakes, no R1
        images, _labels = next(loader)
        d_loss, aux = d_step(P, G, D, opt_D, opt, images, step, red_D, style_mix, r1=False)
    G.eval(); D.eval()
    THROTTLE.end()
    out.update({'D_loss': d_loss.detach(), 'D_penalty': aux['penalty'].detach(), 'D_real': aux['d_real'].detach(),
                'D_gen': aux['d_gen'].detach(), 'lr_note': lr_note})
    return out


def _synthetic_loader(batch, image_size, device, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    h, w, c = image_size
    pool = [torch.rand(batch, c, h, w, generator=g).to(device) for _ in range(4)]     # resident, cycled
    i = 0
    while True:
        yield pool[i % len(pool)], None
        i += 1


def _dataset_loader(name, batch, rank, world, workers):
    import torchvision
    import torchvision.transforms as T
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    root = os.environ.get('DATA_DIR', 'data/')
    if name.startswith('cifar'):
        cls = torchvision.datasets.CIFAR100 if name.startswith('cifar100') else torchvision.datasets.CIFAR10
        tf = [T.RandomHorizontalFlip()] if name.endswith('hflip') else []
        ds = cls(root, train=True, download=False, transform=T.Compose(tf + [T.ToTensor()]))
    elif name.startswith('afhq_'):
        ds = torchvision.datasets.ImageFolder(os.path.join(root, 'afhq/%s/train' % name[5:]),
                                              T.Compose([T.RandomHorizontalFlip(), T.ToTensor()]))
    elif name == 'celeba128':
        ds = torchvision.datasets.ImageFolder(os.path.join(root, 'CelebAMask-HQ/CelebA-128-split/train'), T.ToTensor())
    else:
        raise NotImplementedError(name)
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True)
    loader = DataLoader(ds, shuffle=False, pin_memory=True, num_workers=workers, batch_size=batch, sampler=sampler,
                        drop_last=True)
    epoch = 0
    while True:
        for images, targets in loader:
            yield images.cuda(non_blocking=True), targets
        epoch += 1
        sampler.set_epoch(epoch)


def _prepare(P, options, contrad_script):
    if P.batch_size is not None:
        options['batch_size'] = P.batch_size
    if options['loss'] != 'nonsat' and contrad_script:
        raise NotImplementedError('train_stylegan2_contraD.py hard-codes the non-saturating loss (:105,:113)')
    if P.no_lazy:
        P.d_reg_every = 1
    if P.ema_start_k is None:
        P.ema_start_k = P.halflife_k
    P.accum = 0.5 ** (options['batch_size'] / (P.halflife_k * 1000))       # (the global batch: the ranks divide it later)


def _logdir(P, contrad_script):
    desc = f"R{P.lbd_r1}_mix{P.style_mix}_H{P.halflife_k}"
    if P.halflife_lr > 0:
        desc += f"_lr{P.halflife_lr / 1000000:.1f}M"
    desc += "_NoLazy" if P.no_lazy else "_Lazy"
    sub = 'gan_dp' if contrad_script else 'gan'
    return f'logs/{sub}/st_{P.gin_stem}/{P.architecture}/{P.filename}_{desc}{P.comment}'


def script(contrad_script):
    return train_driver.Script(
        get_options=get_options_dict, image_sizes=IMAGE_SIZES, logdir=lambda P: _logdir(P, contrad_script),
        synthetic_loader=_synthetic_loader, dataset_loader=_dataset_loader, make_critic=GraphedCritic,
        not_contrad=NOT_CONTRAD,
        graph_refusal=None if contrad_script else
        "--graph: train_stylegan2_contraD.py only (train_stylegan2.py feeds the D-step the G-step's fakes)",
        prepare=lambda P, options: _prepare(P, options, contrad_script), divisible_batch=True, seed_cuda=True, ema=True,
        start_up_lines=lambda P: [f"Use G moving average: {P.accum}"])


def main(argv=None, contrad_script=False):
    run = train_driver.build_run(parse_args(argv, contrad_script), script(contrad_script))
    return train_driver.run_loop(run, lambda step: train_iteration(
        run.P, run.options, run.G, run.D, run.g_ema, run.opt_G, run.opt_D, run.loader, step, run.reducers, contrad_script,
        run.graphed))


if __name__ == '__main__':
    main()
