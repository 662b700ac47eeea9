"""What the three training scripts share: the common flags, rank / process group, options, networks and optimizers, the
rank-0 log, the gradient exchange, the loader choice, the monitoring hooks (``HOOKS``: one list, in evaluation order, walked
by four loops -- add the flags, check them, build the monitors on rank 0, evaluate), the ``--graph`` gate and the loop with
its log line and checkpoints.  ``train_gan`` and ``train_stylegan2`` keep what their reference counterparts do differently
and hand it over as a ``Script``; their ``main()`` is ``build_run`` + ``run_loop``."""
import os
import time
from argparse import ArgumentParser
from dataclasses import dataclass
from pathlib import Path
from types import SimpleNamespace
from typing import Callable, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import config, contrast, knn, latent, prdc, spectrum, swd
from .augment import get_augment
from .data import loader_for
from .engine import GradAllReducer, setup_grad_exchange
from .evaluate.gan import LastBatch, Monitor
from .hooks import Hook
from .models.gan import get_architecture
from .optim import FusedAdam
from .training.gan import BASELINE_MODES, setup

# The flags every script has, with one help text.  A script's parser is a layout over them (``make_parser``): the order
# its ``--help`` lists them in, its own flags, and the defaults / help texts in which it differs.
COMMON_FLAGS = {
    'gin_config': dict(type=str, help='Path to the gin configuration file'),
    'architecture': dict(type=str, help='Architecture'),
    '--mode': dict(default='std', type=str, help='Training mode (contrad | simclr_only | std | aug | aug_both)'),
    '--penalty': dict(default='none', type=str),
    '--aug': dict(default='none', type=str,
                  help='Augmentation (simclr | simclr_hq | simclr_hq_cutout | none | hflip | hfrt | diffaug; diffaug needs a gin '
                       'file that binds augment.diffaug_policy = "color,cutout", as configs/gan/diffaug/c10_diffaug.gin '
                       'does: with any other file it raises NotImplementedError until the line is added)'),
    '--use_warmup': dict(action='store_true', help='Use warmup strategy on LR'),
    '--temp': dict(default=0.1, type=float),
    '--lbd_a': dict(default=1.0, type=float),
    # FID / GIF logging is outside the hot path (out of scope) -- the flags are accepted so that the
    # reference's command lines run unchanged
    '--no_fid': dict(action='store_true'),
    '--no_gif': dict(action='store_true',
                     help='with --monitor: keep only the latest fixed-latent grid (fixed_gen_<seed>.png), no '
                          'per-step files and no animation; without --monitor accepted and ignored'),
    '--n_eval_avg': dict(default=3, type=int),
    '--print_every': dict(default=50, type=int),
    '--evaluate_every': dict(default=2000, type=int, help='checkpoint period (steps)'),
    '--save_every': dict(default=100000, type=int),
    '--comment': dict(default='', type=str),
    '--resume': dict(default=None, type=str),
    '--finetune': dict(default=None, type=str),
    '--workers': dict(type=int),
    '--port': dict(type=int),
    # additions
    '--synthetic': dict(action='store_true', help='uniform-random images instead of a dataset'),
    '--data': dict(default=None, type=str,
                   help='npz with x_train uint8 [n, H, W, 3] (tools/make_image_npz.py): the set lives on the device, batches '
                        'are gathered there (contrad_amd/data.py; no torchvision)'),
    '--max_steps': dict(default=None, type=int, help='override options.max_steps'),
    '--logdir': dict(default=None, type=str),
    '--seed': dict(default=0, type=int),
    '--graph': dict(action='store_true'),
    '--monitor': dict(action='store_true'),
}


def monitor_help(shows):
    return ('rank 0 writes image grids at every evaluate_every: progress_<seed>/step_<step>.png and the animated '
            'training_progress_<seed>.png (%s), real_augment_<seed>.png; the training trajectory is unchanged' % shows)


# ``--monitor``: the image grids.  Its flag (and ``--no_gif``) is in the scripts' layouts, with their own help text.
GRIDS = Hook(flags=(), switch='monitor',
             build=lambda H, run: Monitor(*run.head, no_gif=run.P.no_gif, P=run.P, last_batch=lambda: run.loader.last),
             log_lines=lambda monitor, step, out: ())

# Every monitoring hook, in the order of one evaluation (and of its lines in log.txt).  PRDC is last: it decides ``_best``.
HOOKS = (GRIDS, knn.HOOK, contrast.HOOK, swd.HOOK, spectrum.HOOK, latent.HOOK, prdc.HOOK)
HELP_ORDER = (knn.HOOK, prdc.HOOK) + HOOKS[2:-1]        # --help keeps PRDC's flags where they have always been, behind kNN's


def make_parser(description, layout):
    """``layout``: the script's flags in ``--help`` order -- the name of a common flag, or ``(name, kwargs)`` for a flag of
    the script's own or for what it sets differently on a common one.  The flags of ``HOOKS`` come last."""
    parser = ArgumentParser(description=description)
    for item in layout:
        name, own = (item, {}) if isinstance(item, str) else item
        parser.add_argument(name, **dict(COMMON_FLAGS.get(name, {}), **own))
    for hook in HELP_ORDER:
        hook.add_arguments(parser)
    return parser


@dataclass
class Script:
    """What one training script does differently from the others (the reference's scripts differ in the same places)."""
    get_options: Callable                   # its gin-configurable ``get_options_dict``
    image_sizes: dict                       # the datasets it drives (a subset of data.IMAGE_SIZES)
    logdir: Callable                        # P -> the run's default log directory
    synthetic_loader: Callable              # (batch, image_size, device, seed) -> iterator of (images, labels)
    dataset_loader: Callable                # (name, batch, rank, world, workers) -> the same over torchvision's files
    make_critic: Callable                   # () -> its engine.GraphedCritic
    not_contrad: str                        # --graph with another --mode: the refusal (one %s)
    graph_refusal: Optional[str] = None     # --graph refused whatever the mode
    dataset_hint: str = ''                  # appended to the refusal of a dataset outside ``image_sizes``
    prepare: Optional[Callable] = None      # (P, options): its own flags' effect on both, before the per-rank batch
    divisible_batch: bool = False           # ValueError unless the ranks divide the batch; options['global_batch_size']
    seed_cuda: bool = False                 # torch.cuda.manual_seed with the rank's seed as well
    ema: bool = False                       # a third network g_ema: monitored, saved as gen_ema.pt
    data_keeps_partial_batch: bool = False  # --data: drop_last only where a captured step needs one batch size
    start_up_lines: Optional[Callable] = None   # P -> further lines of the log's head


def per_rank_batch(options, world, divisible):
    """The global batch of the gin file -> this rank's.  ``divisible``: the StyleGAN2 scripts' rule (their schedules count
    global images, kept as ``global_batch_size``); train_gan floors (train_gan.py:247)."""
    if divisible:
        if options['batch_size'] % world:
            raise ValueError('batch_size %d is not divisible by the %d ranks' % (options['batch_size'], world))
        options['global_batch_size'] = options['batch_size']
    options['batch_size'] = options['batch_size'] // world


def graph_gate(P, script):
    """``--graph``: (the script's GraphedCritic or None, the log line that says why not)."""
    if not P.graph:
        return None, None
    if script.graph_refusal is not None:
        return None, script.graph_refusal + ' -> eager'
    if P.mode != 'contrad':
        return None, script.not_contrad % P.mode + ' -> eager'
    return script.make_critic(), None


def _rank_and_group(P):
    """The launcher's environment -> (rank, world, device); with several ranks the process group.  The baseline modes are
    refused before the first CUDA call."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1 and P.mode in BASELINE_MODES:
        raise NotImplementedError("--mode=%s runs on one GPU (WORLD_SIZE=%d): the gradient exchange inside D's backward assumes "
                                  "one discriminator call per step, and the baseline modes (%s) with cr / bcr make two"
                                  % (P.mode, world, ', '.join(BASELINE_MODES)))
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(P.port))
        dist.init_process_group('nccl', device_id=dev)
    P.rank, P.distributed = rank, world > 1
    return rank, world, dev


def _options(P, script, world):
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'), P.gin_config])
    options = script.get_options()
    if P.max_steps is not None:
        options['max_steps'] = P.max_steps
    if script.prepare is not None:
        script.prepare(P, options)
    if options['dataset'] not in script.image_sizes:
        raise NotImplementedError("dataset '%s'%s" % (options['dataset'], script.dataset_hint))
    per_rank_batch(options, world, script.divisible_batch)
    return options


def _loader(P, script, options, image_size, rank, world, dev, log):
    use_synth = P.synthetic
    if not use_synth and not P.data:
        try:
            import torchvision  # noqa: F401
        except ImportError:
            log('torchvision not available -> --synthetic (--data FILE.npz trains on real images without it)')
            use_synth = True
    if P.data and not use_synth:
        drop_last = True
        if script.data_keeps_partial_batch:
            # a captured step has ONE batch size (GraphedDStep.load_images copies into a fixed buffer)
            drop_last = bool(P.graph and P.mode == 'contrad')
            if drop_last:
                log("--graph: one captured batch size -> the loader drops each epoch's last partial batch")
        return loader_for(P.data, options['dataset'], image_size, options['batch_size'], rank, world, drop_last, dev)
    if use_synth:
        return script.synthetic_loader(options['batch_size'], image_size, dev, P.seed + rank)
    return script.dataset_loader(options['dataset'], options['batch_size'], rank, world, P.workers)


def build_run(P, script):
    """Everything between the parsed command line and the first iteration -> the run: P, options, G, D, g_ema (or None),
    opt_G, opt_D, reducers, loader, graphed, monitors (rank 0: ``(hook, monitor)`` of every hook that is on, in the order
    of ``HOOKS``), and what ``run_loop`` needs around them."""
    checked = [(hook, hook.check(P)) for hook in HOOKS]             # (refusals that need no device come first)
    if P.comment:
        P.comment = '_' + P.comment
    P.gin_stem = Path(P.gin_config).stem
    P = setup(P)
    rank, world, dev = _rank_and_group(P)
    options = _options(P, script, world)
    image_size = script.image_sizes[options['dataset']]

    torch.manual_seed(P.seed); np.random.seed(P.seed)               # identical initial weights on all ranks
    nets = dict(zip(('gen', 'dis'), get_architecture(P.architecture, image_size, P=P)))
    if script.ema:
        nets['gen_ema'] = get_architecture(P.architecture, image_size, P=P)[0]
    if P.resume:
        for name, net in nets.items():
            net.load_state_dict(torch.load(f"{P.resume}/{name}.pt", map_location='cpu'))
    if P.finetune:
        nets['dis'].load_state_dict(torch.load(f"{P.finetune}/dis.pt", map_location='cpu'), strict=False)
        nets['dis'].reset_parameters(nets['dis'].linear)
        P.comment += 'ft'
    nets = {name: net.to(dev) for name, net in nets.items()}
    G, D, g_ema = nets['gen'], nets['dis'], nets.get('gen_ema')
    if g_ema is not None:
        g_ema.eval()
    torch.manual_seed(P.seed + 1000 * (rank + 1)); np.random.seed(P.seed + 1000 * (rank + 1))
    if script.seed_cuda:
        torch.cuda.manual_seed(P.seed + 1000 * (rank + 1))
    # (neither of the next two draws a random number, on the host or the device: their order is free)
    P.augment_fn = get_augment(mode=P.aug).to(dev)
    opt_G = FusedAdam(G.parameters(), lr=options["lr"], betas=tuple(options["beta"]))
    opt_D = FusedAdam(D.parameters(), lr=options["lr_d"], betas=tuple(options["beta"]))
    starting_step = 1
    if P.resume:
        ck = torch.load(f"{P.resume}/optim.pt", map_location=dev)
        opt_G.load_state_dict(ck['optim_G']); opt_D.load_state_dict(ck['optim_D'])
        starting_step = ck['epoch'] + 1

    logdir = P.logdir or P.resume or script.logdir(P)
    log_file = None
    if rank == 0:
        os.makedirs(logdir, exist_ok=True)
        log_file = open(os.path.join(logdir, 'log.txt'), 'a')

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
            log_file.write(msg + '\n'); log_file.flush()

    reducers = (None, None)
    if world > 1:
        reducers = (GradAllReducer(G.parameters()), setup_grad_exchange(D))      # D: weights exchanged inside the backward
    loader = _loader(P, script, options, image_size, rank, world, dev, log)
    log(f"# Params - G: {sum(p.numel() for p in G.parameters())}, D: {sum(p.numel() for p in D.parameters())}")
    log(str(options))
    for line in (script.start_up_lines(P) if script.start_up_lines is not None else ()):
        log(line)

    if P.monitor and rank == 0:
        loader = LastBatch(loader)                                  # the preview shows the batch the step drew
    monitor_run = SimpleNamespace(head=(logdir, P.architecture, image_size, dev, P.seed), P=P, loader=loader,
                                  batch=options['batch_size'] * world, resumed_step=starting_step - 1)
    monitors = [(hook, hook.build(H, monitor_run)) for hook, H in checked if rank == 0 and hook.on(P)]
    graphed, why_not = graph_gate(P, script)
    if why_not:
        log(why_not)
    return SimpleNamespace(P=P, options=options, G=G, D=D, g_ema=g_ema, opt_G=opt_G, opt_D=opt_D, reducers=reducers,
                           loader=loader, graphed=graphed, nets=nets, rank=rank, world=world, logdir=logdir, log=log,
                           starting_step=starting_step, monitors=monitors)


def run_loop(run, iteration):
    """``iteration(step)`` -> the step's loss tensors (and ``lr_note``: the learning rates a schedule just set, or None)
    from the run's starting step to ``max_steps``; the log line every ``print_every`` steps, monitors and checkpoints
    (rank 0) every ``evaluate_every``.  Returns the log directory."""
    P, log, logdir = run.P, run.log, run.logdir
    images_per_step = run.options['batch_size'] * run.world
    t0 = time.time()
    for step in range(run.starting_step, run.options['max_steps'] + 1):
        losses = iteration(step)
        if losses.get('lr_note'):
            log('LR Updated: [G %.5f] [D %.5f]' % losses['lr_note'])
        if step % P.print_every == 0:
            vals = {k: float(v) for k, v in losses.items() if torch.is_tensor(v)}      # the only host sync of the loop
            log('[Steps %7d] [G %.3f] [D %.3f] [pen %.3f]%s [%.1f img/s]' %
                (step, vals['G_loss'], vals['D_loss'], vals['D_penalty'],
                 (' [r1 %.4g]' % vals['D_r1']) if 'D_r1' in vals else '',
                 P.print_every * images_per_step / max(time.time() - t0, 1e-9)))
            t0 = time.time()
        if step % P.evaluate_every == 0 and run.rank == 0:
            tags = ('', f'_{step}') if step % P.save_every == 0 else ('',)
            for hook, monitor in run.monitors:
                out = monitor.update(step, run.D if hook.shown == 'D' else run.g_ema if run.g_ema is not None else run.G)
                for line in hook.log_lines(monitor, step, out):
                    log(line)
                if hook.improved is not None and hook.improved(out):
                    tags += ('_best',)
            for tag in tags:
                for name, net in run.nets.items():
                    torch.save(net.state_dict(), f'{logdir}/{name}{tag}.pt')
            torch.save({'epoch': step, 'optim_G': run.opt_G.state_dict(), 'optim_D': run.opt_D.state_dict()},
                       logdir + '/optim.pt')
    if run.world > 1:
        dist.destroy_process_group()
    return logdir
