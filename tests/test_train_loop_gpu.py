"""GPU smoke of the full training loop (D-step + G-step, warm-up, checkpoint + resume) through the CLI entry, and the
iteration functions of the three scripts against the same iterations written out on the engine steps, bitwise."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_gan_cli_runs_checkpoints_and_resumes(tmp_path):
    from contrad_amd.train_gan import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gin = os.path.join(root, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    logdir = str(tmp_path / 'run')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--use_warmup', '--synthetic', '--max_steps', '4',
          '--print_every', '2', '--evaluate_every', '4', '--logdir', logdir])
    for f in ('gen.pt', 'dis.pt', 'optim.pt', 'log.txt'):
        assert os.path.exists(os.path.join(logdir, f)), f
    sd = torch.load(os.path.join(logdir, 'dis.pt'))
    assert 'main.0.weight_orig' in sd and 'main.0.weight_u' in sd and all(torch.isfinite(v).all() for v in sd.values())
    ck = torch.load(os.path.join(logdir, 'optim.pt'))
    assert ck['epoch'] == 4
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '6', '--print_every', '1',
          '--resume', logdir])
    log = open(os.path.join(logdir, 'log.txt')).read()
    assert '[Steps       6]' in log and 'nan' not in log.lower()


def _gin(*names):
    from contrad_amd import config
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'gan', *names)])


def _batches(n, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(N, 3, 32, 32, generator=g).cuda() for _ in range(n)]


def _seed(s):
    torch.manual_seed(s); np.random.seed(s); torch.cuda.manual_seed(s)


def _tensors(modules, optimizers):
    """Every parameter and buffer of ``modules`` and every Adam state entry of ``optimizers``, in a fixed order."""
    out = [(k, v.detach().clone()) for m in modules for k, v in m.state_dict().items()]
    for opt in optimizers:
        for i, p in enumerate(opt.param_groups[0]['params']):
            out += [('opt%d.%s' % (i, k), v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()]
    return out


def _assert_same_runs(a, b):
    (ta, la), (tb, lb) = a, b
    assert [k for k, _ in ta] == [k for k, _ in tb] and len(ta) > 0
    for (k, x), (_, y) in zip(ta, tb):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y, k
    assert len(la) == len(lb)
    for x, y in zip(la, lb):
        assert sorted(x) == sorted(y)
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_train_step_is_the_engine_steps_in_the_reference_order():
    """train_gan.train_step (SNDCGAN, N = 8, contrad / simclr, n_critic 2, warm-up over 2 steps) against the same three
    iterations written out: warm-up, set_grad, engine.d_step per critic batch, the generator step -- every parameter,
    buffer, Adam state tensor and returned loss, bitwise."""
    from contrad_amd import engine, train_gan
    from contrad_amd.augment import get_augment
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.optim import FusedAdam
    from contrad_amd.training.gan import setup
    N, K = 8, 3
    batches = _batches(6, N, 1)

    def build():
        _gin('cifar10', 'c10_b64.gin')
        P = setup(train_gan.parse_args(['c10_b64.gin', 'sndcgan', '--mode=contrad', '--aug=simclr', '--use_warmup']))
        P.rank, P.distributed = 0, False
        opt = train_gan.get_options_dict()
        opt['n_critic'], opt['warmup'] = 2, 2
        _seed(0)
        G, D = get_architecture('sndcgan', (32, 32, 3), P=P)
        G, D = G.cuda(), D.cuda()
        P.augment_fn = get_augment(mode='simclr').cuda()
        opt_G = FusedAdam(G.parameters(), lr=opt['lr'], betas=tuple(opt['beta']))
        opt_D = FusedAdam(D.parameters(), lr=opt['lr_d'], betas=tuple(opt['beta']))
        return P, opt, G, D, opt_G, opt_D, ((x, None) for x in batches)

    P, opt, G, D, opt_G, opt_D, loader = build()
    _seed(7)
    losses = [train_gan.train_step(P, opt, G, D, opt_G, opt_D, loader, step, (None, None)) for step in range(1, K + 1)]
    run_a = (_tensors((G, D), (opt_G, opt_D)), losses)

    P, opt, G, D, opt_G, opt_D, loader = build()
    _seed(7)
    losses = []
    for step in range(1, K + 1):
        G.train(); D.train()
        for o, lr in ((opt_G, opt['lr']), (opt_D, opt['lr_d'])):
            for group in o.param_groups:
                group['lr'] = min(1., (step + 1) / opt['warmup']) * lr
        engine.set_grad(G, False); engine.set_grad(D, True)
        for _ in range(opt['n_critic']):
            images, _labels = next(loader)
            d_loss, aux = engine.d_step(P, G, D, opt_D, opt, images)
        engine.set_grad(G, True); engine.set_grad(D, False)
        gen_images = engine.sample_generator(G, images.size(0))
        g_loss = P.train_fn["G"](P, D, opt, images, gen_images)
        opt_G.zero_grad()
        g_loss.backward()
        opt_G.step()
        losses.append({'G_loss': g_loss.detach(), 'D_loss': d_loss.detach(), 'D_penalty': aux['penalty'].detach(),
                       'D_real': aux['d_real'].detach(), 'D_gen': aux['d_gen'].detach()})
    _assert_same_runs(run_a, (_tensors((G, D), (opt_G, opt_D)), losses))


@pytest.mark.parametrize('contrad_script', [True, False])
def test_train_iteration_is_the_engine_steps_in_the_reference_order(contrad_script):
    """train_stylegan2.train_iteration (stylegan2 at 32 x 32, batch 8, lazy R1 every 2nd step, n_critic 2: the lazy-R1
    steps and the extra critic iteration both run) against the same four iterations written out: EMA accumulate, the
    generator step, the D-step (the ContraD script: engine.d_step_stylegan2_contrad; train_stylegan2: the G-step's fakes,
    one 3N call, the R1 term as engine adds it), the extra critic step.  Bitwise, g_ema included; 'D_r1' on steps 2, 4."""
    from contrad_amd import engine, train_stylegan2 as T
    from contrad_amd.augment import get_augment
    from contrad_amd.models.gan import get_architecture
    from contrad_amd.optim import FusedAdam
    from contrad_amd.training.gan import setup
    N, K = 8, 4
    batches = _batches(2 * K, N, 1)

    def build():
        _gin('stylegan2', 'c10_style64.gin')
        P = setup(T.parse_args(['c10_style64.gin', 'stylegan2', '--mode=contrad', '--aug=simclr', '--lbd_r1', '0.1',
                                '--d_reg_every', '2', '--ema_start_k', '0', '--halflife_k', '1'], contrad_script))
        P.rank, P.distributed = 0, False
        opt = T.get_options_dict()
        opt['n_critic'], opt['batch_size'], opt['global_batch_size'] = 2, N, N
        P.accum = 0.5 ** (N / (P.halflife_k * 1000))
        _seed(0)
        G, D = get_architecture('stylegan2', (32, 32, 3), P=P)
        g_ema, _ = get_architecture('stylegan2', (32, 32, 3), P=P)
        G, D, g_ema = G.cuda(), D.cuda(), g_ema.cuda()
        g_ema.eval()
        P.augment_fn = get_augment(mode='simclr').cuda()
        opt_G = FusedAdam(G.parameters(), lr=opt['lr'], betas=tuple(opt['beta']))
        opt_D = FusedAdam(D.parameters(), lr=opt['lr_d'], betas=tuple(opt['beta']))
        return P, opt, G, D, g_ema, opt_G, opt_D, ((x, None) for x in batches)

    P, opt, G, D, g_ema, opt_G, opt_D, loader = build()
    _seed(7)
    losses = []
    for step in range(1, K + 1):
        out = T.train_iteration(P, opt, G, D, g_ema, opt_G, opt_D, loader, step, (None, None), contrad_script)
        assert out.pop('lr_note') is None
        losses.append(out)
    run_a = (_tensors((G, D, g_ema), (opt_G, opt_D)), losses)
    assert [('D_r1' in out) for out in losses] == [False, True, False, True]

    P, opt, G, D, g_ema, opt_G, opt_D, loader = build()
    _seed(7)
    losses = []
    style_mix = 0.9                     # --style_mix's default, and what the ContraD script always uses
    for step in range(1, K + 1):
        out = {}
        T.accumulate(g_ema, G, P.accum)                                     # step * 8 > ema_start_k * 1000 = 0
        G.train(); D.train()
        images, _labels = next(loader)
        engine.set_grad(G, True); engine.set_grad(D, False)
        gen_images = T.sample_generator(G, N, style_mix=style_mix, enable_grad=True)
        if contrad_script:
            d_gen, _aux = D(P.augment_fn(gen_images), sg_linear=False, projection=True, projection2=True)
            g_loss = T.loss_G_nonsat(d_gen)
        else:
            g_loss = P.train_fn["G"](P, D, opt, images, gen_images)
        opt_G.zero_grad()
        g_loss.backward()
        opt_G.step()
        out['G_loss'] = g_loss.detach()
        engine.set_grad(G, False); engine.set_grad(D, True)
        if contrad_script:
            d_loss, aux = engine.d_step_stylegan2_contrad(P, G, D, opt_D, opt, images, step, None, 0.9)
            if 'r1' in aux:
                out['D_r1'] = aux['r1'].detach()
        else:
            d_loss, aux = P.train_fn["D"](P, D, opt, images, gen_images.detach())
            loss = d_loss + aux['penalty']
            if step % P.d_reg_every == 0:
                r1 = engine.r1_loss(D, images, P.augment_fn)
                loss = torch.add(loss, r1, alpha=(0.5 * P.lbd_r1) * P.d_reg_every)
                out['D_r1'] = r1.detach()
            opt_D.zero_grad()
            loss.backward()
            opt_D.step()
        images, _labels = next(loader)                                      # the extra critic iteration: no R1
        gen_images = T.sample_generator(G, N, style_mix=style_mix, enable_grad=False)
        if contrad_script:
            d_loss, aux = engine.loss_D_fn_separate(P, D, opt, images, gen_images)
        else:
            d_loss, aux = P.train_fn["D"](P, D, opt, images, gen_images)
        opt_D.zero_grad()
        (d_loss + aux['penalty']).backward()
        opt_D.step()
        G.eval(); D.eval()
        out.update({'D_loss': d_loss.detach(), 'D_penalty': aux['penalty'].detach(), 'D_real': aux['d_real'].detach(),
                    'D_gen': aux['d_gen'].detach()})
        losses.append(out)
    _assert_same_runs(run_a, (_tensors((G, D, g_ema), (opt_G, opt_D)), losses))
