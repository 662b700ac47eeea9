"""Host-side logic that needs no GPU: RNG draw order of the augmentation samplers against the oracle (incl. simclr_hq
and simclr_hq_cutout), state-dict contracts of every architecture against the oracle's tables / the reference manifest,
the LR schedules and EMA schedule of the StyleGAN2 loops, the optimizer's graph-replay scalars, gin parsing."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import contrad_oracle as O
from oracle import stylegan2_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('mode,cfg,size', [('simclr', O.SIMCLR_CIFAR, 32), ('simclr_hq', O.SIMCLR_HQ_AFHQ, 64),
                                           ('simclr_hq_cutout', O.SIMCLR_HQ_CUTOUT_AFHQ, 96)])
def test_host_sampler_reproduces_the_reference_draw_order(mode, cfg, size):
    from contrad_amd import config
    from contrad_amd.augment import get_augment
    config.clear_config()
    files = [os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin')]
    if mode != 'simclr':
        files.append(os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'afhq_dog_style64.gin'))
    config.parse_config_files_and_bindings(files)
    aug = get_augment(mode=mode)
    for seed in (0, 1, 2):
        B = 24
        torch.manual_seed(seed); np.random.seed(seed)
        P, cf, sigma = aug.sample(B, size, size)
        torch.manual_seed(seed); np.random.seed(seed)
        p = O.sample_simclr_params(B, size, size, cfg)
        th = p['theta']
        assert torch.equal(P[:, 0], th[:, 0, 0]) and torch.equal(P[:, 1], th[:, 1, 1])
        assert torch.equal(P[:, 2], th[:, 0, 2]) and torch.equal(P[:, 3], th[:, 1, 2])
        for col, key in ((4, 'flip_sign'), (5, 'jitter_mask'), (6, 'f_contrast'), (7, 'f_h'), (8, 'f_s'), (9, 'f_v'),
                         (10, 'gray_mask')):
            assert torch.equal(P[:, col], p[key]), (mode, key)
        assert cf == p['contrast_first'] and P[0, 15].item() == float(cf)
        if 'blur_mask' in p:
            assert torch.equal(P[:, 11], p['blur_mask']) and abs(sigma - p['sigma']) < 1e-15
        else:
            assert sigma is None
        if 'cut_mask' in p:
            assert torch.equal(P[:, 12], p['cut_mask'])
            assert torch.equal(P[:, 13], p['cut_h'].float()) and torch.equal(P[:, 14], p['cut_w'].float())
    with pytest.raises(NotImplementedError):
        get_augment(mode='diffaug')


def test_state_dict_contracts_of_every_architecture():
    from contrad_amd.models.gan import get_architecture
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'checkpoint_manifest.json')))
    G, D = get_architecture('sndcgan', (32, 32, 3))
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == O.sndcgan_d_param_shapes()
    assert [[k, list(v.shape), str(v.dtype)] for k, v in G.state_dict().items()] == man['sndcgan']['gen']
    G, D = get_architecture('snresnet18', (32, 32, 3))
    shapes = O.snresnet18_param_shapes()
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == shapes and list(D.state_dict()) == list(shapes)
    assert D.d_hidden == 1024 and D.d_penul == 512
    G, D = get_architecture('stylegan2', (32, 32, 3))
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == S.d_param_shapes(32, True)
    assert {k: tuple(v.shape) for k, v in G.state_dict().items()} == S.g_param_shapes(32, True)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in D.state_dict().items()] == man['stylegan2']['dis']
    G, D = get_architecture('stylegan2_512', (512, 512, 3))
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == S.d_param_shapes(512, False, 1.0)
    assert {k: tuple(v.shape) for k, v in G.state_dict().items()} == S.g_param_shapes(512, False, 1.0)
    with pytest.raises(NotImplementedError):
        get_architecture('resnet50', (32, 32, 3))
    # no CPU fallback: the product refuses CPU tensors instead of silently computing somewhere else
    with pytest.raises(RuntimeError):
        D(torch.rand(2, 3, 512, 512))


def test_stylegan2_loop_schedules():
    """_update_warmup / _update_lr (train_stylegan2.py:86-103), the EMA constants (:303-308), option defaults (:126-144)."""
    from contrad_amd import config
    from contrad_amd.train_stylegan2 import IMAGE_SIZES, _update_lr, _update_warmup, get_options_dict, parse_args
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    _update_warmup(opt, 0, 3000, 2e-3)
    assert abs(opt.param_groups[0]['lr'] - min(1., 1 / (3000 + 1e-8)) * 2e-3) < 1e-18
    _update_warmup(opt, 5000, 3000, 2e-3)
    assert opt.param_groups[0]['lr'] == 2e-3
    _update_warmup(opt, 5, 0, 7.0)
    assert opt.param_groups[0]['lr'] == 2e-3                     # warmup 0: untouched
    assert _update_lr(opt, 1500, 64, 1000000, 2e-3) is None      # only every 1000 steps
    assert _update_lr(opt, 2000, 64, 0, 2e-3) is None            # halflife_lr 0: off
    lr = _update_lr(opt, 2000, 64, 1000000, 2e-3)
    assert abs(lr - 0.5 ** (2000 * 64 / 1000000) * 2e-3) < 1e-12 and opt.param_groups[0]['lr'] == lr
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'afhq_dog_style64.gin')])
    o = get_options_dict()
    assert (o['dataset'], o['batch_size'], o['lr'], o['lr_d'], tuple(o['beta']), o['n_critic'], o['warmup']) == \
        ('afhq_dog', 64, 0.0025, 0.0025, (0.0, 0.99), 1, 3000)
    assert IMAGE_SIZES[o['dataset']] == (512, 512, 3) and IMAGE_SIZES['cifar10_hflip'] == (32, 32, 3)
    P = parse_args(['x.gin', 'stylegan2_512', '--mode=contrad', '--aug=simclr_hq', '--lbd_r1=0.5', '--no_lazy'])
    assert (P.d_reg_every, P.style_mix, P.halflife_k, P.ema_start_k, P.lbd_r1, P.no_lazy) == (16, 0.9, 20, None, 0.5, True)
    # the reference's EMA decay: accum = 0.5 ** (batch / (halflife_k * 1000))
    assert abs(0.5 ** (64 / (20 * 1000)) - 0.99778429) < 1e-7


def test_fused_adam_graph_scalars_follow_the_launcher_arithmetic():
    """FusedAdam.hyper_values == what contrad_adam_step computes from its float arguments (bitwise-equal replay)."""
    import struct
    from contrad_amd.optim import FusedAdam
    f32 = lambda v: struct.unpack('f', struct.pack('f', v))[0]
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([p], lr=2e-4, betas=(0.5, 0.999))
    opt.state[p] = {'step': 6, 'exp_avg': torch.zeros(4), 'exp_avg_sq': torch.zeros(4)}
    v0 = p._version
    h = opt.hyper_values(grad_scale=0.125)
    assert int(opt.state[p]['step']) == 7 and p._version == v0 + 1
    b1, b2 = f32(0.5), f32(0.999)
    assert h[0] == f32(2e-4) / (1.0 - b1 ** 7) and h[1] == 1.0 / math.sqrt(1.0 - b2 ** 7) and h[2] == 0.125


def test_packed_buffer_zero_fill_only_when_padding_exists():
    from contrad_amd.autograd_ops import _packed_buffer
    a = _packed_buffer((9 * 16, 32), 32, torch.device('cpu'))
    b = _packed_buffer((9 * 16, 4), 1, torch.device('cpu'))
    assert a.shape == (144, 32) and b.shape == (144, 4) and b.abs().sum().item() == 0.0


def test_bench_workload_table_matches_baseline_json():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    base = json.load(open(os.path.join(ROOT, 'BASELINE.json')))
    assert base['metric'].startswith('discriminator-step images/sec')
    c = bench.CONFIGS
    assert c['c10_b512']['batch'] == 512 and c['c10_b512']['batch_is_global'] and c['c10_b512']['flop_per_image'] == 4.28e9
    assert c['sg2_32']['batch'] == 64 and c['sg2_32']['d_reg_every'] == 1 and c['sg2_32']['lbd_r1'] == 0.1
    assert c['sg2_512']['batch'] == 16 and c['sg2_512']['d_reg_every'] == 16 and c['sg2_512']['aug'] == 'simclr_hq'
    for name, cfg in c.items():
        assert os.path.exists(os.path.join(ROOT, 'configs', *cfg['gin'])), name
    assert 1024 < bench._free_port() < 65536


def test_bench_graph_watchdog_prints_the_kept_eager_result_and_exits_zero():
    """bench.py's fallback order for N > 1: the eager result is kept, the capture runs under a
    per-rank deadline, past it rank 0 prints the line with the eager result and every rank leaves with exit code 0."""
    import json
    import subprocess
    import sys
    code = (
        "import sys, time, json; sys.path.insert(0, %r)\n"
        "import bench\n"
        "results = {'c10_b512': {'value': 1.0, 'config': {'launch': 'hipGraph replay'}}}\n"
        "names = ['c10_b512', 'sg2_32']\n"
        "def emit():\n"
        "    out = results[names[0]]\n"
        "    rest = {n: results[n] for n in names[1:] if n in results}\n"
        "    if rest: out['other_configs'] = rest\n"
        "    print(json.dumps(out), flush=True)\n"
        "wd = bench._GraphWatchdog(int(sys.argv[1]), 0.3, results, emit)\n"
        "wd.keep('sg2_32', {'value': 2.0, 'config': {'launch': 'eager (graph capture timed out)'}})\n"
        "wd.arm('sg2_32')\n"
        "time.sleep(30)\n"
        "print('not reached')\n" % ROOT)
    for rank, want_line in ((0, True), (1, False)):
        r = subprocess.run([sys.executable, '-c', code, str(rank)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120, text=True)
        assert r.returncode == 0 and 'not reached' not in r.stdout
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == (1 if want_line else 0)
        if want_line:
            out = json.loads(lines[0])
            assert out['value'] == 1.0 and out['other_configs']['sg2_32']['config']['launch'].startswith('eager (graph')
    # a disarmed watchdog never fires
    code2 = code.replace("time.sleep(30)", "wd.disarm('sg2_32'); time.sleep(1.0); print('reached')").replace("print('not reached')", "")
    r = subprocess.run([sys.executable, '-c', code2, '0'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, text=True)
    assert r.returncode == 0 and 'reached' in r.stdout and '{' not in r.stdout


def test_train_gan_accepts_every_flag_of_the_reference_cli():
    """train_gan.py:41-85: the reference's command lines must parse unchanged (logging flags are accepted and ignored)."""
    from contrad_amd.train_gan import parse_args
    a = parse_args(['configs/gan/cifar10/c10_b512.gin', 'sndcgan', '--mode', 'contrad', '--aug', 'simclr', '--use_warmup',
                    '--temp', '0.1', '--lbd_a', '1.0', '--no_fid', '--no_gif', '--n_eval_avg', '3', '--print_every', '50',
                    '--evaluate_every', '2000', '--save_every', '100000', '--comment', 'x', '--workers', '0',
                    '--world-size', '1', '--rank', '0', '--port', '40404'])
    assert a.mode == 'contrad' and a.no_fid and a.no_gif and a.n_eval_avg == 3 and a.world_size == 1 and a.rank == 0


class _FakeOptimizer(object):
    def __init__(self, with_state):
        self.state = {'p': {'step': 3}} if with_state else {}


def test_eager_first_gate():
    """captured.EagerFirst alone: the first use of a process is eager; the second captures only once the optimizer holds
    state; a resumed run (state from the start) still runs one eager step first; uses with ``counts=False`` (cDDLS with
    explicit noise) neither count nor capture."""
    from contrad_amd.captured import EagerFirst
    g = EagerFirst()                                     # no optimizer (lineval head, cDDLS)
    assert [g.may_capture() for _ in range(3)] == [False, True, True]

    g, opt = EagerFirst(), _FakeOptimizer(False)         # fresh run: the state appears with the first eager step
    assert not g.may_capture(opt)
    assert not g.may_capture(opt)                        # second use, but the optimizer is still empty
    opt.state['p'] = {'step': 1}
    assert g.may_capture(opt) and g.may_capture(opt)

    g, opt = EagerFirst(), _FakeOptimizer(True)          # --resume: state at once, cold process
    assert [g.may_capture(opt) for _ in range(3)] == [False, True, True]

    g = EagerFirst()                                     # explicit-noise steps
    assert not g.may_capture(counts=False) and not g.may_capture(counts=False) and g.eager == 0
    assert not g.may_capture()                           # the first counted use is still the eager one
    assert not g.may_capture(counts=False)               # ... and an explicit step never captures
    assert g.may_capture() and g.eager == 1


def test_graphed_critic_builds_each_step_once_behind_the_gate():
    """engine.GraphedCritic with stand-in factories: None (eager) in the first iteration, then one step object per
    half, fed the new real batch; any mode but contrad raises the script's own text; the step argument is passed on."""
    import argparse
    from contrad_amd.engine import GraphedCritic
    built = []

    class Step(object):
        def __init__(self, kind, *args):
            built.append((kind, args))
            self.loaded = []

        def load_images(self, images):
            self.loaded.append(images)

        def __call__(self, *step):
            return ('replayed',) + step

    critic = GraphedCritic(lambda *a: Step('d', *a), lambda *a: Step('g', *a), "not '%s'")
    P, opt_D, opt_G = argparse.Namespace(mode='contrad'), _FakeOptimizer(True), _FakeOptimizer(False)
    images = torch.zeros(4, 3, 8, 16)
    assert critic(P, 'opt', 'G', 'D', opt_D, images, 1) is None and critic.generator(P, 'opt', 'G', 'D', opt_G, images) is None
    opt_G.state['p'] = {'step': 1}
    assert critic(P, 'opt', 'G', 'D', opt_D, images, 2) == ('replayed', 2)
    assert critic(P, 'opt', 'G', 'D', opt_D, images) == ('replayed',)
    assert critic.generator(P, 'opt', 'G', 'D', opt_G, images) == ('replayed',)
    assert critic.generator(P, 'opt', 'G', 'D', opt_G, images) == ('replayed',)
    assert built == [('d', (P, 'G', 'D', opt_D, 'opt', images)), ('g', (P, 'G', 'D', opt_G, 'opt', 4, 8, 16))]
    assert len(critic.step.loaded) == 2

    other = GraphedCritic(lambda *a: Step('d', *a), lambda *a: Step('g', *a), "not '%s'")
    Pb = argparse.Namespace(mode='std')
    assert other(Pb, 'opt', 'G', 'D', opt_D, images) is None
    with pytest.raises(NotImplementedError, match="not 'std'"):
        other(Pb, 'opt', 'G', 'D', opt_D, images)


def test_captured_train_step_protocol_on_the_host(monkeypatch):
    """captured.CapturedTrainStep with the capture and the throttle replaced by recorders: the packed weights are dropped
    before and after the capture, the body's tail runs zero_grad -> backward -> reducer -> Adam and returns detached results,
    and a replay is throttle, inputs, the Adam scalars EXACTLY once (hyper_values advances the step count), graph."""
    from contrad_amd import captured
    log = []

    class Recorder(object):
        def __init__(self, *names):
            for n in names:
                setattr(self, n, lambda *a, _n=n, **k: log.append(_n))

    def fake_capture(body, modules, scratch):
        log.append(('capture', tuple(modules)))
        return Recorder('replay'), body()
    monkeypatch.setattr(captured, 'capture', fake_capture)
    monkeypatch.setattr(captured, 'THROTTLE', Recorder('begin', 'end'))

    class Opt(Recorder):
        steps = 0

        def hyper_values(self, grad_scale):
            self.steps += 1
            return [0.5 * self.steps, 0.25, grad_scale]

    class Step(captured.CapturedTrainStep):
        def __init__(self):
            super().__init__(Opt('zero_grad', 'step_captured'), lambda: log.append('reducer'), False, 'cpu')
            self.w = torch.ones(2, requires_grad=True)
            self._capture(quiesce=('D',), repack=(Recorder('invalidate_cache'),))

        def _refresh_inputs(self):
            log.append('inputs')

        def _body(self):
            loss = (self.w * 2).sum()
            return self._finish(loss, (loss, {'twice': loss * 2}))

    step = Step()
    assert log == ['invalidate_cache', ('capture', ('D',)), 'zero_grad', 'reducer', 'step_captured', 'invalidate_cache']
    assert torch.equal(step.w.grad, torch.full((2,), 2.0))
    del log[:]
    for k in (1, 2):
        d_loss, aux = step()
        assert not d_loss.requires_grad and not aux['twice'].requires_grad and (d_loss.item(), aux['twice'].item()) == (4.0, 8.0)
        assert step.opt.steps == k and step.hyper.tolist() == [0.5 * k, 0.25, 1.0]
    assert log == ['begin', 'inputs', 'replay', 'end'] * 2


_GAN_DEFAULTS = {
    'gin_config': 'c.gin', 'architecture': 'arch', 'mode': 'std', 'penalty': 'none', 'aug': 'none', 'use_warmup': False,
    'temp': 0.1, 'lbd_a': 1.0, 'no_fid': False, 'no_gif': False, 'n_eval_avg': 3, 'print_every': 50,
    'evaluate_every': 2000, 'save_every': 100000, 'comment': '', 'resume': None, 'finetune': None, 'workers': 0,
    'world_size': 1, 'rank': 0, 'port': 40404, 'synthetic': False, 'data': None, 'max_steps': None, 'logdir': None,
    'seed': 0, 'graph': False, 'monitor': False, 'knn_data': None, 'knn_k': 200, 'knn_temp': 0.1}
_SG2_DEFAULTS = {
    'gin_config': 'c.gin', 'architecture': 'arch', 'mode': 'std', 'penalty': 'none', 'aug': 'none', 'use_warmup': False,
    'workers': 8, 'temp': 0.1, 'lbd_a': 1.0, 'no_lazy': False, 'd_reg_every': 16, 'lbd_r1': 10, 'style_mix': 0.9,
    'halflife_k': 20, 'ema_start_k': None, 'halflife_lr': 0, 'no_fid': False, 'no_gif': False, 'n_eval_avg': 3,
    'print_every': 50, 'evaluate_every': 2000, 'save_every': 100000, 'comment': '', 'resume': None, 'finetune': None,
    'port': 40405, 'synthetic': False, 'data': None, 'max_steps': None, 'batch_size': None, 'logdir': None, 'seed': 0,
    'graph': False, 'monitor': False, 'knn_data': None, 'knn_k': 200, 'knn_temp': 0.1}
_SHARED_FLAGS = ['--mode', 'contrad', '--penalty', 'bcr', '--aug', 'simclr', '--use_warmup', '--temp', '0.2', '--lbd_a', '2.0',
                 '--no_fid', '--no_gif', '--n_eval_avg', '4', '--print_every', '5', '--evaluate_every', '6', '--save_every',
                 '7', '--comment', 'x', '--resume', 'r', '--finetune', 'f', '--workers', '3', '--port', '1234', '--synthetic',
                 '--data', 'd.npz', '--max_steps', '9', '--logdir', 'l', '--seed', '11', '--graph', '--monitor',
                 '--knn_data', 'k.npz', '--knn_k', '20', '--knn_temp', '0.5']
_SHARED_SET = {'mode': 'contrad', 'penalty': 'bcr', 'aug': 'simclr', 'use_warmup': True, 'temp': 0.2, 'lbd_a': 2.0,
               'no_fid': True, 'no_gif': True, 'n_eval_avg': 4, 'print_every': 5, 'evaluate_every': 6, 'save_every': 7,
               'comment': 'x', 'resume': 'r', 'finetune': 'f', 'workers': 3, 'port': 1234, 'synthetic': True,
               'data': 'd.npz', 'max_steps': 9, 'logdir': 'l', 'seed': 11, 'graph': True, 'monitor': True,
               'knn_data': 'k.npz', 'knn_k': 20, 'knn_temp': 0.5}


def test_the_three_command_lines_keep_every_flag_and_default():
    """Every destination and default of the three parsers, one command line per script that sets every flag, and the
    flags a script does not have."""
    from contrad_amd import train_gan, train_stylegan2
    assert vars(train_gan.parse_args(['c.gin', 'arch'])) == _GAN_DEFAULTS
    assert vars(train_stylegan2.parse_args(['c.gin', 'arch'])) == _SG2_DEFAULTS
    assert vars(train_stylegan2.parse_args(['c.gin', 'arch'], contrad_script=True)) == _SG2_DEFAULTS
    a = vars(train_gan.parse_args(['c.gin', 'arch'] + _SHARED_FLAGS + ['--world-size', '2', '--rank', '1']))
    assert a == dict(_GAN_DEFAULTS, world_size=2, rank=1, **_SHARED_SET)
    own = ['--no_lazy', '--d_reg_every', '4', '--lbd_r1', '0.5', '--style_mix', '0.5', '--halflife_k', '10',
           '--ema_start_k', '2', '--halflife_lr', '1000', '--batch_size', '8']
    own_set = {'no_lazy': True, 'd_reg_every': 4, 'lbd_r1': 0.5, 'style_mix': 0.5, 'halflife_k': 10, 'ema_start_k': 2,
               'halflife_lr': 1000, 'batch_size': 8}
    for contrad_script in (False, True):
        a = vars(train_stylegan2.parse_args(['c.gin', 'arch'] + _SHARED_FLAGS + own, contrad_script))
        assert a == dict(_SG2_DEFAULTS, **_SHARED_SET, **own_set)
        with pytest.raises(SystemExit):
            train_stylegan2.parse_args(['c.gin', 'arch', '--world-size', '1'], contrad_script)
    with pytest.raises(SystemExit):
        train_gan.parse_args(['c.gin', 'arch', '--batch_size', '8'])


def test_train_driver_pure_pieces():
    """What the driver decides on the host: the two log-directory names, the per-rank batch rule of each script, the two
    warm-up ratios, the --graph gate's log lines and the image-size table with train_gan's subset."""
    import argparse
    from contrad_amd import data, train_driver, train_gan, train_stylegan2
    # log directories
    P = argparse.Namespace(gin_stem='c10_b512', architecture='sndcgan', filename='contrad_simclr_L1.0_T0.1', comment='_x')
    assert train_gan.SCRIPT.logdir(P) == 'logs/gan/c10_b512/sndcgan/contrad_simclr_L1.0_T0.1_x'
    P = argparse.Namespace(gin_stem='c10_style64', architecture='stylegan2', filename='contrad_simclr_L1.0_T0.1',
                           comment='', lbd_r1=10, style_mix=0.9, halflife_k=20, halflife_lr=0, no_lazy=False)
    assert train_stylegan2.script(False).logdir(P) == \
        'logs/gan/st_c10_style64/stylegan2/contrad_simclr_L1.0_T0.1_R10_mix0.9_H20_Lazy'
    P.lbd_r1, P.halflife_lr, P.no_lazy, P.comment = 0.5, 2500000, True, '_runft'
    assert train_stylegan2.script(True).logdir(P) == \
        'logs/gan_dp/st_c10_style64/stylegan2/contrad_simclr_L1.0_T0.1_R0.5_mix0.9_H20_lr2.5M_NoLazy_runft'
    # per-rank batch
    o = {'batch_size': 512}
    train_driver.per_rank_batch(o, 8, train_gan.SCRIPT.divisible_batch)
    assert o == {'batch_size': 64}
    o = {'batch_size': 10}
    train_driver.per_rank_batch(o, 4, train_gan.SCRIPT.divisible_batch)
    assert o == {'batch_size': 2}                                   # train_gan floors
    with pytest.raises(ValueError):
        train_driver.per_rank_batch({'batch_size': 10}, 4, train_stylegan2.script(True).divisible_batch)
    o = {'batch_size': 64}
    train_driver.per_rank_batch(o, 8, train_stylegan2.script(False).divisible_batch)
    assert o == {'batch_size': 8, 'global_batch_size': 64}
    # warm-up ratios: (step + 1) / warmup against (step + 1) / (warmup + 1e-8)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    train_gan._update_warmup(opt, 0, 3, 2e-3)
    assert opt.param_groups[0]['lr'] == (1 / 3) * 2e-3
    train_stylegan2._update_warmup(opt, 0, 3, 2e-3)
    assert opt.param_groups[0]['lr'] == (1 / (3 + 1e-8)) * 2e-3 != (1 / 3) * 2e-3
    # --graph
    gate = lambda script, **kw: train_driver.graph_gate(argparse.Namespace(**kw), script)
    assert gate(train_gan.SCRIPT, graph=False, mode='std') == (None, None)
    assert gate(train_gan.SCRIPT, graph=True, mode='std') == \
        (None, "--graph captures the ContraD critic iteration (--mode contrad), not 'std' -> eager")
    critic, why_not = gate(train_gan.SCRIPT, graph=True, mode='contrad')
    assert isinstance(critic, train_gan.GraphedCritic) and why_not is None
    for mode in ('contrad', 'std'):
        assert gate(train_stylegan2.script(False), graph=True, mode=mode) == \
            (None, "--graph: train_stylegan2_contraD.py only (train_stylegan2.py feeds the D-step the G-step's fakes) "
                   "-> eager")
    assert gate(train_stylegan2.script(True), graph=True, mode='aug') == \
        (None, "--graph captures the ContraD D-step (--mode contrad), not 'aug' -> eager")
    critic, why_not = gate(train_stylegan2.script(True), graph=True, mode='contrad')
    assert isinstance(critic, train_stylegan2.GraphedCritic) and why_not is None
    # image sizes
    assert data.IMAGE_SIZES == {'cifar10': (32, 32, 3), 'cifar100': (32, 32, 3), 'cifar10_hflip': (32, 32, 3),
                                'cifar100_hflip': (32, 32, 3), 'celeba128': (128, 128, 3), 'afhq_cat': (512, 512, 3),
                                'afhq_dog': (512, 512, 3), 'afhq_wild': (512, 512, 3)}
    assert train_stylegan2.IMAGE_SIZES == data.IMAGE_SIZES
    assert train_gan.IMAGE_SIZES == {'cifar10': (32, 32, 3), 'cifar100': (32, 32, 3), 'cifar10_hflip': (32, 32, 3)}
    assert train_gan.SCRIPT.image_sizes is train_gan.IMAGE_SIZES and 'afhq_dog' not in train_gan.IMAGE_SIZES
