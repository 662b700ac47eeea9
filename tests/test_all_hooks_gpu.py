"""Every monitoring hook of the training scripts in ONE run (train_driver.HOOKS): the trajectory does not move by a bit,
exactly the expected csv files appear, the lines of one evaluation come in the registry's order, and a hook writes what it
writes when it runs alone -- the hooks do not disturb one another.  Sizes: the smallest the single-hook tests use."""
import os

import numpy as np
import pytest

import spectrum_ref64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKS = ('[kNN Acc@1 ', '[NT-Xent ', '[SWD x1e3 ', '[Spectrum LSD ', '[PPL z ', '[precision ', '[kid ', '[authenticity ', '[fd ')
HEADS = {'knn': 'step,acc@1', 'contrast': 'step,nt_xent,acc@1,acc@5,rank_mean,align,uniform,align_pen,uniform_pen',
         'swd': 'step,swd_32,swd_16,swd_avg', 'spectrum': 'step,lsd_db,hf_db,nyq_h,nyq_v,nyq_d', 'ppl': 'step,ppl,ppl_raw,kept',
         'prdc': 'step,precision,recall,density,coverage', 'kid': 'step,kid,kid_std', 'auth': 'step,authenticity,nearest_mean',
         'fd': 'step,fd,mean_term,trace_fake,cross_term,tail'}


def _read(logdir, name):
    with open(os.path.join(logdir, name)) as f:
        return f.read()


def test_all_hooks_in_one_run(tmp_path_factory):
    import test_knn_gpu as TK
    import test_prdc_gpu as TP
    from contrad_amd import lineval
    from contrad_amd.train_gan import main
    assert TK.SEED == TP.SEED
    plain = TP._run(tmp_path_factory, False, False)
    d = tmp_path_factory.mktemp('all_hooks_files')
    np.savez(str(d / 'held_out.npz'), x_train=lineval.synthetic_set(1, 4, 96, 1)['x_train'])      # test_contrast_stats_gpu's
    np.savez(str(d / 'smooth.npz'), x_train=spectrum_ref64.smooth_noise(64, 32, 13))                # test_spectrum_gpu's
    enc = str(TP._files(tmp_path_factory) / 'enc.pt')
    hooked = str(tmp_path_factory.mktemp('all_hooks_run'))
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
          '--seed', str(TP.SEED), '--logdir', hooked, '--monitor',
          '--knn_data', TK._tiny_npz(tmp_path_factory), '--knn_k', '20',
          '--contrast_data', str(d / 'held_out.npz'), '--contrast_n', '64',
          '--swd_data', str(d / 'smooth.npz'), '--swd_n', '48',
          '--spectrum_data', str(d / 'smooth.npz'), '--spectrum_n', '48',
          '--ppl_encoder', enc, '--ppl_n', '128'] + TP._hook_flags(tmp_path_factory, '') + ['--prdc_kid', '--prdc_auth', '--prdc_fd'])
    # the trajectory
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(hooked, name))
    # the files: each its header and the rows of steps 2 and 4
    assert sorted(f for f in os.listdir(hooked) if f.endswith('.csv')) == sorted('%s_%d.csv' % (name, TP.EVAL_SEED) for name in HEADS)
    for name, head in HEADS.items():
        lines = _read(hooked, '%s_%d.csv' % (name, TP.EVAL_SEED)).split()
        assert lines[0] == head and [ln.split(',')[0] for ln in lines[1:]] == ['2', '4'], name
    assert os.path.exists(os.path.join(hooked, 'progress_%d' % TP.EVAL_SEED, 'step_4.png'))         # --monitor ran too
    assert not [f for f in os.listdir(hooked) if '_best' in f]
    # the log: one evaluation's lines in the registry's order, PRDC's last
    for step in (2, 4):
        said = [ln for ln in _read(hooked, 'log.txt').splitlines() if ln.startswith('[Steps %7d] ' % step)]
        assert len(said) == len(MARKS) and all(mark in ln for ln, mark in zip(said, MARKS)), said
    # independence: a discriminator-side and a generator-side hook write what they write alone
    alone = TK._run(tmp_path_factory, False, True)
    name = 'knn_%d.csv' % TP.EVAL_SEED
    assert _read(hooked, name) == _read(alone, name)
    alone = TP._run(tmp_path_factory, False, 'coverage')
    name = 'prdc_%d.csv' % TP.EVAL_SEED
    assert _read(hooked, name) == _read(alone, name)
