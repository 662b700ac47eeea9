"""bench.py on one GPU: a plain run times the headline workload and reports nothing else (with --dump-outputs: every
workload, whose outputs the dump holds); --full adds the side measurements (roofline, generator step) on the same line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1'] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_workload_only():
    out = _run([])
    assert out['metric'] == 'discriminator-step images/sec (ContraD, SimCLR aug)' and out['unit'] == 'images/sec'
    assert out['higher_is_better'] is True and out['dtype'] == 'f32' and out['n_gpus'] == 1
    assert out['steps'] == 2 and out['warmup'] == 1 and out['config']['name'] == 'c10_b512'
    assert out['config']['global_batch'] == 512 and out['config']['losses_finite'] and out['value'] > 0
    assert abs(out['value'] - 512 * 2 / (out['ms_per_step'] * 2e-3)) < 1e-2 * out['value']
    for side in ('roofline', 'g_step', 'cpu_baseline', 'other_configs'):
        assert side not in out, side
    assert set(out['summary']) == {'c10_b512'} and out['summary']['c10_b512']['value'] == out['value']


def test_plain_run_with_dumps_covers_every_workload(tmp_path):
    """The dump is what two builds are compared on: it holds every workload's outputs, without the side measurements."""
    out = _run(['--dump-outputs', str(tmp_path)], timeout=900)
    assert out['config']['name'] == 'c10_b512' and set(out['other_configs']) == {'sg2_32', 'sg2_512'}
    for w in [out] + list(out['other_configs'].values()):
        assert 'error' not in w and w['value'] > 0 and w['steps'] == 2 and w['config']['losses_finite'], w
        assert 'roofline' not in w and 'g_step' not in w and 'cpu_baseline' not in w
    dumped = os.listdir(tmp_path)
    assert {f.split('.')[0] for f in dumped} == {'c10_b512', 'sg2_32', 'sg2_512'}
    for name in ('c10_b512', 'sg2_32', 'sg2_512'):
        assert name + '.d_loss.npy' in dumped, name


def test_full_run_adds_roofline_and_generator_step():
    out = _run(['--full', '--config', 'c10_b512', '--no-cpu-baseline'])
    assert out['config']['name'] == 'c10_b512' and out['config']['launch'] == 'hipGraph replay' and out['value'] > 0
    assert out['roofline']['kernel'] and out['roofline']['achieved'] > 0 and out['roofline']['launches_per_step'] > 0
    assert out['g_step']['ms_per_step'] > 0 and out['g_step']['finite']
    assert 'cpu_baseline' not in out and 'other_configs' not in out
    s = out['summary']['c10_b512']
    assert s['dominant_kernel'] == out['roofline']['kernel'] and s['g_step_ms'] == out['g_step']['ms_per_step']
