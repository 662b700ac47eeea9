"""The yardstick of the latent-space tools against closed forms, and the refusals that need no device.  No GPU.

* the oracle's slerp has unit norm to 1e-14, its angle from a^ is t theta to 1e-12, t = 0 gives a^ and t = 1 gives b^, b = +-a
  gives a^ for every t;
* the percentile rule on hand-worked lists: of 201 values the two smallest and the two largest are dropped, of 200 one each
  (index floor(1.99) = 1 is kept);
* ``latent.pairs`` refuses ``space='w'`` for SNDCGAN; the command lines refuse ``--eps <= 0``, ``--n < 100`` and truncation on an
  architecture without W before any device is opened (a ValueError, not the RuntimeError of a missing GPU).
"""
import numpy as np
import pytest
import torch

import latent_ref64 as R


def _rows(n, d, seed):
    g = np.random.RandomState(seed)
    return g.randn(n, d), g.randn(n, d)


@pytest.mark.parametrize('d', [2, 3, 128, 512])
def test_slerp_is_a_unit_vector_at_the_angle_t_theta(d):
    a, b = _rows(16, d, d)
    ah, bh = R.normalize(a), R.normalize(b)
    theta = np.arctan2(np.linalg.norm(bh - np.sum(ah * bh, 1, keepdims=True) * ah, axis=1), np.sum(ah * bh, 1))
    for t in (0.0, 0.25, 0.5, 1.0, 1.0 + 1e-4):
        p = R.slerp(a, b, np.full(16, t))
        assert np.abs(np.linalg.norm(p, axis=1) - 1.0).max() <= 1e-14
        along = np.sum(p * ah, 1)
        across = np.linalg.norm(p - along[:, None] * ah, axis=1)
        assert np.abs(np.arctan2(across, along) - t * theta).max() <= 1e-12, t
    assert np.abs(R.slerp(a, b, np.zeros(16)) - ah).max() <= 1e-15
    assert np.abs(R.slerp(a, b, np.ones(16)) - bh).max() <= 1e-14


def test_slerp_of_parallel_and_antiparallel_rows_is_the_start():
    a, _ = _rows(8, 512, 1)
    a32 = a.astype(np.float32).astype(np.float64)
    for b in (a32, -a32, 3.0 * a32, -0.5 * a32):
        for t in (0.0, 0.3, 1.0):
            assert np.array_equal(R.slerp(a32, b, np.full(8, t)), R.normalize(a32))
    near = a32 * (1.0 + 1e-6 * np.random.RandomState(2).randn(8, 512))            # close, but a direction of its own
    ah, c, theta, deg = R.slerp_parts(a32, near)
    assert not deg.any() and np.all(theta > 1e-7) and np.abs(np.sum(ah * c, 1)).max() <= 1e-9
    assert np.abs(R.slerp(a32, near, np.ones(8)) - R.normalize(near)).max() <= 1e-14
    zero = np.zeros((1, 4))
    assert np.array_equal(R.normalize(zero), zero)


def test_pair_forms_t_plus_dt_in_float64():
    a, b = _rows(4, 6, 3)
    t = np.float32([0.1, 0.5, 0.9, 1.0])
    p0, p1 = R.pair(a, b, t, 1e-4, 0)
    t64 = t.astype(np.float64)
    assert np.array_equal(p0, a + t64[:, None] * (b - a)) and np.array_equal(p1, a + (t64 + 1e-4)[:, None] * (b - a))
    q0, q1 = R.pair(a, b, t, 0.0, 1)
    assert np.array_equal(q0, q1)


def test_percentile_rule_on_a_hand_worked_list():
    """np.percentile(d, 1, 'lower') of m sorted values is the one at index floor(0.01 (m - 1)), and (d, 99, 'higher') the one at
    index ceil(0.99 (m - 1)); both are kept (lo <= d <= hi).  By hand: m = 201 gives indices 2 and 198, so the two smallest and
    the two largest are dropped; m = 200 gives floor(1.99) = 1 and ceil(197.01) = 198, so one on each side is."""
    d201 = np.arange(1.0, 202.0)                                   # 1 ... 201
    d201[0], d201[1], d201[199], d201[200] = -50.0, 0.5, 1000.0, 5000.0
    kept_mean, raw, kept = R.percentile_mean(d201[np.random.RandomState(1).permutation(201)])
    assert kept == 197 and kept_mean == pytest.approx(sum(range(3, 200)) / 197.0, abs=1e-12)          # 3 ... 199
    assert raw == pytest.approx(d201.sum() / 201.0, abs=1e-9)
    d = np.arange(1.0, 201.0)                                      # 1 ... 200
    d[0], d[1], d[198], d[199] = -50.0, 0.5, 1000.0, 5000.0
    g = np.random.RandomState(0)
    shuffled = d[g.permutation(200)]
    kept_mean, raw, kept = R.percentile_mean(shuffled)
    assert kept == 198
    assert kept_mean == pytest.approx((0.5 + sum(range(3, 199)) + 1000.0) / 198.0, abs=1e-12)
    assert raw == pytest.approx(d.sum() / 200.0, abs=1e-9)
    from contrad_amd import latent
    keep, lo, hi = latent.percentile_filter(shuffled)
    assert (lo, hi, int(keep.sum())) == (0.5, 1000.0, 198)
    out = latent.summarise(shuffled, 1e-4, 'z', 'full', 7)
    assert out['ppl'] == kept_mean and out['ppl_raw'] == raw and out['kept'] == 198 and out['n'] == 200
    assert sorted(out) == sorted(['ppl', 'ppl_raw', 'kept', 'n', 'eps', 'space', 'sampling', 'seed', 'note'])
    assert 'LPIPS' in out['note'] and 'encoder' in out['note']
    bad = shuffled.copy()
    bad[5] = np.inf
    out = latent.summarise(bad, 1e-4, 'z', 'full', 7)
    assert np.isnan(out['ppl']) and np.isnan(out['ppl_raw']) and out['kept'] == 0


def test_pair_dist_yardstick_closed_forms():
    e0, e1 = np.float32([[1, 0, 0, 0]]), np.float32([[0, 2, 0, 0]])
    assert R.pair_dist(e0, e1)[0] == 2.0 and R.pair_dist(e0, e0)[0] == 0.0
    assert R.pair_dist(np.zeros((1, 4), np.float32), e1, 3.0)[0] == 3.0
    assert R.pair_dist(e0, -e0, 0.5)[0] == 2.0


def test_pairs_refuses_w_for_sndcgan():
    from contrad_amd import latent
    from contrad_amd.models.gan import get_architecture
    G = get_architecture('sndcgan', (32, 32, 3))[0]
    with pytest.raises(ValueError, match='no W'):
        latent.pairs(G, 8, 0, space='w')
    with pytest.raises(ValueError, match='no W'):
        latent.truncated(G, torch.zeros(2, 128), 0.5, None)
    with pytest.raises(ValueError, match='no W'):
        latent.mixed(G, torch.zeros(2, 128), torch.zeros(2, 128), 1)
    with pytest.raises(ValueError):
        latent.pairs(G, 8, 0, space='x')


def test_command_lines_refuse_without_a_device(tmp_path):
    import test_gan_sample  # noqa: F401  (the entry scripts import)
    import test_gan_walk  # noqa: F401
    import test_ppl  # noqa: F401
    from contrad_amd import latent, sample
    gen, enc = str(tmp_path / 'gen.pt'), str(tmp_path / 'dis.pt')
    ppl = [gen, 'sndcgan', '--encoder', enc]
    for bad in (['--eps', '0'], ['--eps=-1e-4'], ['--n', '99'], ['--space', 'w'], ['--batch_size', '0']):
        with pytest.raises(ValueError):
            latent.ppl_main(ppl + bad)
    with pytest.raises(ValueError, match='no W'):
        sample.main([gen, 'sndcgan', '--truncation', '0.7'])
    with pytest.raises(ValueError, match='no W'):
        latent.walk_main([gen, 'snresnet18', '--truncation', '0.7'])
    with pytest.raises(ValueError, match='no W'):
        latent.walk_main([gen, 'sndcgan', '--mix'])
    with pytest.raises(ValueError):
        sample.main([gen, 'stylegan2', '--truncation', '0.7', '--truncation_n', '0'])
    with pytest.raises(ValueError):
        latent.walk_main([gen, 'stylegan2', '--steps', '1'])


def test_hook_flags_refuse_without_a_device():
    from argparse import Namespace
    from contrad_amd import latent
    assert latent.check_hook_arguments(Namespace(architecture='sndcgan')).ppl_encoder is None
    H = latent.check_hook_arguments(Namespace(architecture='sndcgan', ppl_encoder='e.pt'))
    assert (H.ppl_n, H.ppl_space, H.ppl_encoder_arch) == (2000, 'z', None)
    for bad in (dict(ppl_n=500), dict(ppl_space='w'), dict(ppl_encoder='e.pt', ppl_n=99), dict(ppl_encoder='e.pt', ppl_space='w')):
        with pytest.raises(ValueError):
            latent.check_hook_arguments(Namespace(architecture='sndcgan', **bad))
    assert latent.check_hook_arguments(Namespace(architecture='stylegan2', ppl_encoder='e.pt', ppl_space='w')).ppl_space == 'w'
