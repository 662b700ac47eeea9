"""The float64 yardstick of the contrastive diagnostics (tests/contrast_ref64.py) against closed forms and float64 torch,
the ``-EINVAL`` cases of ``contrad_gauss_sums`` on host pointers, every host refusal of contrad_amd/contrast.py, of
``ops.gauss_sums`` and of the ``--contrast_*`` flags (raised before any GPU work), the csv header and the chance level."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import contrast_ref64 as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit_rows(seed, n, d):
    return C.normalize64(np.random.default_rng(seed).standard_normal((n, d)))


# ---- closed forms ----
def test_identical_views_align_zero_and_every_rank_zero():
    A = _unit_rows(0, 24, 6)
    assert C.alignment(A, A) <= 4 * 2.0 ** -52                           # |a|^2 = 1 to a rounding, clamped at 0 from below
    for batch in (24, 12, 11):                                          # (11: blocks of 11, 11 and 2)
        rank, margin = C.ranks(A, A, batch)
        assert rank.shape == (48,) and not rank.any() and np.isfinite(margin).all() and (margin > 0).all()
        assert C.rank_stats(rank) == {'acc@1': 1.0, 'acc@5': 1.0, 'rank_mean': 0.0}


def test_all_rows_equal_uniform_zero_and_every_rank_last():
    A = np.zeros((10, 5))
    A[:, 0] = 1.0                                                       # every dot is exactly 1
    assert C.uniformity(A, 2.0) == 0.0 and C.alignment(A, A) == 0.0
    for b in (10, 5):
        rank, _ = C.ranks(A, A, b)
        assert (rank == 2 * b - 2).all()                                # ties count against the positive
        assert C.rank_stats(rank)['acc@1'] == 0.0 and C.rank_stats(rank)['rank_mean'] == 2 * b - 2
    assert C.rank_stats(C.ranks(A[:3], A[:3], 3)[0])['acc@5'] == 1.0     # 2b - 2 = 4 < 5
    assert abs(C.nt_xent(A, A, 5, 0.1) - math.log(9.0)) <= 1e-12          # 2b - 1 equal logits


def test_two_antipodal_clusters():
    m, d = 7, 4
    A = np.zeros((2 * m, d))
    A[:m, 0], A[m:, 0] = 1.0, -1.0
    for t in (0.5, 2.0, 10.0):
        want = math.log((2 * m * (m - 1) + 2 * m * m * math.exp(-4.0 * t)) / (2 * m * (2 * m - 1.0)))
        assert abs(C.uniformity(A, t) - want) <= 1e-14
    assert C.alignment(A, A) == 0.0 and C.alignment(A, -A) == 4.0
    rank, _ = C.ranks(A, -A, 2 * m)                                      # the positive is the farthest row: every other row beats it
    assert (rank == 4 * m - 2).all()


def test_t_zero_gives_uniform_zero_and_the_pair_count():
    A = _unit_rows(1, 17, 5)
    assert C.uniformity(A, 0.0) == 0.0
    S = (A @ A.T).astype(np.float32)
    assert C.gauss_block_sum(S, 0, 0.0) == 17 * 16 and C.gauss_block_sum(S, -1, 0.0) == 17 * 17
    assert C.gauss_block_sum(S[3:9], 3, 0.0) == 6 * 16                   # a row chunk passes its first row
    assert C.gauss_block_sum(S[:, :4], 35, 0.0) == 17 * 4                # own columns beyond the bank: nothing left out


def test_the_term_its_clamp_and_the_excluded_cell():
    assert C.gauss_block_sum(np.full((3, 4), 1 + 2.0 ** -23, np.float32), -1, 2.0) == 12.0     # u < 0 becomes 0: exactly 1
    assert C.gauss_block_sum(np.full((2, 2), -1.0, np.float32), -1, 2.0) == 4 * math.exp(-8.0)
    X = np.ones((3, 4), np.float32)
    X[1, 1] = np.nan
    assert C.gauss_block_sum(X, 0, 2.0) == 9.0 and math.isfinite(C.gauss_block_bound(X, 0, 2.0))   # left out by index: never seen
    assert math.isnan(C.gauss_block_sum(X, -1, 2.0)) and math.isnan(C.gauss_block_sum(X, -1, 0.0))
    S = np.clip(np.random.RandomState(1).randn(65, 300), -1, 1).astype(np.float32)
    ref, bound = C.gauss_block_sum(S, 3, 2.0), C.gauss_block_bound(S, 3, 2.0)
    assert 0 < bound < 1e-3 * math.exp(-8.0) and bound < 1e-11 * ref     # far below one dropped cell
    half = np.full((1, 1), 0.5, np.float32)                              # u = 1: one term, (t u + 5) + (1 + 16) roundings
    assert C.gauss_block_bound(half, -1, 2.0) == 2.0 ** -53 * 24.0 * math.exp(-2.0) and C.gauss_block_bound(half, 0, 2.0) == 0.0


@pytest.mark.parametrize('n,batch,temp', [(12, 12, 0.1), (13, 5, 0.2), (20, 6, 0.07)])
def test_nt_xent_against_float64_log_softmax(n, batch, temp):
    A, B = _unit_rows(2, n, 7), _unit_rows(3, n, 7)
    total = 0.0
    for i, m in C.blocks_of(n, batch):
        Z = torch.from_numpy(np.concatenate([A[i:i + m], B[i:i + m]]))
        L = (Z @ Z.t()) / temp
        L.fill_diagonal_(-float('inf'))
        lp = torch.log_softmax(L, dim=1)
        pos = (torch.arange(2 * m) + m) % (2 * m)
        total += float(-lp[torch.arange(2 * m), pos].sum())
    assert abs(C.nt_xent(A, B, batch, temp) - total / (2 * n)) <= 1e-12
    assert C.blocks_of(13, 5) == [(0, 5), (5, 5), (10, 3)] and C.blocks_of(4, 9) == [(0, 4)]


def test_planted_views_give_ranks_that_are_not_trivial():
    """The sets of tests/test_contrast_stats_gpu.py: few rows are near-ties, and acc@1 is far from both 0 and 1."""
    for d in (8, 16):
        for n, batch in ((96, 48), (260, 130), (100, 48)):
            for seed in range(3):
                A, B = (C.normalize64(v) for v in C.planted_views(seed, n, d))
                rank, margin = C.ranks(A, B, batch)
                acc = C.rank_stats(rank)['acc@1']
                print('d %d n %d batch %d seed %d: acc@1 %.3f, rows within 1e-5 of a tie %d' % (d, n, batch, seed, acc, int((margin < 1e-5).sum())))
                assert 0.05 < acc < 0.6 and (margin < 1e-5).sum() <= 0.1 * len(rank)


# ---- contrad_gauss_sums on host pointers ----
def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


def test_entry_point_rejects_bad_arguments_before_any_gpu_call():
    """Every pointer below is host memory: a call that got past the argument check would fail differently (or launch)."""
    from contrad_amd._lib import lib
    query, f, g = lib().raw('contrad_kid_sums_workspace_bytes'), lib().raw('contrad_gauss_sums'), lib().raw('contrad_mmd_sums')
    M, n = 2, 8
    need = query(M, n)
    S, out, ws = (ctypes.c_float * (M * n))(), (ctypes.c_double * 1)(-7.0), (ctypes.c_double * (need // 8 + 1))()

    def call(S=S, ldS=n, M=M, n=n, self0=0, t=2.0, accumulate=0, out=out, ws=ws, ws_bytes=need):
        return f(_vp(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), t, accumulate, _vp(out), _vp(ws),
                 ctypes.c_longlong(ws_bytes), ctypes.c_void_p(0))

    for bad in (dict(t=-1.0), dict(t=-2.0 ** -1074), dict(t=float('nan')), dict(t=float('inf')), dict(t=-float('inf')), dict(S=None),
                dict(out=None), dict(M=0), dict(n=0), dict(M=-1), dict(ldS=n - 1), dict(ws=None), dict(ws_bytes=need - 1),
                dict(ws_bytes=0), dict(accumulate=1, out=None)):
        assert call(**bad) == -22, bad
    misaligned = ctypes.c_void_p(ctypes.addressof(ws) + 4)
    assert f(_vp(S), ctypes.c_longlong(n), M, n, ctypes.c_longlong(0), 2.0, 0, _vp(out), misaligned, ctypes.c_longlong(need),
             ctypes.c_void_p(0)) == -22
    for kind in (2, 3, 4, -1):                                          # the internal kinds stay behind their own entry points
        assert g(_vp(S), ctypes.c_longlong(n), M, n, ctypes.c_longlong(0), kind, 1.0, 1.0, 0, _vp(out), _vp(ws), ctypes.c_longlong(need),
                 ctypes.c_void_p(0)) == -22, kind
    assert out[0] == -7.0 and all(v == 0.0 for v in ws)


# ---- host refusals ----
def test_python_layer_refusals_come_before_any_gpu_work(tmp_path):
    from contrad_amd import contrast, ops
    was_initialised = torch.cuda.is_initialized()
    with pytest.raises(RuntimeError, match='CUDA float32'):
        ops.gauss_sums(torch.zeros(2, 8), 8)                           # host S
    for t in (-1.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='finite t >= 0'):
            ops.gauss_sums(torch.zeros(2, 8), 8, t)
    f = torch.zeros(8, 4)
    for args, kw, match in (((f[:1], f[:1], 4, 0.1), {}, 'at least 2 images'),
                            ((f, f, 1, 0.1), {}, 'fewer than 2 images'),
                            ((f, f, 4, 0.0), {}, 'temp must be positive'),
                            ((f, f, 4, -0.1), {}, 'temp must be positive'),
                            ((f, f, 4, float('nan')), {}, 'temp must be positive'),
                            ((f, f, 4, 0.1), dict(t=-1.0), 't must be finite'),
                            ((f, f, 4, 0.1), dict(t=float('inf')), 't must be finite'),
                            ((f, f, 4, 0.1), dict(t=float('nan')), 't must be finite'),
                            ((f, f[:7], 4, 0.1), {}, 'differ in shape'),
                            ((f, torch.zeros(8, 5), 4, 0.1), {}, 'differ in shape'),
                            ((f, f, 4, 0.1), dict(fA=f, fB=f[:, :3]), 'differ in shape'),
                            ((f, f, 4, 0.1), dict(fA=f), 'come as a pair'),
                            ((f, f, 4, 0.1), dict(fA=f[:6], fB=f[:6]), 'penultimate rows for'),
                            ((f, f, 7, 0.1), {}, 'last block of 1 image'),
                            ((torch.zeros(9, 4), torch.zeros(9, 4), 4, 0.1), {}, 'last block of 1 image')):
        with pytest.raises(ValueError, match=match):
            contrast.contrast_stats(*args, **kw)
    with pytest.raises(RuntimeError, match='CUDA float32'):
        contrast.contrast_stats(f, f, 4, 0.1)                          # valid sizes: as far as the device check
    assert contrast.check_sizes(8, 4, 0.1, 2.0) == 4 and contrast.check_sizes(8, 512, 0.1, 0.0) == 8
    # the monitor: the image size is compared before anything goes to a device
    np.savez(str(tmp_path / 'x16.npz'), x_train=np.zeros((8, 16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match='the discriminator takes'):
        contrast.ContrastMonitor(str(tmp_path), 'sndcgan', (32, 32, 3), 'cuda:0', 0, str(tmp_path / 'x16.npz'), aug=object(), batch=4, temp=0.1)
    np.savez(str(tmp_path / 'x32.npz'), x_train=np.zeros((9, 32, 32, 3), np.uint8))
    for kw, match in ((dict(batch=4), 'last block of 1 image'), (dict(batch=1), 'fewer than 2 images'), (dict(batch=4, n=1), 'at least 2 images'),
                      (dict(batch=4, n=8, t=-1.0), 't must be finite'), (dict(batch=4, n=8, temp=0.0), 'temp must be positive'),
                      (dict(n=8), 'needs the block size')):
        kw.setdefault('temp', 0.1)
        with pytest.raises(ValueError, match=match):
            contrast.ContrastMonitor(str(tmp_path), 'sndcgan', (32, 32, 3), 'cuda:0', 0, str(tmp_path / 'x32.npz'), aug=object(), **kw)
    assert not [p for p in os.listdir(str(tmp_path)) if p.endswith('.csv')]
    assert torch.cuda.is_initialized() == was_initialised


def test_csv_header_and_chance_level():
    from contrad_amd import contrast
    assert contrast.CSV_HEADER == 'step,nt_xent,acc@1,acc@5,rank_mean,align,uniform,align_pen,uniform_pen'
    assert contrast.chance_level(512) == 1.0 / 1022 and contrast.chance_level(2) == 0.5
    out = dict(zip(contrast.KEYS, (4.5, 0.25, 0.5, 17.125, 0.75, -3.5, 0.125, -1.0)))
    assert contrast.csv_row(300, out) == '300,4.500000,0.250000,0.500000,17.125000,0.750000,-3.500000,0.125000,-1.000000'
    assert C.stats64(_unit_rows(0, 12, 4), _unit_rows(1, 12, 4), 6, 0.1)['chance'] == contrast.chance_level(6) == 0.1


def test_hook_flags_parse_after_the_prdc_ones_and_leave_no_attribute(tmp_path):
    from contrad_amd import contrast, train_gan, train_stylegan2
    was_initialised = torch.cuda.is_initialized()
    for mod in (train_gan, train_stylegan2):
        Q = mod.parse_args(['cfg.gin', 'sndcgan'])
        assert not [name for name in vars(Q) if name.startswith('contrast')]        # a flag not given leaves no attribute
        H = contrast.check_hook_arguments(Q)
        assert (H.contrast_data, H.contrast_n, H.contrast_t) == (None, 2000, 2.0)
        with_flag = vars(mod.parse_args(['cfg.gin', 'sndcgan', '--contrast_data', 'x.npz', '--contrast_n', '500', '--contrast_t', '3']))
        assert {k: v for k, v in with_flag.items() if not k.startswith('contrast_')} == vars(Q)
        H = contrast.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan', '--contrast_data', 'x.npz', '--contrast_n', '500', '--contrast_t', '3']))
        assert (H.contrast_data, H.contrast_n, H.contrast_t) == ('x.npz', 500, 3.0)
        for flags, match in ((['--contrast_n', '500'], 'nothing without --contrast_data'), (['--contrast_t', '1'], 'nothing without --contrast_data'),
                             (['--contrast_data', 'x.npz', '--contrast_n', '1'], 'at least 2'),
                             (['--contrast_data', 'x.npz', '--contrast_t', '-1'], 'finite and not negative'),
                             (['--contrast_data', 'x.npz', '--contrast_t', 'nan'], 'finite and not negative')):
            with pytest.raises(ValueError, match=match):
                contrast.check_hook_arguments(mod.parse_args(['cfg.gin', 'sndcgan'] + flags))
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(buf):
        train_gan.parse_args(['--help'])
    text = buf.getvalue()
    assert 0 < text.index('--knn_data') < text.index('--prdc_fd_iter') < text.index('--contrast_data') < text.index('--contrast_t')
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    common = [gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '1', '--logdir', str(tmp_path / 'run')]
    with pytest.raises(ValueError, match='nothing without --contrast_data'):
        train_gan.main(common + ['--contrast_n', '64'])
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(str(tmp_path / 'run'))


def test_command_line_defaults():
    from contrad_amd import contrast
    P = contrast.parse_args(['run/dis.pt', 'sndcgan', '--synthetic'])
    assert (P.aug, P.temp, P.n, P.batch_size, P.t, P.seed, P.data, P.fwd_batch) == ('simclr', 0.1, 2000, None, 2.0, None, None, 500)
    P = contrast.parse_args(['run/dis.pt', 'sndcgan', '--data', 'x.npz', '--aug', 'none', '--temp', '0.2', '--n', '64', '--batch_size', '32', '--t', '3', '--seed', '5'])
    assert (P.aug, P.temp, P.n, P.batch_size, P.t, P.seed, P.data) == ('none', 0.2, 64, 32, 3.0, 5, 'x.npz')
