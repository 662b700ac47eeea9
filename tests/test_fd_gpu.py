"""The Frechet distance on the GPU against the yardstick (tests/fd_ref64.py): ``contrad_dot_sums`` alone on given operands,
``fd`` on features against float64 copies of the same rows, ``fd_of`` through a discriminator, the command line and
``--prdc_fd`` of the training scripts (which must not move a checkpoint by a bit, nor a byte of the other csv files).

Bounds.  ``contrad_dot_sums``: every product of two floats is exact in float64, so the device sum is a float64 sum of the
exact terms in some order: |out - math.fsum(terms)| <= (M n + 16) 2^-53 sum |a b| (the derivation at the head of
tests/test_kid_gpu.py: any order and a fused multiply-add lie inside it, one dropped or doubled element far outside).
``fd``: |fd_dev - fd_ref| <= TOL * s with s = mean_term + trace_real + trace_fake of the yardstick.  TOL is MEASURED, not
derived: 5 times the largest |diff| / s observed over the cases below on the MI355X (the factor covers the pool's machines
and another summation split, which move the last digits), under the cap TOL <= 1e-5 that keeps the test from hiding a defect
(ddof 0 for 1 moves s by 1 / n >= 1e-3 here; a missing centring or a lost transposition moves everything; the float32
emulation of tests/fd_ref64.py stays below 3e-7 of s, tests/test_fd_ref64_cpu.py).

Observed on the MI355X (every figure is printed before it is asserted; profiles/fd.txt):
``contrad_dot_sums`` |out - fsum| at most 5.8e-11 and at most 6.5e-6 of the bound anywhere (the aliased 4 x 70 000 block), 0
in most cases.  ``fd`` |diff| / s per case, in the order of ``fd_ref64.FEATURE_CASES``: 3.79e-8, 1.58e-8, 3.32e-8, 2.71e-8,
4.51e-8, 3.79e-8 (the real state; the swapped orientation the same), 4.31e-8 (equal sets: fd = -5.2e-8 for a true 0); through
``sndcgan`` 4.25e-9.  The largest is 4.51e-8 (d = 8192), so TOL = 5 x 4.51e-8 = 2.3e-7, a 43rd of the cap.  The largest fall of
the estimate between two steps was 5.7e-8 of the estimate (allowed: 1e-6)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import fd_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
TOL = 2.3e-7                                                               # 5 x 4.51e-8, the largest |diff| / s observed (above)
assert TOL <= R.TOL_CAP


# ---- contrad_dot_sums on given operands ----
DOT_SHAPES = [(1, 1), (3, 7), (7, 3), (65, 300), (257, 1025), (1000, 1000), (4, 70000)]
_DOT_REF = {}


def _fsum_and_bound(A, B):
    terms = (A.astype(np.float64) * B.astype(np.float64)).ravel()
    return math.fsum(terms.tolist()), (terms.size + 16) * 2.0 ** -53 * float(np.abs(terms).sum())


def _dot_inputs(shape):
    """{name: (A, B, fsum of A * B, its bound, fsum of A * A, its bound)} for a shape, made once."""
    if shape not in _DOT_REF:
        M, n = shape
        r = np.random.RandomState(0)
        data = {'randn': (np.clip(r.randn(M, n), -1, 1).astype(np.float32), np.clip(r.randn(M, n), -1, 1).astype(np.float32)),
                'equal': (np.full((M, n), 0.25, np.float32), np.full((M, n), -0.75, np.float32))}
        _DOT_REF[shape] = {name: (A, B) + _fsum_and_bound(A, B) + _fsum_and_bound(A, A) for name, (A, B) in data.items()}
    return _DOT_REF[shape]


def _device_operand(S, pad, off):
    """S on the device with ``pad`` columns of NaN behind every row (a padding column that is read shows) and its base
    ``off`` floats past an allocation: off = 1 is not 16-byte aligned.  Returns (the allocation, the [M][n + pad] view)."""
    M, n = S.shape
    ld = n + pad
    flat = torch.full((off + M * ld + 8,), float('nan'), device='cuda')
    view = flat[off:off + M * ld].view(M, ld)
    view[:, :n] = torch.from_numpy(S).cuda()
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return flat, view


def _raw_dot(A, B, M, n, accumulate=False, out=None, row0=0):
    """contrad_dot_sums on rows [row0, row0 + M) of the views with guard bands around ``out`` and around a workspace of
    exactly the size the query names.  Returns (the float64 result, the guarded out buffer)."""
    from contrad_amd import ops
    from contrad_amd._lib import lib
    if out is None:
        out = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    nbytes = lib().raw('contrad_kid_sums_workspace_bytes')(M, n)
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
    rc = lib().raw('contrad_dot_sums')(ops._p(A[row0:row0 + M]), ctypes.c_longlong(A.stride(0)), ops._p(B[row0:row0 + M]),
                                       ctypes.c_longlong(B.stride(0)), M, n, 1 if accumulate else 0, ops._p(out[GUARD:]),
                                       ops._p(ws[GUARD:]), ctypes.c_longlong(nbytes), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf in (out, ws):
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all()), 'guard band overwritten'
    return float(out[GUARD]), out


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize('offs', [(0, 0), (1, 1), (1, 0)], ids=['aligned', 'base+4B', 'A+4B'])
@pytest.mark.parametrize('pads', [(0, 0), (3, 0), (0, 3), (3, 3)], ids=['dense', 'ldA+3', 'ldB+3', 'ld+3'])
@pytest.mark.parametrize('shape', DOT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dot_sums_on_given_operands(shape, pads, offs):
    M, n = shape
    for name, (A, B, ref, bound, ref_sq, bound_sq) in _dot_inputs(shape).items():
        tag = 'dot sums %dx%d %s ld+%d,%d base+%d,%d' % (M, n, name, pads[0], pads[1], offs[0], offs[1])
        _, va = _device_operand(A, pads[0], offs[0])
        _, vb = _device_operand(B, pads[1], offs[1])
        got, _ = _raw_dot(va, vb, M, n)
        print('%s: device %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (tag, got, ref, abs(got - ref), bound))
        assert abs(got - ref) <= bound, tag
        again, _ = _raw_dot(va, vb, M, n)
        assert _bits(got) == _bits(again), tag + ': two calls differ'
        swapped, _ = _raw_dot(vb, va, M, n)
        assert _bits(got) == _bits(swapped), tag + ': the operands do not commute'           # (exact products, one order)
        sq, _ = _raw_dot(va, va, M, n)                                  # B aliases A: the sum of squares
        print('%s: aliased %.17g  fsum %.17g  |diff| %.3g  bound %.3g' % (tag, sq, ref_sq, abs(sq - ref_sq), bound_sq))
        assert abs(sq - ref_sq) <= bound_sq and sq >= 0.0, tag + ': aliased'
        X = A.copy()
        X[M // 2, n // 2] = np.nan                                      # a NaN inside either block propagates
        assert math.isnan(_raw_dot(_device_operand(X, pads[0], offs[0])[1], vb, M, n)[0]), tag + ': a NaN inside the block was lost'
        if M >= 2:                                                      # two row chunks, the second accumulates
            m1 = (M + 1) // 2 if M < 200 else 129                       # (129: one row past eight 16-row tiles)
            (r1, b1), (_, b2) = _fsum_and_bound(A[:m1], B[:m1]), _fsum_and_bound(A[m1:], B[m1:])
            first, out = _raw_dot(va, vb, m1, n)
            assert abs(first - r1) <= b1, tag + ': first chunk'
            both, _ = _raw_dot(va, vb, M - m1, n, accumulate=True, out=out, row0=m1)
            print('%s: chunked %.17g  |chunked - one call| %.3g  bounds %.3g + %.3g' % (tag, both, abs(both - got), b1, b2))
            assert abs(both - got) <= b1 + b2 and abs(both - ref) <= b1 + b2, tag + ': chunked'
            out2 = torch.full((1 + 2 * GUARD,), -7.0, dtype=torch.float64, device='cuda')
            _raw_dot(va, vb, m1, n, out=out2)
            again, _ = _raw_dot(va, vb, M - m1, n, accumulate=True, out=out2, row0=m1)
            assert _bits(both) == _bits(again), tag + ': two chunked runs differ'


def test_dot_sums_wrapper_equals_the_entry_point_and_checks_its_arguments():
    from contrad_amd import ops
    A, B, ref, bound, ref_sq, bound_sq = _dot_inputs((65, 300))['randn']
    A_dev, B_dev = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    wide = torch.full((65, 304), float('nan'), device='cuda')
    wide[:, :300] = B_dev
    raw, _ = _raw_dot(A_dev, B_dev, 65, 300)
    for Y in (B_dev, wide):                                             # a row view of a wider matrix: only n columns are read
        out = ops.dot_sums(A_dev, Y, 300)
        assert out.dtype == torch.float64 and tuple(out.shape) == (1,) and _bits(float(out)) == _bits(raw)
    assert abs(float(ops.dot_sums(A_dev, A_dev, 300)) - ref_sq) <= bound_sq
    table = torch.zeros(2, 3, dtype=torch.float64, device='cuda')
    assert ops.dot_sums(A_dev[:33], B_dev[:33], 300, out=table[1, 1:2]).data_ptr() == table[1, 1:2].data_ptr()
    ops.dot_sums(A_dev[33:], B_dev[33:], 300, out=table[1, 1:2], accumulate=True)
    assert abs(float(table[1, 1]) - ref) <= bound and float(table.abs().sum()) == abs(float(table[1, 1]))
    out = torch.full((1,), 1e6, dtype=torch.float64, device='cuda')      # accumulate adds to what is there
    ops.dot_sums(A_dev, B_dev, 300, out=out, accumulate=True)
    assert abs(float(out) - (1e6 + ref)) <= bound + 2.0 ** -53 * 2e6
    for bad in (dict(n=301), dict(n=0), dict(accumulate=True), dict(out=torch.zeros(1, device='cuda')),
                dict(out=torch.zeros(2, dtype=torch.float64, device='cuda')), dict(out=torch.zeros(1, dtype=torch.float64)),
                dict(B=B_dev[:64]), dict(B=B_dev[:, :299]), dict(B=B_dev.double()), dict(B=B_dev.cpu()), dict(B=None)):
        a = dict(B=B_dev, n=300); a.update(bad)
        with pytest.raises(RuntimeError):
            ops.dot_sums(A_dev, **a)
    # the kinds of the one-operand entry points are what they were, bit for bit, next to the new one
    import kid_ref64 as K
    S = np.clip(np.random.RandomState(1).randn(65, 300), -1, 1).astype(np.float32)
    S_dev = torch.from_numpy(S).cuda()
    assert abs(float(ops.kid_sums(S_dev, 300, self0=3)) - K.block_sum(S, 3)) <= K.block_bound(S, 3)
    assert _bits(float(ops.kid_sums(S_dev, 300, self0=3))) == _bits(float(ops.mmd_sums(S_dev, 300, 'poly3', self0=3)))
    for kind in (2, 3, 'dot'):
        with pytest.raises(RuntimeError):
            ops.mmd_sums(S_dev, 300, kind)


def test_dot_sums_returns_einval_on_device_pointers():
    from contrad_amd import ops
    from contrad_amd._lib import lib
    f, g, query = lib().raw('contrad_dot_sums'), lib().raw('contrad_mmd_sums'), lib().raw('contrad_kid_sums_workspace_bytes')
    A, B = torch.zeros(2, 8, device='cuda'), torch.zeros(2, 8, device='cuda')
    out = torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
    need = query(2, 8)
    ws = torch.full((need // 8 + 1,), -7.0, dtype=torch.float64, device='cuda')
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    for a in (dict(A=None), dict(B=None), dict(out=None), dict(M=0), dict(n=0), dict(ldA=7), dict(ldB=7), dict(ws=None),
              dict(ws_bytes=need - 1), dict(ws=off4(ws)), dict(out=off4(out))):
        b = dict(A=A, ldA=8, B=B, ldB=8, M=2, n=8, out=out, ws=ws, ws_bytes=need); b.update(a)
        p = lambda t: t if isinstance(t, ctypes.c_void_p) else ops._p(t)
        assert f(p(b['A']), ctypes.c_longlong(b['ldA']), p(b['B']), ctypes.c_longlong(b['ldB']), b['M'], b['n'], 0, p(b['out']),
                 p(b['ws']), ctypes.c_longlong(b['ws_bytes']), ops._stream()) == -22, a
    for kind in (2, 3):
        assert g(ops._p(A), ctypes.c_longlong(8), 2, 8, ctypes.c_longlong(-1), kind, 1.0, 1.0, 0, ops._p(out), ops._p(ws),
                 ctypes.c_longlong(need), ops._stream()) == -22
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())


# ---- fd against the yardstick on float64 copies of the same rows ----
_FD_REF = {}


def _case(case):
    """(real, fake) float32 numpy rows, their device copies and the float64 yardstick, made once per case."""
    if case not in _FD_REF:
        real, fake = R.sets(case)
        _FD_REF[case] = (real, fake, torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), R.fd_ref64(real, fake))
    return _FD_REF[case]


def _report(tag, got, ref):
    s = ref['scale']
    print('%s: device fd %.12g  float64 %.12g  |diff| %.3g = %.3g of s = %.6g  (tolerance %.3g of s)  terms: means %.3g  tr real %.3g  '
          'tr fake %.3g  cross %.3g of s  tail %.3g of the estimate' % (
              tag, got['fd'], ref['fd'], abs(got['fd'] - ref['fd']), abs(got['fd'] - ref['fd']) / s, s, TOL,
              abs(got['mean_term'] - ref['mean_term']) / s, abs(got['trace_real'] - ref['trace_real']) / s,
              abs(got['trace_fake'] - ref['trace_fake']) / s, abs(got['cross_term'] - ref['cross_term']) / s,
              got['tail'] / got['estimates'][-1] if got['estimates'][-1] else 0.0))
    est = np.asarray(got['estimates'])
    if len(est) > 1:
        print('%s: largest fall of the estimate between two steps %.3g of the last (allowed 1e-6)' % (tag, max(0.0, -np.diff(est).min()) / est[-1]))


def _check(tag, got, ref, n_r, n_f, d, n_iter=60):
    _report(tag, got, ref)
    s = ref['scale']
    assert sorted(got) == sorted(['fd', 'mean_term', 'trace_real', 'trace_fake', 'cross_term', 'n_iter', 'estimates', 'tail', 'n_real',
                                  'n_fake', 'dim', 'note']), tag
    assert (got['n_iter'], got['n_real'], got['n_fake'], got['dim'], len(got['estimates'])) == (n_iter, n_r, n_f, d, n_iter)
    assert abs(got['fd'] - ref['fd']) <= TOL * s, tag
    for name in ('mean_term', 'trace_real', 'trace_fake', 'cross_term'):
        assert abs(got[name] - ref[name]) <= TOL * s, (tag, name)
    est = np.asarray(got['estimates'])
    assert np.all(np.isfinite(est)) and np.diff(est).min(initial=0.0) >= -1e-6 * est[-1], tag + ': the estimates fall'
    assert got['tail'] == (est[-1] - est[-6] if n_iter >= 6 else 0.0)
    assert got['fd'] == got['mean_term'] + got['trace_real'] + got['trace_fake'] - 2.0 * got['cross_term']
    assert 'never with Inception-based FID' in got['note']


@pytest.mark.parametrize('case', R.FEATURE_CASES, ids=lambda c: 'd%d-%dx%d-%s' % c)
def test_fd_on_features_against_float64(case):
    from contrad_amd import fd, features
    d, n_r, n_f, kind = case
    _, _, Rd, Fd, ref = _case(case)
    tag = 'fd features d%d %dx%d %s' % case
    if kind == 'state':                                                 # the hook's form of the real set: its bank, centred once
        Rn, Fn = features.normalize_rows(Rd), features.normalize_rows(Fd)
        state = fd.real_state_of(features.bank_of(Rn), n_r)
        got = fd.fd(None, Fn, normalize=False, real_state=state)
        _check(tag, got, ref, n_r, n_f, d)
        assert fd.fd(None, Fn, normalize=False, real_state=state) == got                        # the state is not consumed
        assert bool((state.bankT[:, n_r:] == 0).all())
        # the other orientation (the banked set is the smaller one): the distance is symmetric in its two sets
        swapped = fd.fd(None, Rn, normalize=False, real_state=fd.real_state_of(features.bank_of(Fn), n_f))
        _report(tag + ' swapped', swapped, dict(ref, trace_real=ref['trace_fake'], trace_fake=ref['trace_real']))
        assert abs(swapped['fd'] - ref['fd']) <= TOL * ref['scale'] and abs(swapped['trace_real'] - ref['trace_fake']) <= TOL * ref['scale']
        return
    got = fd.fd(Rd, Fd)
    _check(tag, got, ref, n_r, n_f, d)
    if kind == 'equal':
        assert got['mean_term'] == 0.0 and got['trace_real'] == got['trace_fake']
    else:
        assert got['fd'] >= R.MIN_FD * ref['scale'] / 2                 # the check is not empty (tests/test_fd_ref64_cpu.py: the float64 side)
    assert fd.fd(Rd, Fd) == got                                         # two calls: the same dict, bit for bit
    if d <= 512:
        pre = fd.fd(features.normalize_rows(Rd), features.normalize_rows(Fd), normalize=False)
        assert pre == got


def test_fewer_steps_give_a_smaller_estimate_and_row_chunks_the_same_distance(monkeypatch):
    from contrad_amd import fd, features
    case = R.FEATURE_CASES[0]
    d, n_r, n_f, _ = case
    _, _, Rd, Fd, ref = _case(case)
    full = fd.fd(Rd, Fd)
    few = fd.fd(Rd, Fd, n_iter=5)
    assert few['n_iter'] == 5 and few['tail'] == 0.0 and few['estimates'] == full['estimates'][:5]      # the same path, cut short
    assert few['cross_term'] < full['cross_term'] and few['fd'] > full['fd']                           # from below
    assert fd.fd(Rd, Fd, n_iter=1)['n_iter'] == 1
    monkeypatch.setattr(features, 'MAX_CHUNK_ROWS', 32)                 # every GEMM in chunks of 32 rows
    assert features.chunk_rows_of(260) == 32
    chunked = fd.fd(Rd, Fd)
    _check('fd in chunks of 32 rows', chunked, ref, n_r, n_f, d)


def test_host_refusals_on_device_tensors():
    from contrad_amd import fd
    _, _, Rd, Fd, _ = _case(R.FEATURE_CASES[0])
    for bad in (dict(n_iter=0), dict(n_iter=-1)):
        with pytest.raises(ValueError):
            fd.fd(Rd, Fd, **bad)
    with pytest.raises(ValueError):
        fd.fd(Rd[:1], Fd)
    with pytest.raises(ValueError):
        fd.fd(Rd, Fd[:1])
    with pytest.raises(RuntimeError):
        fd.fd(Rd, Fd[:, :8].contiguous())                               # widths differ
    with pytest.raises(RuntimeError):
        fd.fd(Rd.cpu(), Fd)
    with pytest.raises(RuntimeError):
        fd.fd(None, Fd, real_state=fd.real_state_of(torch.zeros(8, 300, device='cuda'), 300))       # a bank of another width


# ---- through a discriminator ----
def test_fd_of_through_sndcgan_equals_the_yardstick_on_the_device_features():
    from contrad_amd import fd
    from contrad_amd.features import extract_features
    import test_prdc_gpu as TP
    g = torch.Generator().manual_seed(11)
    real_u8 = torch.randint(0, 256, (64, 32, 32, 3), generator=g, dtype=torch.uint8).cuda()
    fake_u8 = torch.randint(0, 256, (48, 32, 32, 3), generator=g, dtype=torch.uint8).cuda()
    _, D = TP._encoder()
    D = D.cuda()
    for p in D.parameters():
        p.requires_grad_(False)
    with torch.no_grad():                                               # one train-mode forward: the power iteration a checkpoint has behind it
        D.train()(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda())
    D.eval()
    got = fd.fd_of(D, real_u8, fake_u8, batch=20)
    fr, ff = extract_features(D, real_u8, 20), extract_features(D, fake_u8, 20)
    ref = R.fd_ref64(fr.cpu().numpy(), ff.cpu().numpy(), normalize=False)          # the device's own (normalised) features, in float64
    _check('fd_of sndcgan', got, ref, 64, 48, D.d_penul)
    assert fd.fd_of(D, real_u8, fake_u8, n_iter=7, batch=64)['n_iter'] == 7
    with pytest.raises(ValueError):
        fd.fd_of(D, real_u8, fake_u8[:, :16, :16].contiguous())
    with pytest.raises(ValueError):
        fd.fd_of(D, real_u8[:0], fake_u8)
    with pytest.raises(ValueError):
        fd.fd_of(D, real_u8, fake_u8[:1])
    with pytest.raises(ValueError):
        fd.fd_of(D, real_u8, fake_u8, n_iter=0)
    with pytest.raises(RuntimeError):
        fd.fd_of(D.train(), real_u8, fake_u8)


# ---- scripts (the encoder, the real set and the plain run are those of tests/test_prdc_gpu.py) ----
KEYS = ['fd', 'mean_term', 'trace_real', 'trace_fake', 'cross_term', 'n_iter', 'estimates', 'tail', 'n_real', 'n_fake', 'dim', 'note']


def test_command_line_writes_the_json(tmp_path_factory, tmp_path):
    import shutil
    import test_fd
    import test_prdc_gpu as TP
    d = TP._files(tmp_path_factory)
    gen = str(tmp_path / 'gen.pt')
    shutil.copy(os.path.join(TP._run(tmp_path_factory, False, False), 'gen.pt'), gen)
    os.makedirs(str(tmp_path / 'samples'))
    TP._sampled_reals([gen], 'sndcgan', 96, str(tmp_path / 'x.npz'), seed=777)
    with np.load(str(tmp_path / 'x.npz')) as z:
        np.savez(str(tmp_path / 'samples' / 'samples.npz'), images=z['x_train'])
    common = [str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz')]
    path = test_fd.main(common + ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--seed', '3', '--n_fake', '80', '--n_iter', '40'])
    assert path == str(tmp_path / 'samples' / 'fd_3.json')
    with open(path) as f:
        out = json.load(f)
    assert sorted(out) == sorted(KEYS)
    assert (out['n_real'], out['n_fake'], out['n_iter'], out['dim'], len(out['estimates'])) == (256, 80, 40, 8192, 40)
    assert math.isfinite(out['fd']) and out['trace_real'] > 0 and out['trace_fake'] > 0 and 'never with Inception-based FID' in out['note']
    assert out['fd'] == out['mean_term'] + out['trace_real'] + out['trace_fake'] - 2.0 * out['cross_term']
    path = test_fd.main(common + ['--gen', gen, '--seed', '3', '--n_fake', '64', '--n_real', '200'])
    assert path == str(tmp_path / 'fd_3.json')
    with open(path) as f:
        out = json.load(f)
    assert (out['n_real'], out['n_fake'], out['n_iter']) == (200, 64, 60)
    np.savez(str(tmp_path / 'small.npz'), images=np.zeros((8, 16, 16, 3), np.uint8))
    for bad in (['--fake', str(tmp_path / 'small.npz')],                                   # 16 x 16 fakes, 32 x 32 reals
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_fake', '1'],       # no covariance of one row
                ['--fake', str(tmp_path / 'samples' / 'samples.npz'), '--n_real', '1'],
                ['--gen', gen, '--n_iter', '0']):
        with pytest.raises(ValueError):
            test_fd.main(common + bad)


def test_hook_appends_the_distance_and_leaves_everything_else_alone(tmp_path_factory):
    import test_fd
    import test_prdc_gpu as TP
    from contrad_amd.train_gan import main
    plain = TP._run(tmp_path_factory, False, False)
    d = TP._files(tmp_path_factory)
    gin = os.path.join(ROOT, 'configs', 'gan', 'cifar10', 'c10_b64.gin')
    runs = {}
    for name, extra in (('others', []), ('fd', ['--prdc_fd', '--prdc_fd_iter', '40'])):
        runs[name] = str(tmp_path_factory.mktemp('fd_run_' + name))
        main([gin, 'sndcgan', '--mode=contrad', '--aug=simclr', '--synthetic', '--max_steps', '4', '--evaluate_every', '2', '--save_every', '2',
              '--seed', str(TP.SEED), '--logdir', runs[name]] + TP._hook_flags(tmp_path_factory, None) + ['--prdc_kid', '--prdc_auth'] + extra)
    for name in ('gen.pt', 'dis.pt', 'optim.pt', 'gen_2.pt', 'dis_2.pt'):
        TP._same_files(os.path.join(plain, name), os.path.join(runs['fd'], name))
    csvs = sorted(f for f in os.listdir(runs['others']) if f.endswith('.csv'))
    assert csvs == sorted(['prdc_%d.csv' % TP.EVAL_SEED, 'kid_%d.csv' % TP.EVAL_SEED, 'auth_%d.csv' % TP.EVAL_SEED])
    for name in csvs:                                                   # byte for byte the rows of a run without the flag
        with open(os.path.join(runs['others'], name), 'rb') as a, open(os.path.join(runs['fd'], name), 'rb') as b:
            assert a.read() == b.read(), name
    assert sorted(f for f in os.listdir(runs['fd']) if f.endswith('.csv')) == sorted(csvs + ['fd_%d.csv' % TP.EVAL_SEED])
    assert not [f for f in os.listdir(runs['fd']) if '_best' in f]      # it records only
    with open(os.path.join(runs['fd'], 'fd_%d.csv' % TP.EVAL_SEED)) as f:
        lines = f.read().split()
    print('fd rows: %s' % lines)
    assert lines[0] == 'step,fd,mean_term,trace_fake,cross_term,tail' and len(lines) == 3
    rows = [ln.split(',') for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == [2, 4] and all(math.isfinite(float(v)) for r in rows for v in r[1:])
    with open(os.path.join(runs['fd'], 'log.txt')) as f:
        log = f.read()
    assert all('[fd %s]' % r[1] in log for r in rows)
    # the logged figures are the checkpoint's: the command line on the saved generator, with the eval seed, gives the last row
    path = test_fd.main([str(d / 'enc.pt'), 'sndcgan', '--real', str(d / 'real.npz'), '--gen', os.path.join(runs['fd'], 'gen.pt'),
                         '--seed', str(TP.EVAL_SEED), '--n_fake', str(TP.N_FAKE), '--n_iter', '40'])
    with open(path) as f:
        out = json.load(f)
    s = out['mean_term'] + out['trace_real'] + out['trace_fake']
    print('fd of the last row %s, of the command line %.6f' % (rows[-1][1], out['fd']))
    assert abs(float(rows[-1][1]) - out['fd']) <= 2 * TOL * s + 1e-6    # (the hook centres the bank, the command line the rows)
