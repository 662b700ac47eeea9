"""The kernels of csrc/project/project.hip on the GPU, each alone, against the yardstick (tests/project_ref64.py): whole outputs
within the derived bounds (the module's docstring derives them; nothing is fitted), bitwise equal on a second call.  Every output
and the caller-owned scratch sit in guard storage filled with a poison word of tests/ws_guard.py: a write outside breaks a
guard, an unwritten scratch word that reaches an output makes it NaN.  Every figure goes through ``margin`` (conftest.py)."""
import ctypes

import numpy as np
import pytest
import torch

import project_ref64 as R
from ws_guard import POISONS

pytestmark = pytest.mark.gpu

GUARD = 64                     # floats on either side: the view stays 256-byte aligned
EINVAL = -22


def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def _guarded(shape, poison='qnan'):
    """(view, check): a contiguous fp32 tensor of ``shape`` inside guard bands, all of it the poison word."""
    numel = int(np.prod(shape))
    flat = torch.empty((numel + 2 * GUARD,), device='cuda', dtype=torch.float32)
    word = _i32(POISONS[poison])
    flat.view(torch.int32).fill_(word)

    def check():
        torch.cuda.synchronize()
        bands = flat.view(torch.int32)
        assert bool((bands[:GUARD] == word).all()) and bool((bands[GUARD + numel:] == word).all()), 'guard band overwritten'
    return flat[GUARD:GUARD + numel].view(*shape), check


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _ratio(got, want, bound):
    """max error / bound over the elements with a positive bound; where the bound is 0 the value must be exact."""
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(np.isfinite(got))
    zero = bound == 0
    assert np.all(err[zero] == 0)
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ---- image_end ----
_images = {}


def _image_pair(size):
    if size not in _images:
        g = np.random.RandomState(size)
        _images[size] = (g.rand(3, 3, size, size).astype(np.float32), g.rand(3, 3, size, size).astype(np.float32))
    return _images[size]


LAMS = {1: (1.0,), 2: (0.75, 1.5), 4: (1.0, 0.5, 2.0, 0.25)}


def _image_end(x, t, lam):
    from contrad_amd import ops
    N, _, H, W = x.shape
    L = len(lam)
    pix, c0 = _guarded((L, N))
    gx, c1 = _guarded(x.shape)
    part, c2 = _guarded((ops.proj_image_end_partial_floats(L, N, H, W),))
    ops.proj_image_end(_dev(x), _dev(t), lam, pix=pix, gx=gx, partial=part)
    for c in (c0, c1, c2):
        c()
    return pix.clone(), gx.clone()


@pytest.mark.parametrize('L', [1, 2, 4])
@pytest.mark.parametrize('size', [8, 16, 32])
def test_image_end_against_the_yardstick(margin, size, L):
    x, t = _image_pair(size)
    lam = LAMS[L]
    pix, gx = _image_end(x, t, lam)
    want_pix, want_gx = R.image_end(x, t, lam)
    bound_pix, bound_gx = R.image_end_bounds(x, t, lam)
    rp, rg = _ratio(pix.cpu().numpy(), want_pix, bound_pix), _ratio(gx.cpu().numpy(), want_gx, bound_gx)
    print('image_end %d^2 L=%d: worst error / bound: pix %.4f, gx %.4f' % (size, L, rp, rg))
    margin('proj image_end pix size=%d L=%d' % (size, L), rp, 1.0)
    margin('proj image_end gx size=%d L=%d' % (size, L), rg, 1.0)
    pix2, gx2 = _image_end(x, t, lam)
    assert np.array_equal(_bits(pix), _bits(pix2)) and np.array_equal(_bits(gx), _bits(gx2))


def test_image_end_of_equal_images_is_exactly_zero():
    x, _ = _image_pair(32)
    pix, gx = _image_end(x, x.copy(), LAMS[4])
    assert not _bits(pix).any() and not (gx.cpu().numpy() != 0).any()


def test_image_end_refusals():
    from contrad_amd import _lib, ops
    x = torch.zeros(2, 3, 12, 12, device='cuda')
    with pytest.raises(RuntimeError, match='divisible by 8'):
        ops.proj_image_end(x, x.clone(), LAMS[4])
    with pytest.raises(ValueError):
        ops.proj_image_end(x, x.clone(), (1.0,) * 5)
    with pytest.raises(RuntimeError):
        ops.proj_image_end(x, x[:, :, :8].contiguous(), (1.0,))
    raw = _lib.lib().raw('contrad_proj_image_end')
    p, ll = ops._p, ctypes.c_longlong
    pix, gx, part = torch.empty(4, 2, device='cuda'), torch.empty_like(x), torch.empty(4096, device='cuda')
    lam = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    assert raw(p(x), p(x), lam, 4, p(pix), p(gx), p(part), ll(4096), 2, 12, 12, None) == EINVAL     # 12 is no multiple of 8
    assert raw(p(x), p(x), lam, 3, p(pix), p(gx), p(part), ll(4096), 2, 12, 12, None) == 0
    assert raw(p(x), p(x), lam, 3, p(pix), p(gx), p(part), ll(3 * 2 * 3 * 1 - 1), 2, 12, 12, None) == EINVAL
    torch.cuda.synchronize()


# ---- noise_grad ----
@pytest.mark.parametrize('shape', [(3, 5, 7, 8), (3, 5, 7, 24), (3, 5, 7, 512), (2, 32, 32, 128), (3, 5, 7, 10)])
def test_noise_grad_against_the_yardstick(margin, shape):
    from contrad_amd import ops
    g = np.random.RandomState(shape[-1])
    gp = g.randn(*shape).astype(np.float32)
    nw = np.float32(-0.37)
    d_gp, d_nw = _dev(gp), _dev(np.float32([nw]))
    outs = []
    for _ in range(2):
        out, check = _guarded((shape[0], 1, shape[1], shape[2]))
        ops.proj_noise_grad(d_gp, d_nw, out=out)
        check()
        outs.append(out.clone())
    ratio = _ratio(outs[0].cpu().numpy(), R.noise_grad(gp, nw), R.noise_grad_bound(gp, nw))
    print('noise_grad %s: worst error / bound = %.4f' % (shape, ratio))
    margin('proj noise_grad %s' % (shape,), ratio, 1.0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_noise_grad_refusals():
    from contrad_amd import ops
    g = torch.zeros(2, 4, 4, 8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.proj_noise_grad(g.permute(0, 3, 1, 2), torch.zeros(1, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_grad(g, torch.zeros(2, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_grad(g, torch.zeros(1, device='cuda'), out=torch.zeros(2, 4, 4, device='cuda'))


# ---- noise_reg ----
def _noise_reg(m, acc0, scale, poison):
    from contrad_amd import ops
    N, _, Rr, _ = m.shape
    reg, c0 = _guarded((N,), poison)
    acc, c1 = _guarded(m.shape, poison)
    acc.copy_(_dev(acc0))
    scratch, c2 = _guarded((ops.proj_noise_reg_scratch_floats(N, Rr),), poison)
    ops.proj_noise_reg(_dev(m), acc, scale, reg=reg, scratch=scratch)
    for c in (c0, c1, c2):
        c()
    return reg.clone(), acc.clone()


@pytest.mark.parametrize('N,side', [(n, r) for r in (4, 8, 16, 32, 64) for n in (1, 3)] + [(1, 512)])
def test_noise_reg_against_the_yardstick(margin, N, side):
    g = np.random.RandomState(10 * side + N)
    m = g.randn(N, 1, side, side).astype(np.float32)
    m[0] += 0.5                                                       # (a mean: the products do not average out)
    acc0 = g.randn(N, 1, side, side).astype(np.float32)
    scale = 3.5
    reg, acc = _noise_reg(m, acc0, scale, 'qnan')
    want_reg, want_grad = R.noise_reg(m)
    bound_reg, bound_acc = R.noise_reg_bounds(m, acc0, scale)
    rr = _ratio(reg.cpu().numpy(), want_reg, bound_reg)
    rg = _ratio(acc.cpu().numpy(), acc0.astype(np.float64) + scale * want_grad, bound_acc)
    print('noise_reg N=%d R=%d: worst error / bound: reg %.4f, accumulated gradient %.4f' % (N, side, rr, rg))
    margin('proj noise_reg reg N=%d R=%d' % (N, side), rr, 1.0)
    margin('proj noise_reg grad N=%d R=%d' % (N, side), rg, 1.0)
    reg2, acc2 = _noise_reg(m, acc0, scale, 'ones')                   # (another poison in scratch: nothing of it is read)
    assert np.array_equal(_bits(reg), _bits(reg2)) and np.array_equal(_bits(acc), _bits(acc2))
    # the gradient alone moves the buffer: scale 0 leaves it as it was
    _reg0, acc_same = _noise_reg(m, acc0, 0.0, 'qnan')
    assert np.array_equal(acc_same.cpu().numpy(), acc0)


def test_noise_reg_refusals():
    from contrad_amd import ops
    m = torch.zeros(2, 1, 16, 16, device='cuda')
    with pytest.raises(RuntimeError, match='power of two'):
        ops.proj_noise_reg(torch.zeros(2, 1, 12, 12, device='cuda'), torch.zeros(2, 1, 12, 12, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_reg(m, torch.zeros(2, 1, 8, 8, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_reg(m, torch.zeros_like(m), scratch=torch.zeros(8, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_reg(m, m)                                      # the gradient buffer is not the map


# ---- noise_normalize ----
def _normalize(m):
    from contrad_amd import ops
    buf, check = _guarded(m.shape)
    buf.copy_(_dev(m))
    ops.proj_noise_normalize_(buf)
    check()
    return buf.clone()


@pytest.mark.parametrize('N,side', [(n, r) for r in (4, 8, 16, 32, 64) for n in (1, 3)] + [(1, 512)])
def test_noise_normalize_against_the_yardstick(margin, N, side):
    g = np.random.RandomState(7 * side + N)
    m = (g.randn(N, 1, side, side) * 1.7 + 0.4).astype(np.float32)
    got = _normalize(m)
    ratio = _ratio(got.cpu().numpy(), R.noise_normalize(m), R.noise_normalize_bound(m))
    print('noise_normalize N=%d R=%d: worst error / bound = %.4f' % (N, side, ratio))
    margin('proj noise_normalize N=%d R=%d' % (N, side), ratio, 1.0)
    assert np.array_equal(_bits(got), _bits(_normalize(m)))
    out = got.cpu().numpy().astype(np.float64)
    assert np.abs(out.mean(axis=(1, 2, 3))).max() < 1e-5 and np.abs((out ** 2).mean(axis=(1, 2, 3)) - 1.0).max() < 1e-5


@pytest.mark.parametrize('value', [0.1, -3.0, 0.0])
def test_a_constant_map_normalises_to_zeros(value):
    m = np.full((2, 1, 16, 16), value, np.float32)
    m[1] = np.random.RandomState(1).randn(1, 16, 16)
    got = _normalize(m).cpu().numpy()
    assert not (got[0] != 0).any()                                    # the deviation of DESIGN.md 25: zeros, not a division by zero
    assert np.all(np.isfinite(got)) and abs(float((got[1].astype(np.float64) ** 2).mean()) - 1.0) < 1e-5


def test_noise_normalize_refusals():
    from contrad_amd import ops
    with pytest.raises(RuntimeError, match='power of two'):
        ops.proj_noise_normalize_(torch.zeros(2, 1, 12, 12, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_normalize_(torch.zeros(2, 3, 8, 8, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.proj_noise_normalize_(torch.zeros(2, 1, 8, 8, device='cuda', dtype=torch.float64))
