"""GPU parity of the gradient-penalty kernels (csrc/gp.hip: contrad_gp_interpolate, contrad_gp_penalty) against float64
(tests/gp_ref64.py), over every launch form.

The rule of tests/test_baselines_gpu.py: operands live in NaN-filled guard storage (every sentinel must survive, an over-read
shows up as a NaN), the max-norm error max|e| / max|ref| stays below the 1e-3 contract and, with the rel-L2 error, below a
per-family bound of 5x the worst seen on an MI355X (FAMILY_TOL, recorded through ``margin``).  What is exact is compared
bitwise: interpolated rows with alpha 0 / 1, the cotangent of an all-zero row, and two calls on the same inputs.
"""
import math

import pytest
import torch

import gp_ref64 as R
from contrad_amd import ops

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
LBD = 10.0

FAMILY_TOL = {                  # family: (max-norm, rel-L2) = 5x the observed worst on an MI355X (max-norm, rel-L2)
    'gp_interp': (3.7e-7, 1.7e-7),              # 7.26e-8, 3.25e-8
    'gp_penalty_fwd': (4.7e-7, 4.7e-7),         # 9.33e-8, 9.33e-8  (value and norms)
    'gp_penalty_cot': (6.3e-7, 4.4e-7),         # 1.26e-7, 8.63e-8
}

# (N, C, H, W): the LDS form at the workload's image; fewer elements than threads; more images than one round of workgroups
# on a small grid; the two-launch form (image > 16 KiB); C*H*W = 35: rows start at all four offsets modulo 16 bytes, scalar
# head and tail around the vector body
SHAPES = [(6, 3, 32, 32), (1, 3, 8, 8), (67, 3, 8, 8), (3, 3, 66, 66), (5, 1, 5, 7)]


def small_form(shape):
    return math.prod(shape[1:]) * 4 <= 16 * 1024


def test_gp_shapes_reach_both_forms():
    assert [small_form(s) for s in SHAPES] == [True, True, True, False, True]
    ws = ops.lib().raw('contrad_gp_penalty_workspace_bytes')
    assert ws(6, 3 * 32 * 32) == 16 and ws(67, 3 * 8 * 8) == 16 and ws(5, 35) == 16
    assert ws(3, 3 * 66 * 66) == 3 * 4 * 4                       # 13068 floats: 4 partial sums per image
    assert any(math.prod(s[1:]) % 4 for s in SHAPES) and any(math.prod(s[1:]) < 256 for s in SHAPES)


def errors(out, ref):
    out, ref = out.detach().cpu().to(torch.float64), ref.to(torch.float64)
    e = out - ref
    return (e.abs().max().item() / max(ref.abs().max().item(), 1e-30), e.norm().item() / max(ref.norm().item(), 1e-30))


def check(margin, family, what, out, ref):
    assert torch.isfinite(out).all(), (family, what, 'non-finite output')
    emax, el2 = errors(out, ref)
    print('%s %s: max-norm %.3e rel-L2 %.3e' % (family, what, emax, el2))
    assert emax < CONTRACT and el2 < CONTRACT, (family, what, emax, el2)
    tmax, tl2 = FAMILY_TOL[family]
    margin('gp %s max-norm' % family, emax, tmax)
    margin('gp %s rel-L2' % family, el2, tl2)


class Guard(object):
    """``shape`` inside NaN-filled storage with spare floats on both sides; ``shift`` floats off the 16-byte grid."""

    def __init__(self, shape, fill=None, shift=0):
        n = math.prod(shape)
        self.pad = (math.prod(shape[1:]) + 3) // 4 * 4 + 4
        self.n, self.lo = n, self.pad + shift
        self.buf = torch.full((n + 2 * self.pad + 4,), NAN, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


def interpolate(x, g, alpha, shift=0):
    gx, gg, ga, go = Guard(x.shape, x, shift), Guard(g.shape, g, shift), Guard(alpha.shape, alpha), Guard(x.shape, None, shift)
    ops.gp_interpolate(gx.view, gg.view, ga.view, out=go.view)
    torch.cuda.synchronize()
    assert gx.intact() and gg.intact() and ga.intact() and go.intact(), 'a guard sentinel was overwritten'
    assert torch.equal(gx.view.cpu(), x) and torch.equal(gg.view.cpu(), g), 'an input was modified'
    return go.view.cpu()


def penalty(grad, shift=0):
    """-> (out (1,), norms (N,), cot) on the host; the call is made twice and must repeat bit for bit."""
    runs = []
    for _ in range(2):
        gg, gc = Guard(grad.shape, grad, shift), Guard(grad.shape, None, shift)
        out, norms, cot = ops.gp_penalty(gg.view, LBD, cot=gc.view)
        torch.cuda.synchronize()
        assert gg.intact() and gc.intact(), 'a guard sentinel was overwritten'
        assert torch.equal(gg.view.cpu(), grad), 'the input was modified'
        assert cot.data_ptr() == gc.view.data_ptr()
        runs.append((out.cpu(), norms.cpu(), cot.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two calls differ'
    return runs[0]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('shift', [0, 1])          # 1: base pointers off the 16-byte grid, the all-scalar instance
def test_interpolate_matches_float64_and_keeps_the_end_rows(shape, shift, margin):
    N = shape[0]
    gen = torch.Generator().manual_seed(sum(shape) + shift)
    x, g = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    x.view(-1)[::7] = -0.0                                        # signed zeros must come through as they are
    g.view(-1)[::5] = 0.0
    alpha = torch.rand(N, generator=gen)
    what = '%s shift %d' % (shape, shift)
    check(margin, 'gp_interp', what, interpolate(x, g, alpha, shift), R.interpolate(x, g, alpha))
    for a in (0.0, 1.0):                                          # every row at an end (covers N = 1)
        out = interpolate(x, g, torch.full((N,), a), shift)
        assert same_bits(out, x if a == 1.0 else g), (what, a)
    if N >= 3:                                                    # ends next to interior rows
        alpha[0], alpha[N - 1] = 0.0, 1.0
        out = interpolate(x, g, alpha, shift)
        assert same_bits(out[0], g[0]) and same_bits(out[N - 1], x[N - 1]), what
        check(margin, 'gp_interp', what + ' mixed', out, R.interpolate(x, g, alpha))


def penalty_inputs(shape, seed):
    """Random rows; with at least three: row 0 all zero, row 1 scaled to norm 1 (in float64, then rounded)."""
    gen = torch.Generator().manual_seed(seed)
    grad = torch.randn(shape, generator=gen)
    if shape[0] >= 3:
        grad[0] = 0.0
        grad[1] = (grad[1].double() / grad[1].double().norm()).float()
    return grad


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('shift', [0, 1])
def test_penalty_matches_float64(shape, shift, margin):
    N = shape[0]
    what = '%s shift %d' % (shape, shift)
    variants = [penalty_inputs(shape, sum(shape) + shift)]
    if N == 1:                                                    # the single row as a zero row and as a unit row
        unit = (variants[0].double() / variants[0].double().norm()).float()
        variants += [torch.zeros(shape), unit]
    for k, grad in enumerate(variants):
        out, norms, cot = penalty(grad, shift)
        value, rnorms, rcot = R.penalty(grad, LBD)
        check(margin, 'gp_penalty_fwd', what + ' norms %d' % k, norms, rnorms)
        assert torch.isfinite(cot).all() and torch.isfinite(norms).all() and torch.isfinite(out).all(), what
        zero = rnorms == 0
        assert (norms[zero] == 0).all() and (cot[zero] == 0).all(), what          # exactly 0, no NaN from 0 / 0
        # a row of norm 1 (to float32 rounding): norm - 1 cancels, so its cotangent is judged by its size -- tiny, no blow-up --
        # and the relative checks need at least one other non-zero row to scale by
        unit = (rnorms - 1).abs() < 1e-5
        if N >= 3 or k > 0:
            assert zero.any() or unit.any(), what
        if unit.any():
            bound = 2 * LBD * 1e-5 / N * grad[unit].abs().max().item()
            assert cot[unit].abs().max().item() <= bound, (what, cot[unit].abs().max().item(), bound)
        if (~unit & ~zero).any() or zero.all():
            check(margin, 'gp_penalty_fwd', what + ' value %d' % k, out, value.reshape(1))
        else:
            assert out.abs().item() <= LBD * 1e-10, (what, out)
        if (~unit & ~zero).any():
            check(margin, 'gp_penalty_cot', what + ' cot %d' % k, cot, rcot)
    # autograd through penalty._GradientPenalty = the cotangent, scaled by the upstream gradient
    from contrad_amd.penalty import _GradientPenalty
    grad = variants[0]
    leaf = grad.to(DEV).requires_grad_()
    (_GradientPenalty.apply(leaf, LBD) * 3.0).backward()
    check(margin, 'gp_penalty_cot', what + ' autograd', leaf.grad.cpu(), 3.0 * R.penalty(grad, LBD)[2])
