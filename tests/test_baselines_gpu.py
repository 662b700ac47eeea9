"""GPU tests of the baseline training modes (std / aug / aug_both, CR / bCR, hfrt / DiffAugment): the kernels of
csrc/baseline_aug.hip against float64 (tests/baselines_ref64.py) and the reference's recorded outputs
(tests/golden/baselines.npz), the recorded training steps, determinism and the command lines.

Kernel parity follows the rule of tests/test_augment_kernels_gpu.py: operands live in NaN-filled guard storage (every
sentinel must survive, an over-read shows up as a NaN), the max-norm error max|e| / max|ref| stays below the 1e-3
contract and, with the rel-L2 error, below a per-family bound of about 5x the worst seen on an MI355X (FAMILY_TOL,
recorded through ``margin``).  What is exact is compared bitwise: the hfrt index map and its adjoint on integer-valued
gradients, the 0.5 of cut and shifted-out DiffAugment pixels, and the zero gradient of those pixels wherever the backward
is a pure mask (policies without ``color``, and colour rows with s = c = 1; with colour the two mean terms reach every
pixel, so there the float64 reference decides).
"""
import argparse
import math
import os

import pytest
import torch

import baselines_ref64 as R
from contrad_amd import config, ops
from contrad_amd.augment import DiffAugLayer, HorizontalFlipLayer, HorizontalFlipRandomCrop, get_augment
from contrad_amd.engine import set_grad
from contrad_amd.models.gan import get_architecture
from contrad_amd.penalty import _Consistency
from contrad_amd.training.gan import setup
from oracle import contrad_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
TOL = 1e-3
# as in tests/test_sndcgan_gpu.py (its comment on leaky-ReLU flips applies unchanged)
FLIP_TOL = float(os.environ.get('CONTRAD_FLIP_TOL', '1e-3'))

FAMILY_TOL = {                  # family: (max-norm, rel-L2) = 5x the observed worst on an MI355X (max-norm, rel-L2)
    'diffaug_fwd': (6.4e-7, 2.4e-7),            # 1.29e-7, 4.78e-8
    'diffaug_bwd': (4.3e-7, 2.1e-7),            # 8.69e-8, 4.26e-8
    'consistency': (5.3e-7, 5.3e-7),            # 1.06e-7, 1.06e-7
}
POLICIES = ('color', 'translation', 'cutout', 'color,cutout', 'color,translation,cutout')


def T(a):
    return torch.from_numpy(a)


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
    margin('baselines %s max-norm' % family, emax, tmax)
    margin('baselines %s rel-L2' % family, el2, tl2)


class Guard(object):
    """``shape`` inside NaN-filled storage with spare floats (a multiple of 4) on both sides."""

    def __init__(self, shape, fill=None, shift=0):
        n = math.prod(shape)
        self.pad = (math.prod(shape[1:]) + 3) // 4 * 4 + 4 + shift        # (shift: floats off 16-byte alignment)
        self.n = n
        self.buf = torch.full((n + 2 * self.pad,), NAN, device=DEV)
        self.view = self.buf[self.pad:self.pad + n].view(*shape)
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.pad]).all()) and bool(torch.isnan(self.buf[self.pad + self.n:]).all())


def guarded(fn, x, params, out_shift=0):
    """fn(x, params, out=...) with all three operands in guard storage; returns the output on the host."""
    gx, gp, go = Guard(tuple(x.shape), x), Guard(tuple(params.shape), params), Guard(tuple(x.shape), shift=out_shift)
    fn(gx.view, gp.view, go.view)
    torch.cuda.synchronize()
    assert gx.intact() and gp.intact() and go.intact(), 'a guard sentinel was overwritten'
    assert torch.equal(gx.view.cpu(), x), 'the input was modified'
    return go.view.cpu()


# ======================================================================================================================
# HorizontalFlipRandomCrop
# ======================================================================================================================
def forced_hfrt_rows(m):
    """+-m on both axes with both flip signs (deep reflection at m = W - 1)."""
    return torch.tensor([[s, kx, ky, 0.] for s in (1., -1.) for kx in (-m, 0, m) for ky in (-m, 1, m)])


@pytest.mark.parametrize('tag', ['hfrt32', 'hfrt8'])
def test_hfrt_forward_is_the_reference_bit_for_bit(tag, golden):
    g = golden('baselines')
    x, P, y, m = T(g[tag + '/x']), T(g[tag + '/P']), T(g[tag + '/y']), int(g[tag + '/m'])
    for B in (1, 5):
        out = guarded(lambda a, p, o: ops.hfrt(a, p, m, out=o), x[:B].contiguous(), P[:B].contiguous())
        assert torch.equal(out, y[:B]), (tag, B)
        assert torch.equal(out, R.hfrt_forward(x[:B], P[:B])), (tag, B)
    F = forced_hfrt_rows(m)
    W = x.shape[2]
    xf = torch.rand(F.shape[0], 3, W, W, generator=torch.Generator().manual_seed(3))
    out = guarded(lambda a, p, o: ops.hfrt(a, p, m, out=o), xf, F)
    assert torch.equal(out, R.hfrt_forward(xf, F)), tag
    for r in (0, F.shape[0] - 1):                          # B = 1 with a forced row
        out = guarded(lambda a, p, o: ops.hfrt(a, p, m, out=o), xf[r:r + 1].contiguous(), F[r:r + 1].contiguous())
        assert torch.equal(out, R.hfrt_forward(xf[r:r + 1], F[r:r + 1]))


@pytest.mark.parametrize('W,m,shift', [(6, 5, 0), (7, 3, 0), (8, 7, 1), (32, 4, 2)])
def test_hfrt_forward_one_pixel_per_thread_is_exact(W, m, shift):
    """hfrt_fwd_kernel<false>: a width that is no multiple of 4, or an output off 16-byte alignment (the other instance makes
    four columns per thread and stores them as one vector) -- the same index map, bit for bit, nothing else written."""
    F = forced_hfrt_rows(m)
    for B in (1, 5, F.shape[0]):
        P = F[:B].contiguous() if B > 1 else F[-1:].contiguous()
        x = torch.rand(B, 3, W, W, generator=torch.Generator().manual_seed(10 * W + B))
        out = guarded(lambda a, p, o: ops.hfrt(a, p, m, out=o), x, P, out_shift=shift)
        assert torch.equal(out, R.hfrt_forward(x, P)), (W, m, shift, B)


@pytest.mark.parametrize('W,m', [(32, 4), (8, 7)])
def test_hfrt_adjoint_is_exact_on_integer_gradients(W, m):
    F = forced_hfrt_rows(m)
    gen = torch.Generator().manual_seed(4)
    for B in (1, 5, F.shape[0]):
        P = F[:B].contiguous() if B > 1 else F[-1:].contiguous()
        gy = torch.randint(-8, 9, (B, 3, W, W), generator=gen).float()      # sums of at most 4 of them are exact in fp32
        out = guarded(lambda a, p, o: ops.hfrt(a, p, m, adjoint=True, out=o), gy, P)
        assert torch.equal(out.double(), R.hfrt_adjoint(gy, P)), (W, m, B)


def test_hfrt_layers_and_their_autograd(golden):
    g = golden('baselines')
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin')])
    layer = get_augment(mode='hfrt').to(DEV)
    x, y = T(g['hfrt32/x']), T(g['hfrt32/y'])
    torch.manual_seed(int(g['hfrt32/seed']))
    assert torch.equal(layer(x.to(DEV)).cpu(), y)                    # sample() replays the reference's draws
    xd = x.to(DEV).requires_grad_()
    w = torch.randint(-8, 9, x.shape).float()
    P = T(g['hfrt32/P'])
    (layer.apply(xd, P) * w.to(DEV)).sum().backward()
    assert torch.equal(xd.grad.cpu().double(), R.hfrt_adjoint(w, P))
    flip = HorizontalFlipLayer()
    Pf = torch.tensor([[-1., 0, 0, 0], [1., 0, 0, 0]])
    out = flip.apply(x[:2].to(DEV), Pf).cpu()
    assert torch.equal(out[0], x[0].flip(-1)) and torch.equal(out[1], x[1])
    with pytest.raises(RuntimeError):                                # H != W, width mismatch, max_pixels >= W
        ops.hfrt(torch.rand(1, 3, 8, 16, device=DEV), Pf[:1].to(DEV), 4)
    with pytest.raises(RuntimeError):
        layer(torch.rand(2, 3, 16, 16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.hfrt(torch.rand(1, 3, 8, 8, device=DEV), Pf[:1].to(DEV), 8)


# ======================================================================================================================
# DiffAugment
# ======================================================================================================================
def diffaug_rows(B, H, W, seed):
    """Forced rows first -- translations at +-max, cutout offsets 0 and max (the window hangs over both borders), s = 0,
    c = 0.5, and a row with s = c = 1 (a pure mask in the backward) -- then the sampler's own draws."""
    sx, sy, cx, cy = int(H * .125 + .5), int(W * .125 + .5), int(H * .5 + .5), int(W * .5 + .5)
    ox_max, oy_max = H - cx % 2, W - cy % 2
    forced = torch.tensor([[0.25, 0.0, 0.5, sx, -sy, 0, oy_max, 0],
                           [-0.5, 1.0, 1.0, -sx, sy, ox_max, 0, 0],
                           [0.4, 2.0, 1.5, sx, sy, ox_max, oy_max, 0],
                           [-0.3, 0.7, 0.5, -sx, -sy, 0, 0, 0]])
    torch.manual_seed(seed)
    drawn = DiffAugLayer(policy='color,translation,cutout').sample(max(B - 4, 1), H, W)
    return torch.cat([forced, drawn])[:B].contiguous() if B > 1 else forced[1:2].contiguous()


def small_form(H, W):
    return 3 * H * W * 4 <= 16 * 1024


# LDS form; LDS form, cutout 15 x 10 and shifts 4 and 3; two-pass form; W % 4 != 0: the scalar instances of both forms
DIFFAUG_SHAPES = [(32, 32), (30, 20), (64, 64), (18, 18), (66, 66)]


def test_diffaug_shapes_reach_both_forms():
    assert [small_form(H, W) for H, W in DIFFAUG_SHAPES] == [True, True, False, True, False]
    assert ops.lib().raw('contrad_diffaug_workspace_bytes')(5, 64, 64) == 5 * 3 * 4      # 12288 floats: 3 partial sums
    assert ops.lib().raw('contrad_diffaug_workspace_bytes')(5, 32, 32) == 16


def diffaug_inputs(H, W, B):
    """(x, gy, P) on the host: images, an upstream gradient and diffaug_rows.  (Shared with tests/test_workspace_contract_gpu.py.)"""
    gen = torch.Generator().manual_seed(H * 100 + W + B)
    x = torch.rand(B, 3, H, W, generator=gen)
    gy = torch.randn(B, 3, H, W, generator=gen)
    return x, gy, diffaug_rows(B, H, W, seed=H + W + B)


@pytest.mark.parametrize('H,W', DIFFAUG_SHAPES)
@pytest.mark.parametrize('B', [1, 5])
def test_diffaug_forward_and_backward_match_float64(H, W, B, margin):
    x, gy, P = diffaug_inputs(H, W, B)
    for policy in POLICIES:
        bits = ops.diffaug_policy_bits(policy)
        what = '%dx%d B=%d %s' % (H, W, B, policy)
        y = guarded(lambda a, p, o: ops.diffaug(a, p, bits, out=o), x, P)
        check(margin, 'diffaug_fwd', what, y, R.diffaug_forward(x, P, policy))
        dead = R.diffaug_dead_outputs(P, policy, H, W)
        assert (y.permute(0, 2, 3, 1)[dead] == 0.5).all(), what          # cut / shifted-out pixels: exactly 0.5
        if policy != 'color':
            assert dead.any(), what
        gx = guarded(lambda a, p, o: ops.diffaug(a, p, bits, backward=True, out=o), gy, P)
        check(margin, 'diffaug_bwd', what, gx, R.diffaug_backward(gy, P, policy))
        # the gradient of an input pixel whose output was cut or that no output reads is exactly 0 where the backward is a
        # pure mask: without colour, and on the colour row with s = c = 1 (row 1 of the forced rows; B = 1 uses that row)
        ref = R.diffaug_backward(gy, P, policy)
        pure = torch.ones(B, dtype=torch.bool) if 'color' not in policy else (P[:, 1] == 1) & (P[:, 2] == 1)
        zero = (ref == 0) & pure.view(B, 1, 1, 1)
        assert (gx[zero] == 0).all(), what
        if policy != 'color':
            assert zero.any(), what
        if 'color' not in policy:                                        # 2 * (0.5 g) is g itself
            live = ref != 0
            assert torch.equal(gx[live].double(), ref[live]), what


def test_diffaug_layer_replays_the_reference(golden, margin):
    g = golden('baselines')
    x = T(g['diffaug/x'])
    for policy in POLICIES:
        layer = DiffAugLayer(policy=policy)
        torch.manual_seed(int(g['diffaug/%s/seed' % policy]))
        y = layer(x.to(DEV)).cpu()                                    # sample() replays the reference's draws
        check(margin, 'diffaug_fwd', 'layer forward ' + policy, y, R.diffaug_forward(x, T(g['diffaug/%s/P' % policy]), policy))
        # the recorded output is the reference's own fp32 result (within 1e-6 of float64, tests/test_baselines_ref64_cpu.py)
        assert errors(y, T(g['diffaug/%s/y' % policy]))[0] < 1e-6 + FAMILY_TOL['diffaug_fwd'][0], policy
        # autograd through the layer = the backward kernel
        P = T(g['diffaug/%s/P' % policy])
        xd = x.to(DEV).requires_grad_()
        w = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
        (layer.apply(xd, P) * w.to(DEV)).sum().backward()
        check(margin, 'diffaug_bwd', 'layer ' + policy, xd.grad.cpu(), R.diffaug_backward(w, P, policy))
    assert DiffAugLayer(policy='')(x) is x


# ======================================================================================================================
# consistency term and the (2N, 1) GAN loss
# ======================================================================================================================
@pytest.mark.parametrize('n0,n1', [(6, 0), (6, 6), (300, 300), (1, 0), (257, 3)])
def test_consistency_kernel_matches_float64(n0, n1, margin):
    gen = torch.Generator().manual_seed(n0 + n1)
    n = n0 + n1
    a, b = torch.randn(n, 1, generator=gen), torch.randn(n, 1, generator=gen)
    wide = torch.randn(n, 3, generator=gen)                  # a strided logit column
    for av, ad in ((a, a.to(DEV)), (wide[:, 1:2], wide.to(DEV)[:, 1:2])):
        assert tuple(ad.shape) == (n, 1) and (n == 1 or ad.stride(0) == av.stride(0))
        out, ga, gb = ops.consistency(ad, b.to(DEV), n0, n1, 10.0, 3.0)
        val, ra, rb = R.consistency(av, b, n0, n1, 10.0, 3.0)
        check(margin, 'consistency', 'value %d+%d' % (n0, n1), out, val.reshape(1))
        check(margin, 'consistency', 'grad a %d+%d' % (n0, n1), ga, ra)
        check(margin, 'consistency', 'grad b %d+%d' % (n0, n1), gb, rb)
    ad, bd = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    (_Consistency.apply(ad, bd, n0, n1, 10.0, 3.0) * 2.0).backward()
    check(margin, 'consistency', 'autograd %d+%d' % (n0, n1), ad.grad, 2.0 * R.consistency(a, b, n0, n1, 10.0, 3.0)[1])


@pytest.mark.parametrize('kind', ['nonsat', 'wgan', 'hinge', 'lsgan'])
def test_gan_d_loss_2n_matches_the_oracle(kind):
    gen = torch.Generator().manual_seed(12)
    for N in (1, 6, 300):
        d = (torch.randn(2 * N, 1, generator=gen) * 2).double().requires_grad_()
        want = O.gan_d_loss(d[:N], d[N:], kind)
        want.backward()
        out, grad = ops.gan_d_loss_2n(d.detach().float().to(DEV), N, kind)
        assert abs(out[0].item() - want.item()) < TOL * max(abs(want.item()), 1.0), (kind, N)
        assert abs(out[1].item() - d[:N].mean().item()) < TOL and abs(out[2].item() - d[N:].mean().item()) < TOL
        assert (grad.cpu().double() - d.grad).abs().max().item() < TOL * d.grad.abs().max().item(), (kind, N)


# ======================================================================================================================
# recorded training steps
# ======================================================================================================================
def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def build():
    G, D = get_architecture('sndcgan', (32, 32, 3))
    D.load_state_dict(O.det_fill(O.sndcgan_d_param_shapes(), seed=1234))
    gsd = dict(G.state_dict()); gsd.update(O.det_fill(O.sndcgan_g_param_shapes(), seed=4321)); G.load_state_dict(gsd)
    return G.to(DEV).train(), D.to(DEV).train()


def make_P(mode, penalty, aug):
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'gan', 'diffaug', 'c10_diffaug.gin')])
    P = setup(argparse.Namespace(mode=mode, penalty=penalty, aug=aug, distributed=False))
    P.augment_fn = get_augment(mode=aug).to(DEV)
    return P


def compare_grads(g, prefix, named, grads, flip_tol):
    """Gradient norms within TOL, tensors (or their first 512 entries) within flip_tol / TOL of the norm; parameters the
    reference's term does not reach (its gradient is None there) must be exactly zero."""
    seen, zeros = 0, []
    for (name, _), got in zip(named, grads):
        if prefix + 'none/' + name in g.files:
            assert got is None or got.abs().max().item() == 0.0, (prefix, name)
            continue
        ref = float(g[prefix + 'gradnorm/' + name])
        seen += 1
        if got is None:
            got = torch.zeros(1)
        if ref == 0.0 and name.startswith('projection'):    # heads these modes never read: exactly zero in the reference
            assert got.abs().max().item() == 0.0, (prefix, name)
            zeros.append(name)
            continue
        if ref < 1e-7:              # a gradient that cancels: a bias in front of a batch-statistics BatchNorm (tests/
                                    # test_gstep_gpu.py), the logit bias under a consistency term: zero up to noise
            assert got.norm().item() < 1e-5, (prefix, name)
            continue
        e = abs(got.norm().item() - ref) / ref
        print('%s gradnorm %s: %.3e' % (prefix, name, e))
        assert e < TOL, (prefix, name, e)
        if prefix + 'grad/' + name in g.files:
            e = l2(got, g[prefix + 'grad/' + name])
            print('%s grad-l2 %s: %.3e' % (prefix, name, e))
            assert e < flip_tol, (prefix, name, e)
        else:
            head = got.reshape(-1)[:512].cpu().double()
            e = (head - T(g[prefix + 'gradhead/' + name]).double()).abs().max().item() / ref
            print('%s gradhead %s: %.3e' % (prefix, name, e))
            assert e < TOL, (prefix, name, e)
    assert seen > 0
    return zeros


D_CASES = [('std+none', 'std', 'none', 'none'), ('std+cr+hfrt', 'std', 'cr', 'hfrt'), ('std+bcr+hfrt', 'std', 'bcr', 'hfrt'),
           ('aug+hfrt', 'aug', 'none', 'hfrt'), ('aug_both+diffaug', 'aug_both', 'none', 'diffaug')]


def run_d_step(g, tag, mode, penalty, aug):
    _, D = build()
    P = make_P(mode, penalty, aug)
    options = {'loss': 'nonsat', 'lbd': float(g['step/lbd']), 'lbd2': float(g['step/lbd2'])}
    x, fake = T(g['step/x']).to(DEV), T(g['step/fake']).to(DEV)
    torch.manual_seed(int(g['step/%s/seed' % tag]))              # the augmentation's sample() replays the recorded draws
    d_loss, aux = P.train_fn['D'](P, D, options, x, fake)
    return D, d_loss, aux


@pytest.mark.parametrize('tag,mode,penalty,aug', D_CASES)
def test_discriminator_steps_match_the_reference(tag, mode, penalty, aug, golden):
    g = golden('baselines')
    t = 'step/%s/' % tag
    D, d_loss, aux = run_d_step(g, tag, mode, penalty, aug)
    assert abs(d_loss.item() - float(g[t + 'd_loss'])) < TOL * abs(float(g[t + 'd_loss']))
    for key in ('d_real', 'd_gen'):           # mean logits of a fresh D are ~1e-3: relative, or all-zero logits would pass
        ref = float(g[t + key])
        print('%s %s %.6e ref %.6e' % (tag, key, aux[key].item(), ref))
        assert abs(aux[key].item() - ref) < TOL * abs(ref), (tag, key)
    assert aux['penalty'].shape == (1,) if penalty == 'none' else aux['penalty'].dim() == 0
    ref_pen = float(g[t + 'penalty'])
    print('%s penalty %.6e ref %.6e' % (tag, aux['penalty'].item(), ref_pen))
    assert abs(aux['penalty'].item() - ref_pen) <= TOL * abs(ref_pen)
    named = list(D.named_parameters())
    params = [p for _, p in named]
    has_pen = penalty != 'none'
    assert aux['penalty'].requires_grad == has_pen
    zeros = compare_grads(g, t + 'gan/', named,
                          torch.autograd.grad(d_loss, params, retain_graph=has_pen, allow_unused=True), FLIP_TOL)
    assert zeros and all(k.startswith('projection') for k in zeros), zeros
    if has_pen:
        zeros = compare_grads(g, t + 'pen/', named, torch.autograd.grad(aux['penalty'], params, allow_unused=True), FLIP_TOL)
        assert zeros and all(k.startswith('projection') for k in zeros), zeros
    # u / v after the step: CR / bCR ran TWO power iterations (the second D call saw the first call's u / v)
    sd = D.state_dict()
    n_after = 0
    for k in g.files:
        if k.startswith(t + 'after/'):
            assert rel(sd[k[len(t) + 6:]], g[k]) < TOL, k
            n_after += 1
        elif k.startswith(t + 'afterhead/'):
            assert rel(sd[k[len(t) + 10:]][:512], g[k]) < TOL, k
            n_after += 1
    assert n_after == 26


def test_two_discriminator_calls_are_two_power_iterations(golden):
    """The fixture separates one power iteration from two by far more than the 1e-3 the step test allows."""
    g = golden('baselines')
    k = 'after/main.2.weight_u'
    assert rel(g['step/std+none/' + k], g['step/std+cr+hfrt/' + k]) > 10 * TOL


def test_generator_step_matches_the_reference(golden):
    g = golden('baselines')
    G, D = build()
    set_grad(G, True); set_grad(D, False)
    P = make_P('aug_both', 'none', 'diffaug')
    gen = G(T(g['step/z']).to(DEV))
    assert rel(gen, g['step/fake']) < TOL
    torch.manual_seed(int(g['gstep/seed']))
    g_loss = P.train_fn['G'](P, D, {'loss': 'nonsat'}, None, gen)
    assert abs(g_loss.item() - float(g['gstep/g_loss'])) < TOL * abs(float(g['gstep/g_loss']))
    named = list(G.named_parameters())
    grads = torch.autograd.grad(g_loss, [p for _, p in named], allow_unused=True)
    assert all(p.grad is None for p in D.parameters())
    compare_grads(g, 'gstep/', named, grads, FLIP_TOL)


def test_bcr_step_is_bitwise_deterministic(golden):
    g = golden('baselines')
    runs = []
    for _ in range(2):
        D, d_loss, aux = run_d_step(g, 'std+bcr+hfrt', 'std', 'bcr', 'hfrt')
        (d_loss + aux['penalty']).backward()
        runs.append(([d_loss.detach().clone(), aux['penalty'].detach().clone()], [p.grad.clone() for p in D.parameters()],
                     [b.clone() for b in D.buffers()]))
    for a, b in zip(runs[0], runs[1]):
        assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.isfinite(p).all() for p in runs[0][1])


# ======================================================================================================================
# command lines
# ======================================================================================================================
def _finite_checkpoints(logdir, files):
    for f in files:
        sd = torch.load(os.path.join(logdir, f))
        assert all(torch.isfinite(v).all() for v in sd.values() if torch.is_tensor(v) and v.is_floating_point()), f
    assert 'nan' not in open(os.path.join(logdir, 'log.txt')).read().lower()


@pytest.mark.parametrize('gin,extra', [
    ('cifar10/c10_b64.gin', ['--mode=std', '--penalty=bcr', '--aug=hfrt']),
    ('diffaug/c10_diffaug.gin', ['--mode=aug_both', '--aug=diffaug'])])
def test_train_gan_cli_runs_the_baselines(gin, extra, tmp_path):
    from contrad_amd.train_gan import main
    logdir = str(tmp_path / 'run')
    main([os.path.join(config.CONFIG_ROOT, 'gan', gin), 'sndcgan'] + extra +
         ['--synthetic', '--max_steps', '3', '--print_every', '1', '--evaluate_every', '3', '--logdir', logdir])
    _finite_checkpoints(logdir, ('gen.pt', 'dis.pt'))
    assert '[Steps       3]' in open(os.path.join(logdir, 'log.txt')).read()


def test_train_stylegan2_cli_runs_std_mode(tmp_path):
    """--mode=std on StyleGAN2; the R1 penalty (every 2nd step here) goes through get_augment('none')."""
    from contrad_amd.train_stylegan2 import main
    logdir = str(tmp_path / 'run')
    main([os.path.join(config.CONFIG_ROOT, 'gan', 'stylegan2', 'c10_style64.gin'), 'stylegan2', '--mode=std', '--synthetic',
          '--max_steps', '2', '--batch_size', '8', '--d_reg_every', '2', '--print_every', '1', '--evaluate_every', '2',
          '--logdir', logdir])
    _finite_checkpoints(logdir, ('gen.pt', 'dis.pt', 'gen_ema.pt'))
    assert 'r1' in open(os.path.join(logdir, 'log.txt')).read()
