"""The gradient penalty (--penalty=gp), the part that needs no GPU: the float64 restatement (tests/gp_ref64.py) equals float64
autograd of the reference's expression and reproduces the reference's recorded step (tests/golden/gp.npz); the new ABI entries
report their argument errors; a discriminator without a second-order path raises; the WGAN-GP configuration parses."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import gp_ref64 as R
from contrad_amd import _lib, config, ops
from contrad_amd.penalty import compute_penalty
from oracle import contrad_oracle as O

f64 = torch.float64


def T(a):
    return torch.from_numpy(a)


def close(a, b, tol):
    a, b = torch.as_tensor(a).to(f64), torch.as_tensor(b).to(f64)
    return ((a - b).abs().max() <= tol * b.abs().max().clamp_min(1e-300)).item()


def test_interpolate_and_penalty_match_float64_autograd():
    gen = torch.Generator().manual_seed(1)
    x, g = torch.rand(5, 3, 4, 6, generator=gen, dtype=f64), torch.rand(5, 3, 4, 6, generator=gen, dtype=f64)
    alpha = torch.tensor([0.0, 1.0, 0.25, 0.5, 0.875], dtype=f64)
    xh = R.interpolate(x, g, alpha)
    assert torch.equal(xh[0], g[0]) and torch.equal(xh[1], x[1])
    assert close(xh, alpha.view(-1, 1, 1, 1).expand_as(x) * x + (1 - alpha.view(-1, 1, 1, 1).expand_as(x)) * g, 1e-15)
    grad = torch.randn(5, 3, 4, 6, generator=gen, dtype=f64)
    grad[1] = 0.0                                             # a zero row: torch's 2-norm backward returns 0 there
    grad[2] /= grad[2].norm()                                 # norm 1: the cotangent all but vanishes
    leaf = grad.clone().requires_grad_()
    norms = leaf.view(5, -1).norm(2, dim=1)
    want = 10.0 * ((norms - 1) ** 2).mean()
    want.backward()
    value, n, cot = R.penalty(grad, 10.0)
    assert close(value, want, 1e-12) and close(n, norms.detach(), 1e-12) and close(cot, leaf.grad, 1e-12)
    assert cot[1].abs().max().item() == 0.0 and leaf.grad[1].abs().max().item() == 0.0
    assert torch.isfinite(cot).all() and cot[2].abs().max().item() < 1e-12


def test_second_order_gradients_of_a_two_conv_network():
    gen = torch.Generator().manual_seed(2)
    w1 = (torch.randn(8, 3, 3, 3, generator=gen, dtype=f64) * 0.3).requires_grad_()
    b1 = (torch.randn(8, generator=gen, dtype=f64) * 0.1).requires_grad_()
    w2 = (torch.randn(1, 8, 4, 4, generator=gen, dtype=f64) * 0.3).requires_grad_()
    params = [w1, b1, w2]

    def d_fn(t):
        h = F.leaky_relu(F.conv2d(t * 2 - 1, w1, b1, padding=1), 0.1)
        return F.conv2d(h, w2, None, stride=2, padding=1).flatten(1).sum(1, keepdim=True)

    x, g = torch.rand(4, 3, 8, 8, generator=gen, dtype=f64), torch.rand(4, 3, 8, 8, generator=gen, dtype=f64)
    alpha = torch.rand(4, generator=gen, dtype=f64)
    value, norms, grads = R.second_order_grads(d_fn, params, x, g, alpha, 10.0)
    want, want_norms = R.reference_expression(d_fn, x, g, alpha, 10.0)
    want_grads = torch.autograd.grad(want, params, allow_unused=True)
    assert close(value, want.detach(), 1e-12) and close(norms, want_norms.detach(), 1e-12)
    for got, ref in zip(grads, want_grads):
        # the bias enters the input gradient only through the LeakyReLU's region, which is locally constant
        assert (got is None or got.abs().max().item() == 0.0) if ref is None or ref.abs().max().item() == 0.0 \
            else close(got, ref, 1e-12)
    assert want_grads[0].abs().max().item() > 0 and want_grads[2].abs().max().item() > 0


SHAPES = {'sndcgan': O.sndcgan_d_param_shapes, 'snresnet18': O.snresnet18_param_shapes}


@pytest.mark.parametrize('arch', ['sndcgan', 'snresnet18'])
def test_ref64_reproduces_the_recorded_reference_step(arch, golden):
    """The tie to the imported reference, as for the other families: 1e-6 (the fixture is stored rounded to float32)."""
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    g = golden('gp')
    t = arch + '/'
    N, lbd = int(g['N']), float(g['lbd'])
    x, fake, alpha = T(g['x']).double(), T(g['fake']).double(), T(g[t + 'alpha']).double()
    torch.manual_seed(int(g['alpha_seed']))
    assert torch.equal(torch.rand(N, 1, 1, 1).view(N), T(g[t + 'alpha']))          # the draw at the reference's point
    sd = R.leaf_state(O.det_fill(SHAPES[arch](), seed=1234))
    d_all = R.d_logits(arch, sd, True)(torch.cat([x, fake]))                        # first D call: first power iteration
    d_loss = d_all[N:].mean() - d_all[:N].mean()
    assert close(d_loss.detach(), g[t + 'd_loss'], 1e-6)
    assert close(d_all[:N].mean().detach(), g[t + 'd_real'], 1e-6) and close(d_all[N:].mean().detach(), g[t + 'd_gen'], 1e-6)
    value, norms, grads = R.gp_step(arch, sd, x, fake, alpha, lbd)                  # second D call
    assert close(value, g[t + 'penalty'], 1e-6) and close(norms, g[t + 'norms'], 1e-6)
    seen = 0
    for name, got in grads.items():
        if t + 'pen/none/' + name in g.files:
            assert got is None or got.abs().max().item() == 0.0, name
            continue
        ref = float(g[t + 'pen/gradnorm/' + name])
        if ref < 1e-7:
            assert got is None or got.norm().item() < 1e-7, name
            continue
        seen += 1
        assert abs(got.norm().item() - ref) < 1e-6 * ref, name
        if t + 'pen/grad/' + name in g.files:
            assert ((got - T(g[t + 'pen/grad/' + name]).double()).norm() / ref).item() < 1e-6, name
        else:
            assert ((got.reshape(-1)[:512] - T(g[t + 'pen/gradhead/' + name]).double()).abs().max() / ref).item() < 1e-6, name
    assert seen >= 9                # every weight on the logit path (sndcgan: 7 convs + the two logit-head layers)
    n_after = 0
    for k in g.files:                                                               # u / v after TWO power iterations
        if k.startswith(t + 'after/'):
            assert close(sd[k[len(t) + 6:]], g[k], 1e-6), k
            n_after += 1
        elif k.startswith(t + 'afterhead/'):
            assert close(sd[k[len(t) + 10:]][:512], g[k], 1e-6), k
            n_after += 1
    assert n_after == 2 * len([k for k in sd if k.endswith('weight_u')])


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_gp_entries_report_argument_errors_without_gpu(built):
    assert {'contrad_gp_interpolate', 'contrad_gp_penalty', 'contrad_gp_penalty_workspace_bytes'} <= set(built.protos)
    assert callable(ops.gp_interpolate) and callable(ops.gp_penalty)
    a, b, c, d = (ctypes.c_void_p(16 * k) for k in (1, 2, 3, 4))      # distinct non-null pointers, never dereferenced:
    ll = ctypes.c_longlong                                            # the checks come before any launch
    for args in ((None, b, c, d, 2, ll(12)), (a, None, c, d, 2, ll(12)), (a, b, None, d, 2, ll(12)), (a, b, c, None, 2, ll(12)),
                 (a, b, c, d, 0, ll(12)), (a, b, c, d, -3, ll(12)), (a, b, c, d, 2, ll(0)), (a, b, c, d, 2, ll(-5)),
                 (a, b, c, a, 2, ll(12)), (a, b, c, b, 2, ll(12))):                # in place
        with pytest.raises(RuntimeError):
            built.call('contrad_gp_interpolate', *args, None)
    for args in ((None, b, c, d, 2, ll(12)), (a, None, c, d, 2, ll(12)), (a, b, None, d, 2, ll(12)), (a, b, c, None, 2, ll(12)),
                 (a, b, c, d, 0, ll(12)), (a, b, c, d, 2, ll(0)), (a, b, c, a, 2, ll(12)),
                 (a, b, c, d, 2, ll(66 * 66 * 3))):                        # the two-launch form without its workspace
        with pytest.raises(RuntimeError):
            built.call('contrad_gp_penalty', *args, 10.0, None, ll(0), None)
    ws = built.raw('contrad_gp_penalty_workspace_bytes')
    assert ws(0, ll(12)) < 0 and ws(2, ll(0)) < 0 and ws(-1, ll(-1)) < 0
    assert ws(6, ll(3 * 32 * 32)) == 16 and ws(6, ll(4096)) == 16              # up to 16 KiB: one workgroup per image
    assert ws(3, ll(4097)) == 3 * 2 * 4 and ws(3, ll(3 * 66 * 66)) == 3 * 4 * 4    # partial sums of 4096 floats


class _NoSecondOrder(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1).sum(1, keepdim=True)


def test_gp_needs_a_discriminator_with_a_second_order_path():
    x = torch.rand(2, 3, 4, 4)
    with pytest.raises(NotImplementedError, match='second-order'):
        compute_penalty('gp', D=_NoSecondOrder(), images=x, gen_images=x, lbd=10.0, P=None)
    from contrad_amd.models.gan import get_architecture
    for arch in ('sndcgan', 'snresnet18'):
        _, D = get_architecture(arch, (32, 32, 3))
        assert callable(getattr(D, 'second_order', None)), arch
    D = get_architecture('sndcgan', (32, 32, 3))[1]
    assert not getattr(D, '_second_order', False)
    with D.second_order():
        assert D._second_order
    assert not D._second_order


def test_wgangp_config_parses():
    from contrad_amd.train_gan import get_options_dict
    config.clear_config()
    config.parse_config_files_and_bindings([os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin'),
                                            os.path.join(config.CONFIG_ROOT, 'gan', 'cifar10', 'c10_wgangp.gin')])
    opt = get_options_dict()
    assert (opt['dataset'], opt['batch_size'], opt['loss'], opt['n_critic'], opt['max_steps']) == \
        ('cifar10', 64, 'wgan', 5, 200000)
    assert opt['lr'] == 1e-4 and opt['lr_d'] == 1e-4 and tuple(opt['beta']) == (0.0, 0.9) and opt['lbd'] == 10.0
    config.clear_config()
