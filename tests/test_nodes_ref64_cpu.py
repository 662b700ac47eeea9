"""The float64 twins of tests/nodes_ref64.py are themselves checked here, without a GPU:

* every twin against torch's own CPU float64 operators (F.conv2d / F.conv_transpose2d / F.leaky_relu, an upfirdn2d written
  tap by tap from its definition, the torch-op minibatch-stddev layer, torch.nn.utils.spectral_norm, ops.pack_weight): the
  whole protocol -- value, first-order and second-order gradients -- agrees to 1e-12;
* every case with an activation keeps the reference's smallest |pre-activation| above nodes_ref64.GUARD;
* the conv cases reach a Winograd-planned forward, dgrad and wgrad call and the direct paths 0 - 3 and 5
  (contrad_conv2d_path, host logic only);
* the protocol is sensitive: a twin with one wrong arrow in its backward misses the bound of its class by more than 100x;
* every Function class of contrad_amd/autograd_ops.py has a case in tests/test_autograd_nodes_gpu.py.
"""
import ctypes
import importlib.util
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import dstep_ref64 as D  # noqa: E402
import nodes_ref64 as N  # noqa: E402
from contrad_amd import _lib, ops  # noqa: E402

f64 = torch.float64
TIGHT = 1e-12
_BIG = ('wino', 'f44')                       # the Winograd-planned shapes: float64 on a GPU only (they have no activation)


def _gpu_module():
    """The GPU test module, loaded for its tables only (importing it touches no GPU)."""
    spec = importlib.util.spec_from_file_location('_autograd_nodes_cases', os.path.join(_HERE, 'test_autograd_nodes_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _small(case):
    return not case['id'].split('-', 1)[1].startswith(_BIG)


SMALL = [c for c in N.CASES if _small(c)]


# ---- the same operations from torch's own operators ------------------------------------------------------------------
def _oihw(wp, K, C, k):
    return wp[:, :K].reshape(k, k, C, K).permute(3, 2, 0, 1)


def _packed(w, ldw):
    K, C, k, _ = w.shape
    return F.pad(w.permute(2, 3, 1, 0).reshape(k * k * C, K), (0, ldw - K))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def i_conv2d(c, x, wp):
    return _nhwc(F.conv2d(_nchw(x), _oihw(wp, c['K'], c['C'], c['k']), stride=c['s'], padding=c['p']))


def i_dgrad(c, gy, wp):
    k, s, p = c['k'], c['s'], c['p']
    op = (c['H'] - ((gy.shape[1] - 1) * s - 2 * p + k), c['W'] - ((gy.shape[2] - 1) * s - 2 * p + k))
    return _nhwc(F.conv_transpose2d(_nchw(gy), _oihw(wp, c['K'], c['C'], k), stride=s, padding=p, output_padding=op))


def _i_dw(c, x, gy):
    w0 = torch.zeros(c['K'], c['C'], c['k'], c['k'], dtype=f64)
    return N.adjoint(lambda w: _nhwc(F.conv2d(_nchw(x), w, stride=c['s'], padding=c['p'])), w0, gy)


def i_wgrad(c, x, gy):
    return _packed(_i_dw(c, x, gy), c.get('ldw', N.round4(c['K'])))


def i_wgrad_bias(c, x, gy):
    return i_wgrad(c, x, gy), gy.reshape(-1, c['K']).sum(0)


def i_act(c, x):
    return F.leaky_relu(x, c['slope']) * c['gain']


def i_act_bwd(c, g, y):
    return N.adjoint(lambda t: F.leaky_relu(t, c['slope']) * c['gain'], y.detach(), g)


def i_colsum(c, g):
    return g.reshape(-1, g.shape[-1]).sum(0)


def i_conv_bias_act(c, x, wp, bias):
    y = F.conv2d(_nchw(x), _oihw(wp, c['K'], c['C'], c['k']), bias, stride=c['s'], padding=c['p'])
    return _nhwc(F.leaky_relu(y, c['slope']) * c['gain'])


def i_rgb_conv(c, img, wp):
    return _nhwc(F.conv2d(img * c['a'] + c['b'], _oihw(wp, c['K'], 3, c['k']), padding=c['k'] // 2))


def i_rgb_dgrad(c, g, wp):
    return c['a'] * F.conv_transpose2d(_nchw(g), _oihw(wp, c['K'], 3, c['k']), padding=c['k'] // 2)


def i_rgb_wgrad(c, img, g):
    w0 = torch.zeros(c['K'], 3, c['k'], c['k'], dtype=f64)
    dw = N.adjoint(lambda w: _nhwc(F.conv2d(img * c['a'] + c['b'], w, padding=c['k'] // 2)), w0, g)
    return _packed(dw, N.round4(c['K']))


def i_rgb_conv_bias_act(c, img, wp, bias):
    y = F.conv2d(img * c['a'] + c['b'], _oihw(wp, c['K'], 3, c['k']), bias, padding=c['k'] // 2)
    return _nhwc(F.leaky_relu(y, c['slope']) * c['gain'])


def i_upfirdn(c, x, kernel):
    """upfirdn2d from its definition, tap by tap: out[i, j] = sum_ab xp[i * down + a, j * down + b] * k[kh-1-a, kw-1-b] on
    the zero-stuffed input xp padded (negative pads crop)."""
    u, d = c['up'], c['down']
    px0, px1, py0, py1 = c['pad']
    B, H, W, C = x.shape
    kh, kw = kernel.shape
    up = torch.zeros(B, H * u, W * u, C, dtype=f64)
    up[:, ::u, ::u] = x
    xp = F.pad(up, (0, 0, max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)))
    xp = xp[:, max(-py0, 0):xp.shape[1] - max(-py1, 0), max(-px0, 0):xp.shape[2] - max(-px1, 0)]
    oh, ow = (xp.shape[1] - kh) // d + 1, (xp.shape[2] - kw) // d + 1
    out = 0
    for a in range(kh):
        for b in range(kw):
            out = out + xp[:, a:a + (oh - 1) * d + 1:d, b:b + (ow - 1) * d + 1:d] * kernel[kh - 1 - a, kw - 1 - b]
    return out


def i_upfirdn_bwd(c, gy, kernel):
    x0 = torch.zeros(gy.shape[0], c['in_hw'][0], c['in_hw'][1], gy.shape[3], dtype=f64)
    return N.adjoint(lambda x: i_upfirdn(c, x, kernel), x0, gy)


def _i_mbstd(c, x):
    from contrad_amd.models.gan.stylegan2.discriminator import minibatch_stddev_nhwc
    return torch.cat([minibatch_stddev_nhwc(t) for t in torch.split(x, list(c['splits'] or [x.shape[0]]), 0)], 0)


def i_mbstd(c, x):
    return _i_mbstd(c, x)


def i_mbstd_bwd(c, x, gy):
    return N.adjoint(lambda t: _i_mbstd(c, t), x, gy)


def i_sumsq(c, g):
    return g.pow(2).reshape(g.shape[0], -1).sum(1).mean()


def i_lincomb(c, x, z):
    return c['a'] * x + c['b'] * z


def _as4(w):
    return w if w.dim() == 4 else w[:, :, None, None]


def i_pack(c, *ws):
    outs = [torch.zeros(g, dtype=f64) for g in c['groups']]
    for (K, C, T, scale, grp, off), w in zip(c['entries'], ws):
        outs[grp][:, off:off + K] = ops.pack_weight(_as4(w))[:, :K] * scale
    return tuple(outs)


def i_unpack(c, *gouts):
    res = []
    for (K, C, T, scale, grp, off), shape in zip(c['entries'], c['shapes']):
        k = int(round(T ** 0.5))
        res.append(ops.unpack_weight(gouts[grp][:, off:off + K], K, C, k, k).reshape(shape) * scale)
    return tuple(res)


def i_sn_pack(c, *t):
    """torch.nn.utils.spectral_norm itself (one power iteration in training mode), its weight packed."""
    n = len(c['kcts'])
    outs = []
    for w, u, v, shape, (K, C, T) in zip(t[:n], t[n:2 * n], t[2 * n:], c['shapes'], c['kcts']):
        m = torch.nn.Conv2d(shape[1], shape[0], shape[2]) if len(shape) == 4 else torch.nn.Linear(shape[1], shape[0])
        m = torch.nn.utils.spectral_norm(m.double(), n_power_iterations=1, eps=1e-12).train(c['training'])
        del m._parameters['weight_orig']
        m.weight_orig = w                                   # (the graph leaf of the protocol)
        m.weight_u.copy_(u)
        m.weight_v.copy_(v)
        for hook in m._forward_pre_hooks.values():
            hook(m, None)
        outs.append(F.pad(D.pack(m.weight.reshape(K, C * T), C, T), (0, N.round4(K) - K)))
    return tuple(outs)


def i_nhwc_scale(c, x, s):
    return x * s[:, None, None, :]


def i_modconv_epilogue(c, y, demod, noise, noise_w, bias):
    pre = y * demod[:, None, None, :] + noise_w * noise.permute(0, 2, 3, 1) + bias
    return F.leaky_relu(pre, 0.2) * 2.0 ** 0.5


INDEPENDENT = {
    'Conv2dFn': i_conv2d, 'ConvDgradFn': i_dgrad, 'ConvWgradFn': i_wgrad, 'ConvWgradBiasFn': i_wgrad_bias, 'ActFn': i_act,
    'ActBwdFn': i_act_bwd, 'ColSumFn': i_colsum, 'ConvBiasActFn': i_conv_bias_act, 'RgbConvFn': i_rgb_conv,
    'RgbDgradFn': i_rgb_dgrad, 'RgbWgradFn': i_rgb_wgrad, 'RgbConvBiasActFn': i_rgb_conv_bias_act, 'UpFirDn2dFn': i_upfirdn,
    'UpFirDn2dBackwardFn': i_upfirdn_bwd, 'MinibatchStddevFn': i_mbstd, 'MinibatchStddevBwdFn': i_mbstd_bwd,
    'SumSqMeanFn': i_sumsq, 'LinCombFn': i_lincomb, 'PackWeightsFn': i_pack, 'UnpackWeightsFn': i_unpack,
    'SnPackWeightsFn': i_sn_pack, 'NhwcScaleFn': i_nhwc_scale, 'ModconvEpilogueFn': i_modconv_epilogue,
}


def _protocol64(case, fn, drop=None):
    return N.protocol(fn, N.inputs(case), N.diff_flags(case), N.drawer(case), N.SPECS[case['node']][3], f64, 'cpu', drop)


@pytest.fixture(scope='module')
def refs():
    """The float64 reference of every small case, computed once: (results, smallest |pre-activation|)."""
    return {c['id']: N.reference(c) for c in SMALL}


@pytest.mark.parametrize('case', SMALL, ids=lambda c: c['id'])
def test_twin_matches_torchs_own_float64_operators(case, refs):
    assert set(N.SPECS) == set(INDEPENDENT)
    c = case['cfg']
    other = _protocol64(case, lambda *t: INDEPENDENT[case['node']](c, *t))
    ref = refs[case['id']][0]
    assert set(other) == set(ref)
    seen = 0
    for key, order, emax, el2, exact in N.compare(other, ref):
        assert emax < TIGHT and el2 < TIGHT, (case['id'], key, emax, el2)
        seen += not exact
    assert seen >= 2                                     # (a value and at least one gradient are not structurally zero)


def test_multi_output_twins_with_one_cotangent_missing(refs):
    for cid, drop in (('ConvWgradBiasFn-k3s1p1', 0), ('ConvWgradBiasFn-k3s1p1', 1), ('PackWeightsFn-3in2', 1),
                      ('UnpackWeightsFn-3in2', 2)):
        case = N.BY_ID[cid]
        ref = N.reference(case, drop=drop)[0]
        other = _protocol64(case, lambda *t: INDEPENDENT[case['node']](case['cfg'], *t), drop=drop)
        for key, order, emax, el2, exact in N.compare(other, ref):
            assert emax < TIGHT and el2 < TIGHT, (cid, drop, key, emax, el2)


def test_sn_twin_gradient_is_dstep_ref64_sn_grad():
    """The native-autograd gradient of the twin is the closed form the kernel test uses (dstep_ref64.sn_grad)."""
    for training in (True, False):
        case = N.BY_ID['SnPackWeightsFn-%s' % ('train' if training else 'eval')]
        c = case['cfg']
        t = [x.to(f64) for x in N.inputs(case)]
        n = len(c['kcts'])
        ws = [w.clone().requires_grad_() for w in t[:n]]
        outs, state = N.sn_pack(ws, t[n:2 * n], t[2 * n:], c['kcts'], training)
        gs = [torch.randn(o.shape, dtype=f64, generator=torch.Generator().manual_seed(3)) for o in outs]
        gws = torch.autograd.grad(outs, ws, gs)
        for w, gw, g, (u, v, sigma), (K, C, T) in zip(ws, gws, gs, state, c['kcts']):
            want = D.sn_grad(D.unpack(g, K, C, T), w.detach().reshape(K, C * T), u, v)
            assert D.errors(gw.reshape(K, C * T), want)[0] < TIGHT


def test_every_activated_case_keeps_clear_of_the_kink(refs):
    checked = 0
    for case in N.CASES:
        if case['node'] in N.ACTIVATED:
            assert _small(case)
            lo = refs[case['id']][1]
            assert lo >= N.GUARD, (case['id'], lo)
            assert lo < 1.0                                 # (the twin did report its pre-activation)
            checked += 1
        elif _small(case):
            assert refs[case['id']][1] == float('inf'), case['id']
    assert checked >= 15


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _paths(L, case):
    n, H, W, C, K, k, s, p, ldw = N.conv_descs(case)
    d = _lib.ConvDesc(n, H, W, C, C, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, K, K, k, k, s, p, ldw)
    return tuple(L.raw('contrad_conv2d_path')(ctypes.byref(d), mode) for mode in (0, 1, 2))


def test_the_conv_cases_reach_winograd_and_every_direct_path(L):
    """Forward, backward and double backward of a conv root call the engine in all three modes on one geometry."""
    conv = [c for c in N.CASES if c['node'] in ('Conv2dFn', 'ConvDgradFn', 'ConvWgradFn', 'ConvWgradBiasFn', 'ConvBiasActFn')]
    seen = set()
    for case in conv:
        paths = _paths(L, case)
        assert min(paths) >= 0, (case['id'], paths)
        seen |= {(mode, P) for mode, P in enumerate(paths)}
        worst = max(paths)
        want = 'conv F(4x4)' if worst in (9, 11) else 'conv Winograd' if worst >= 7 else 'conv direct'
        assert case['cls'] == want, (case['id'], paths)      # (a case is judged by the bound of the loosest family it calls)
    for mode in (0, 1, 2):
        assert any(m == mode and P >= 7 for m, P in seen), 'no Winograd-planned call in mode %d' % mode
    assert {P for _, P in seen} >= {0, 1, 2, 3, 5}, sorted(seen)
    assert any(P in (9, 11) for _, P in seen) and any(P == 8 for _, P in seen)


# ---- sensitivity: one wrong arrow in a backward ----------------------------------------------------------------------
def _mutants():
    from torch.autograd import Function

    def rgb_dgrad_b(case):
        c = case['cfg']
        wrong = dict(c, b=0.5)                               # RgbDgradFn.backward: (k, a, b) with b != 0 for (k, scale, 0)

        class Mut(Function):
            @staticmethod
            def forward(ctx, g, wp):
                ctx.save_for_backward(g, wp)
                return N.t_rgb_dgrad(c, g, wp)

            @staticmethod
            def backward(ctx, h):
                g, wp = ctx.saved_tensors
                return N.t_rgb_conv(wrong, h, wp), N.t_rgb_wgrad(dict(c, b=0.0), h, g)
        return Mut.apply

    def g_pad_off_by_one(case):
        c = case['cfg']
        gp = c['g_pad']
        shifted = dict(c, up=c['down'], down=c['up'], pad=(gp[0] + 1, gp[1] - 1, gp[2], gp[3]))

        class Mut(Function):
            @staticmethod
            def forward(ctx, x, kernel):
                ctx.save_for_backward(kernel)
                return N.t_upfirdn(c, x, kernel)

            @staticmethod
            def backward(ctx, gy):
                kernel, = ctx.saved_tensors
                return N.t_upfirdn(shifted, gy, torch.flip(kernel, [0, 1])), None
        return Mut.apply

    return [
        ('ConvDgradFn.backward without its weight gradient', 'ConvDgradFn-k3s1p1',
         lambda case: lambda gy, wp: N.t_dgrad(case['cfg'], gy, wp.detach())),
        ('RgbDgradFn.backward with a shift', 'RgbDgradFn-k3-a2', rgb_dgrad_b),
        ('g_pad off by one', 'UpFirDn2dFn-blur22', g_pad_off_by_one),
        ('ActBwdFn reads the region from the gradient', 'ActBwdFn-a0',
         lambda case: lambda g, y: N.act_bwd(g, g, case['cfg']['slope'], case['cfg']['gain'])),
        ('ConvWgradBiasFn.backward drops hb', 'ConvWgradBiasFn-k3s1p1',
         lambda case: lambda x, gy: (N.t_wgrad(case['cfg'], x, gy), gy.detach().sum((0, 1, 2)) + 0.0 * gy.sum((0, 1, 2)))),
        ('UnpackWeightsFn without the scale', 'UnpackWeightsFn-3in2',
         lambda case: lambda *g: N.unpack_groups(case['cfg']['entries'], case['cfg']['shapes'], g, scaled=False)),
    ]


@pytest.mark.parametrize('what,cid,make', _mutants(), ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else None)
def test_the_protocol_sees_one_wrong_arrow(what, cid, make, refs):
    case = N.BY_ID[cid]
    tol = _gpu_module().TOL[case['cls']]
    bound = max(max(t) for t in tol.values())
    mutated = _protocol64(case, make(case))
    worst = max(emax for key, order, emax, el2, exact in N.compare(mutated, refs[cid][0]))
    assert worst > 100 * bound, (what, worst, bound)
    # (and the right twin passes its own protocol exactly: the error above is the mutation's)
    again = _protocol64(case, N.twin(case))
    assert max(emax for _, _, emax, _, _ in N.compare(again, refs[cid][0])) == 0.0
    N.guard_min()


def test_every_function_class_has_a_case():
    """A node added to autograd_ops.py without a case in the GPU test fails here."""
    src = open(os.path.join(os.path.dirname(_HERE), 'contrad_amd', 'autograd_ops.py')).read()
    classes = set(re.findall(r'^class (\w+)\(Function\)', src, re.M))
    M = _gpu_module()
    text = open(os.path.join(_HERE, 'test_autograd_nodes_gpu.py')).read()
    assert classes == set(M.HIP) | set(M.BEHAVIOUR_ONLY), classes ^ (set(M.HIP) | set(M.BEHAVIOUR_ONLY))
    assert set(M.HIP) == set(N.SPECS) == {c['node'] for c in N.CASES}
    for name in classes | {'exchange_packed', 'input_grad_only'}:
        assert re.search(r'\b%s\b' % name, text), name
    for cls in {c['cls'] for c in N.CASES}:
        assert set(M.TOL[cls]) == {0, 1, 2}
