"""Differentiable float64 twins of the any-order autograd nodes (contrad_amd/autograd_ops.py) and the parity protocol
that compares a node with its twin to second order.

A twin is a plain-torch function on float64 tensors that torch's NATIVE autograd differentiates: no ``Function`` subclass
and none of this project's kernels.  It takes the fp32 tensors the node read, cast to float64, on whatever device they
live on.  The formulas are those of the existing references: the unfold / fold + matmul convolution of conv_ref64.py
(written here without in-place operations on graph tensors, so that it differentiates), dstep_ref64's pack / unpack /
sn_prep / rgb_*, sg2_ref64's upfirdn2d, minibatch-stddev and modconv epilogue.  A packed weight is OIHW float64 behind the
pack / unpack permutation: the padding columns (ldw > K) of a packed tensor carry no gradient and come back as zeros.

Leaky-ReLU twins take their linear region from the float64 pre-activation; every case with an activation therefore has to
keep the reference's smallest |pre-activation| above GUARD (``guard_min``; tests/test_nodes_ref64_cpu.py asserts it for
every case of the table on exactly the inputs the GPU test uses: the table is built with CPU generators).

``protocol(fn, ...)`` is the same code for the HIP node and for the twin:
    out = fn(a...); r = cotangents (leaves); g = grad(out, a, r, create_graph=True); s = grad(g, (a..., r...), h)
and returns {'out0'.., 'g0'.., 's0'..} (None where autograd gives None).  tests/test_autograd_nodes_gpu.py compares the
two dictionaries on whole tensors; tests/test_nodes_ref64_cpu.py checks the twins against torch's own float64 operators.
"""
import math

import torch
import torch.nn.functional as F

import dstep_ref64 as D
import sg2_ref64 as S

f64 = torch.float64
GUARD = 1e-5                      # smallest |pre-activation| a case may have (about 100x the kernels' fp32 error at O(1))
PAD_FILL = 1e3                    # what the padding columns of a packed COTANGENT hold in the cases that say so


def f32(v):
    """The fp32 value a kernel receives for a Python scalar."""
    return float(torch.tensor(float(v), dtype=torch.float32))


SQRT2 = f32(math.sqrt(2.0))
_PRE = []                         # min |pre-activation| of every activation a twin evaluated since the last guard_min()


def _note(pre):
    _PRE.append(float(pre.detach().abs().min()))


def round4(v):
    return (v + 3) // 4 * 4


# ---- primitives ------------------------------------------------------------------------------------------------------
def unpack_w(wp, K, C, KH, KW):
    """Packed [(tap, c)][ldw] -> OIHW (the padding columns are not read)."""
    return D.unpack(wp, K, C, KH * KW).reshape(K, C, KH, KW)


def pack_w(w, ldw):
    """OIHW -> packed [(tap, c)][ldw], padding columns zero."""
    K, C, KH, KW = w.shape
    return F.pad(D.pack(w.reshape(K, C * KH * KW), C, KH * KW), (0, ldw - K))


def conv(x, w, s, p):
    """x (N,H,W,C), w OIHW -> y (N,Ho,Wo,K): conv_ref64.fwd without its epilogue."""
    N, H, W, C = x.shape
    K, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
    cols = F.unfold(x.permute(0, 3, 1, 2), (KH, KW), padding=p, stride=s)
    return torch.matmul(w.reshape(K, -1), cols).transpose(1, 2).reshape(N, Ho, Wo, K)


def conv_dgrad(gy, w, x_hw, s, p):
    """gy (N,Ho,Wo,K), w OIHW -> dx (N,H,W,C): conv_ref64.dgrad."""
    N, Ho, Wo, K = gy.shape
    _, C, KH, KW = w.shape
    cols = torch.matmul(w.reshape(K, -1).t(), gy.reshape(N, Ho * Wo, K).transpose(1, 2))
    return F.fold(cols, tuple(x_hw), (KH, KW), padding=p, stride=s).permute(0, 2, 3, 1)


def conv_wgrad(x, gy, KH, KW, s, p):
    """x (N,H,W,C), gy (N,Ho,Wo,K) -> dw OIHW: conv_ref64.wgrad."""
    N, H, W, C = x.shape
    K = gy.shape[3]
    cols = F.unfold(x.permute(0, 3, 1, 2), (KH, KW), padding=p, stride=s)
    g = gy.reshape(N, -1, K).transpose(1, 2)
    return torch.matmul(g, cols.transpose(1, 2)).sum(0).reshape(K, C, KH, KW)


def lrelu(pre, slope, gain):
    _note(pre)
    return torch.where(pre > 0, pre, pre * slope) * gain


def act_bwd(g, region, slope, gain):
    """g * gain * lrelu'(region): the region tensor is a constant of the graph."""
    _note(region)
    one = torch.ones((), dtype=f64, device=g.device)
    return g * torch.where(region.detach() > 0, one * gain, one * (gain * slope))


def adjoint(fn, x_like, gy):
    """<fn(x), gy> differentiated at x by native autograd, differentiable in gy (and in x): the transpose of a linear op,
    or the backward of a non-linear one, without writing either down."""
    x = x_like if x_like.requires_grad else x_like.detach().requires_grad_()
    return torch.autograd.grad(fn(x), x, gy, create_graph=True)[0]


def blur_kernel(taps, gain=1.0):
    k = torch.tensor(taps, dtype=torch.float32)
    k = k[None, :] * k[:, None]
    return k / k.sum() * gain


def mbstd(x, cpad, splits):
    B, H, W, C = x.shape
    parts = [S.mbstd_forward(t.reshape(t.shape[0], H * W, C), t.shape[0], H * W, C, cpad)
             for t in torch.split(x, list(splits or [B]), dim=0)]
    return torch.cat(parts, 0).reshape(B, H, W, cpad)


def pack_groups(entries, groups, ws, scaled=True):
    """PackWeightsFn: one (rows, cols) tensor per group, entry i = pack(w_i) * scale_i at its column offset, zeros elsewhere."""
    outs = []
    for gi, (rows, cols) in enumerate(groups):
        pieces, at = [], 0
        for (K, C, T, scale, grp, off), w in sorted(((e, w) for e, w in zip(entries, ws) if e[4] == gi), key=lambda t: t[0][5]):
            pieces.append(torch.zeros(rows, off - at, dtype=f64, device=w.device))
            pieces.append(D.pack(w.reshape(K, C * T), C, T) * (scale if scaled else 1.0))
            at = off + K
        pieces.append(torch.zeros(rows, cols - at, dtype=f64, device=ws[0].device))
        outs.append(torch.cat(pieces, 1))
    return tuple(outs)


def unpack_groups(entries, shapes, gouts, scaled=True):
    """UnpackWeightsFn: w-shaped gradients * scale from the packed per-group gradients."""
    return tuple(D.unpack(gouts[grp][:, off:off + K], K, C, T).reshape(shape) * (scale if scaled else 1.0)
                 for (K, C, T, scale, grp, off), shape in zip(entries, shapes))


def sn_pack(ws, us, vs, kcts, training):
    """SnPackWeightsFn: W / sigma packed, sigma = u^T W v with the u, v of THIS forward as constants of the graph (what
    torch.nn.utils.spectral_norm's autograd sees).  -> (packed outputs, [(u', v', sigma)])."""
    outs, state = [], []
    for w, u, v, (K, C, T) in zip(ws, us, vs, kcts):
        w2 = w.reshape(K, C * T)
        _, u2, v2, _ = D.sn_prep(w2.detach(), u, v, training)
        sigma = torch.dot(u2, w2 @ v2)
        outs.append(F.pad(D.pack(w2 / sigma, C, T), (0, round4(K) - K)))
        state.append((u2, v2, sigma.detach()))
    return tuple(outs), state


# ---- twins: twin(cfg, *float64 inputs) -> output or tuple of outputs -------------------------------------------------
def _geo(c):
    Ho, Wo = (c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1
    return Ho, Wo, c.get('ldw', round4(c['K']))


def _w(c, wp):
    return unpack_w(wp, c['K'], c['C'], c['k'], c['k'])


def t_conv2d(c, x, wp):
    return conv(x, _w(c, wp), c['s'], c['p'])


def t_dgrad(c, gy, wp):
    return conv_dgrad(gy, _w(c, wp), (c['H'], c['W']), c['s'], c['p'])


def t_wgrad(c, x, gy):
    return pack_w(conv_wgrad(x, gy, c['k'], c['k'], c['s'], c['p']), _geo(c)[2])


def t_wgrad_bias(c, x, gy):
    return t_wgrad(c, x, gy), gy.sum((0, 1, 2))


def t_act(c, x):
    return lrelu(x, c['slope'], c['gain'])


def t_act_bwd(c, g, y):
    return act_bwd(g, y, c['slope'], c['gain'])


def t_colsum(c, g):
    return g.sum(tuple(range(g.dim() - 1)))


def t_conv_bias_act(c, x, wp, bias):
    return lrelu(conv(x, _w(c, wp), c['s'], c['p']) + bias, c['slope'], c['gain'])


def _rgb_w(c, wp):
    return unpack_w(wp, c['K'], 3, c['k'], c['k'])


def t_rgb_conv(c, img, wp):
    return D.rgb_fwd(img, _rgb_w(c, wp), None, c['a'], c['b'], 1.0, 1.0)


def t_rgb_dgrad(c, g, wp):
    return D.rgb_dgrad(g, _rgb_w(c, wp), None, 0, c['a'])


def t_rgb_wgrad(c, img, g):
    return pack_w(D.rgb_wgrad(img, g, c['k'], c['a'], c['b'])[0], round4(c['K']))


def t_rgb_conv_bias_act(c, img, wp, bias):
    return lrelu(D.rgb_fwd(img, _rgb_w(c, wp), bias, c['a'], c['b'], 1.0, 1.0), c['slope'], c['gain'])


def t_upfirdn(c, x, kernel):
    u, d = c['up'], c['down']
    return S.upfirdn2d(x, kernel, u, u, d, d, *c['pad'])


def t_upfirdn_bwd(c, gy, kernel):
    B, C = gy.shape[0], gy.shape[3]
    x0 = torch.zeros(B, c['in_hw'][0], c['in_hw'][1], C, dtype=f64, device=gy.device)
    return adjoint(lambda x: t_upfirdn(c, x, kernel), x0, gy)


def t_mbstd(c, x):
    return mbstd(x, c['cpad'], c['splits'])


def t_mbstd_bwd(c, x, gy):
    return adjoint(lambda t: mbstd(t, gy.shape[3], c['splits']), x, gy)


def t_sumsq(c, g):
    return S.sumsq(g, 1.0 / g.shape[0])


def t_lincomb(c, x, z):
    return S.lincomb(x, z, c['a'], c['b'])


def t_pack(c, *ws):
    return pack_groups(c['entries'], c['groups'], ws)


def t_unpack(c, *gouts):
    return unpack_groups(c['entries'], c['shapes'], gouts)


def t_sn_pack(c, *t):
    n = len(c['kcts'])
    return sn_pack(t[:n], t[n:2 * n], t[2 * n:], c['kcts'], c['training'])[0]


def t_nhwc_scale(c, x, s):
    N, H, W, C = x.shape
    return S.nhwc_scale(x, s, N, H * W, C).reshape(x.shape)


def t_modconv_epilogue(c, y, demod, noise, noise_w, bias):
    N = y.shape[0]
    _note(y * demod.view(N, 1, 1, -1) + noise_w[0] * noise.reshape(N, y.shape[1], y.shape[2], 1) + bias)
    return S.modconv_epilogue(y, bias, demod, noise, noise_w)


# ---- inputs: make(cfg, generator) -> fp32 CPU tensors ----------------------------------------------------------------
def _r(g, *shape):
    return torch.randn(*shape, generator=g)


def _wp(g, K, C, k, ldw):
    w = _r(g, K, C, k, k) / math.sqrt(C * k * k)
    return pack_w(w.to(f64), ldw).float().contiguous()


def m_conv2d(c, g):
    return [_r(g, c['N'], c['H'], c['W'], c['C']), _wp(g, c['K'], c['C'], c['k'], _geo(c)[2])]


def m_dgrad(c, g):
    Ho, Wo, ldw = _geo(c)
    return [_r(g, c['N'], Ho, Wo, c['K']), _wp(g, c['K'], c['C'], c['k'], ldw)]


def m_wgrad(c, g):
    Ho, Wo, _ = _geo(c)
    return [_r(g, c['N'], c['H'], c['W'], c['C']), _r(g, c['N'], Ho, Wo, c['K'])]


def m_one(c, g):
    return [_r(g, *c['shape'])]


def m_two(c, g):
    return [_r(g, *c['shape']), _r(g, *c['shape'])]


def m_conv_bias_act(c, g):
    return m_conv2d(c, g) + [_r(g, c['K']) * 0.3]


def m_rgb_conv(c, g):
    return [_r(g, c['N'], 3, c['H'], c['W']), _wp(g, c['K'], 3, c['k'], round4(c['K']))]


def m_rgb_dgrad(c, g):
    return [_r(g, c['N'], c['H'], c['W'], c['K']), _wp(g, c['K'], 3, c['k'], round4(c['K']))]


def m_rgb_wgrad(c, g):
    return [_r(g, c['N'], 3, c['H'], c['W']), _r(g, c['N'], c['H'], c['W'], c['K'])]


def m_rgb_conv_bias_act(c, g):
    return m_rgb_conv(c, g) + [_r(g, c['K']) * 0.3]


def m_upfirdn(c, g):
    return [_r(g, *c['shape']), blur_kernel(c['taps'], c.get('kgain', 1.0))]


def m_mbstd_bwd(c, g):
    B, H, W, C = c['shape']
    return [_r(g, B, H, W, C), _r(g, B, H, W, c['cpad'])]


def m_pack(c, g):
    return [_r(g, *s) for s in c['shapes']]


def m_unpack(c, g):
    outs = []
    for gi, (rows, cols) in enumerate(c['groups']):
        t = torch.full((rows, cols), PAD_FILL)
        for (K, C, T, scale, grp, off) in c['entries']:
            if grp == gi:
                t[:, off:off + K] = _r(g, rows, K)
        outs.append(t)
    return outs


def m_sn_pack(c, g):
    ws = [_r(g, *s) / math.sqrt(C * T) for s, (K, C, T) in zip(c['shapes'], c['kcts'])]
    us = [F.normalize(_r(g, K), dim=0) for (K, C, T) in c['kcts']]
    vs = [F.normalize(_r(g, C * T), dim=0) for (K, C, T) in c['kcts']]
    return ws + us + vs


def m_nhwc_scale(c, g):
    N, H, W, C = c['shape']
    return [_r(g, N, H, W, C), _r(g, N, C)]


def m_modconv_epilogue(c, g):
    N, H, W, K = c['shape']
    return [_r(g, N, H, W, K), _r(g, N, K).abs() + 0.5, _r(g, N, 1, H, W), _r(g, 1) * 0.5 + 1.0, _r(g, K) * 0.3]


def _fill_packed(c, K):
    def fix(t):
        if c.get('padfill') and t.dim() == 2 and t.shape[1] > K:
            t[:, K:] = PAD_FILL
        return t
    return fix


# node -> (make, differentiable inputs, twin, highest order, indices of PACKED conv-weight tensors among
#          (outputs, inputs): their cotangents / directions get PAD_FILL in the padding columns when the case says so)
SPECS = {
    'Conv2dFn': (m_conv2d, (1, 1), t_conv2d, 2, ((), (1,))),
    'ConvDgradFn': (m_dgrad, (1, 1), t_dgrad, 2, ((), (1,))),
    'ConvWgradFn': (m_wgrad, (1, 1), t_wgrad, 2, ((0,), ())),
    'ConvWgradBiasFn': (m_wgrad, (1, 1), t_wgrad_bias, 2, ((0,), ())),
    'ActFn': (m_one, (1,), t_act, 2, ((), ())),
    'ActBwdFn': (m_two, (1, 0), t_act_bwd, 2, ((), ())),
    'ColSumFn': (m_one, (1,), t_colsum, 2, ((), ())),
    'ConvBiasActFn': (m_conv_bias_act, (1, 1, 1), t_conv_bias_act, 2, ((), (1,))),
    'RgbConvFn': (m_rgb_conv, (1, 1), t_rgb_conv, 2, ((), ())),
    'RgbDgradFn': (m_rgb_dgrad, (1, 1), t_rgb_dgrad, 2, ((), ())),
    'RgbWgradFn': (m_rgb_wgrad, (1, 1), t_rgb_wgrad, 2, ((), ())),
    'RgbConvBiasActFn': (m_rgb_conv_bias_act, (1, 1, 1), t_rgb_conv_bias_act, 2, ((), ())),
    'UpFirDn2dFn': (m_upfirdn, (1, 0), t_upfirdn, 2, ((), ())),
    'UpFirDn2dBackwardFn': (m_upfirdn, (1, 0), t_upfirdn_bwd, 2, ((), ())),
    'MinibatchStddevFn': (m_one, (1,), t_mbstd, 2, ((), ())),
    'MinibatchStddevBwdFn': (m_mbstd_bwd, (1, 1), t_mbstd_bwd, 1, ((), ())),      # (its second order is the forward's third)
    'SumSqMeanFn': (m_one, (1,), t_sumsq, 1, ((), ())),
    'LinCombFn': (m_two, (1, 1), t_lincomb, 2, ((), ())),
    'PackWeightsFn': (m_pack, None, t_pack, 2, ((), ())),
    'UnpackWeightsFn': (m_unpack, None, t_unpack, 2, ((), ())),
    'SnPackWeightsFn': (m_sn_pack, None, t_sn_pack, 1, ((), ())),
    'NhwcScaleFn': (m_nhwc_scale, (1, 1), t_nhwc_scale, 1, ((), ())),
    'ModconvEpilogueFn': (m_modconv_epilogue, (1, 1, 0, 1, 1), t_modconv_epilogue, 1, ((), ())),
}
ACTIVATED = ('ActFn', 'ActBwdFn', 'ConvBiasActFn', 'RgbConvBiasActFn', 'ModconvEpilogueFn')


def diff_flags(case):
    node, c = case['node'], case['cfg']
    flags = SPECS[node][1]
    if flags is not None:
        return flags
    if node == 'SnPackWeightsFn':
        n = len(c['kcts'])
        return (1,) * n + (0,) * (2 * n)
    return (1,) * (len(c['shapes']) if node == 'PackWeightsFn' else len(c['groups']))


def inputs(case):
    """The fp32 CPU tensors the node reads, from the case's own seed."""
    return SPECS[case['node']][0](case['cfg'], torch.Generator().manual_seed(case['seed']))


def twin(case):
    fn, c = SPECS[case['node']][2], case['cfg']
    return lambda *t: fn(c, *t)


def drawer(case):
    """draw(shapes) -> fp32 CPU standard-normal tensors from the case's second generator: the cotangents, then the
    second-order directions.  Packed conv weights get PAD_FILL in their padding columns where the case asks for it."""
    g = torch.Generator().manual_seed(case['seed'] + 7919)
    c = case['cfg']
    fix = _fill_packed(c, c.get('K', 0))
    packed_out, packed_in = SPECS[case['node']][4]

    def draw(shapes, what):
        ts = [_r(g, *s) if len(s) else _r(g, 1)[0] for s in shapes]
        marked = packed_out if what == 'cot' else packed_in
        return [fix(t) if i in marked else t for i, t in enumerate(ts)]
    return draw


def guard_min():
    """Smallest |pre-activation| any activation twin has seen since the last call."""
    m = min(_PRE) if _PRE else float('inf')
    del _PRE[:]
    return m


# ---- the protocol ----------------------------------------------------------------------------------------------------
def protocol(fn, ins, diff, draw, order=2, dtype=torch.float32, device=None, drop=None):
    """Steps 1 - 5 of the parity protocol on ``fn`` (a HIP node or a twin).  ``ins``: fp32 tensors; ``draw``: see drawer();
    ``drop``: index of an output that gets no cotangent.  -> dict of detached results, None where autograd gives None."""
    device = device or ins[0].device
    a = [t.detach().to(device, dtype).clone().requires_grad_(bool(d)) for t, d in zip(ins, diff)]
    out = fn(*a)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    res = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    act = [a[i] for i, d in enumerate(diff) if d]
    idx = [i for i, d in enumerate(diff) if d]
    r = [t.to(device, dtype).requires_grad_() for t in draw([tuple(o.shape) for o in outs], 'cot')]
    hs = [t.to(device, dtype) for t in draw([tuple(t.shape) for t in a], 'dir')]
    keep = [i for i in range(len(outs)) if i != drop]
    g = torch.autograd.grad([outs[i] for i in keep], act, [r[i] for i in keep], create_graph=order > 1, allow_unused=True)
    for i, gi in zip(idx, g):
        res['g%d' % i] = None if gi is None else gi.detach()
    if order < 2:
        return res
    live = [(gi, hs[i]) for i, gi in zip(idx, g) if gi is not None and gi.requires_grad]
    wrt = act + [r[i] for i in keep]
    names = ['s%d' % i for i in idx] + ['sr%d' % i for i in keep]
    if live:
        s = torch.autograd.grad([t[0] for t in live], wrt, [t[1] for t in live], allow_unused=True)
    else:
        s = [None] * len(wrt)
    for n, si in zip(names, s):
        res[n] = None if si is None else si.detach()
    return res


def reference(case, device='cpu', drop=None):
    """The protocol on the float64 twin.  -> (results, smallest |pre-activation| seen)."""
    guard_min()
    res = protocol(twin(case), inputs(case), diff_flags(case), drawer(case), SPECS[case['node']][3], f64, device, drop)
    return res, guard_min()


def compare(res, ref):
    """Rows (key, order, max-norm error, rel-L2 error, exact) of a protocol result against the twin's.  Where the twin gives
    None or an all-zero tensor the other side must give None or exact zeros (``exact`` rows: error 0, or inf when it does
    not); a gradient that is missing where the twin has one counts as an error of 1."""
    rows = []
    for key, want in ref.items():
        got = res[key]
        order = 0 if key.startswith('out') else 1 if key.startswith('g') else 2
        if want is None or not bool(want.ne(0).any()):
            bad = got is not None and bool(got.ne(0).any())
            rows.append((key, order, float('inf') if bad else 0.0, float('inf') if bad else 0.0, True))
        elif got is None:
            rows.append((key, order, 1.0, 1.0, False))
        else:
            assert tuple(got.shape) == tuple(want.shape), (key, got.shape, want.shape)
            emax, el2 = D.errors(got, want)
            rows.append((key, order, emax, el2, False))
    return rows


# ---- the case table --------------------------------------------------------------------------------------------------
def _conv(N, H, W, C, K, k, s, p, **kw):
    return dict(N=N, H=H, W=W, C=C, K=K, k=k, s=s, p=p, **kw)


# geometries the models use, at the smallest maps (tag, cfg)
CONV_GEOMS = [
    ('k3s1p1', _conv(2, 5, 7, 8, 8, 3, 1, 1)),                          # odd non-square map; C, K % 4 == 0: fused bias
    ('k4s2p1', _conv(2, 8, 8, 8, 12, 4, 2, 1)),                         # SNDCGAN; generator dgrad x_shape 2H
    ('k3s2p0', _conv(2, 9, 9, 8, 8, 3, 2, 0)),                          # StyleGAN2 downsample on the blurred odd map; 2H+1
    ('k3s2p1', _conv(2, 8, 8, 8, 16, 3, 2, 1)),                         # SNResNet
    ('k1s2p0', _conv(2, 8, 8, 8, 16, 1, 2, 0)),                         # SNResNet shortcut
    ('logit', _conv(3, 1, 1, 16, 1, 1, 1, 0)),                          # K = 1 on 1x1 maps (ldw 4 > K)
    ('head', _conv(3, 1, 1, 32, 64, 1, 1, 0)),
    ('k6', _conv(2, 4, 4, 5, 6, 3, 1, 1, padfill=True)),                # ldw 8 > K 6, C % 4 != 0: unfused bias branch
    ('rgb3', _conv(2, 5, 5, 3, 8, 3, 1, 1)),                            # C = 3: the scalar-gather kernels
    ('c128', _conv(16, 2, 2, 128, 8, 3, 1, 1)),                         # pixel-major wgrad tiles
]
# the smallest shapes the planner sends to a Winograd kernel in the forward / dgrad / wgrad call (Conv2dFn root only)
WINO_GEOMS = [
    ('wino-fwd', _conv(12, 32, 32, 16, 256, 3, 1, 1)),
    ('wino-dgrad', _conv(12, 32, 32, 256, 16, 3, 1, 1)),
    ('wino-wgrad', _conv(8, 32, 32, 256, 256, 3, 1, 1)),
    ('wino22-dgrad', _conv(24, 32, 32, 256, 16, 4, 2, 1)),
    ('f44-fwd', _conv(16, 32, 32, 32, 256, 3, 1, 1)),
    ('f44-dgrad', _conv(16, 32, 32, 256, 32, 3, 1, 1)),
]
ACTS = [(f32(0.2), SQRT2), (f32(0.1), 1.0), (1.0, 1.0)]
_PACK = dict(entries=[(8, 4, 9, 0.5, 0, 0), (4, 4, 9, 0.25, 0, 8), (8, 16, 1, 2.0, 1, 4)], groups=[(36, 16), (16, 12)],
             shapes=[(8, 4, 3, 3), (4, 4, 3, 3), (8, 16)])
_SN = dict(shapes=[(8, 4, 3, 3), (6, 32)], kcts=[(8, 4, 9), (6, 8, 4)])


def _cases():
    out = []

    def add(node, tag, cfg, cls, seed=0):
        out.append(dict(id='%s-%s' % (node, tag), node=node, cfg=cfg, cls=cls, seed=seed))

    for node in ('Conv2dFn', 'ConvDgradFn', 'ConvWgradFn', 'ConvWgradBiasFn'):
        for tag, c in CONV_GEOMS:
            if node == 'ConvWgradBiasFn' and (c['C'] % 4 or c['K'] % 4):
                continue                                              # (the launcher's argument error: asserted in the GPU test)
            add(node, tag, c, 'conv direct')
    for tag, c in WINO_GEOMS:
        add('Conv2dFn', tag, c, 'conv F(4x4)' if tag.startswith('f44') else 'conv Winograd')
    for i, (slope, gain) in enumerate(ACTS):
        a = dict(slope=slope, gain=gain)
        tag = 'a%d' % i
        add('ActFn', tag, dict(shape=(2, 5, 5, 12), **a), 'element-wise')
        add('ActBwdFn', tag, dict(shape=(2, 5, 5, 12), **a), 'element-wise')
        add('ConvBiasActFn', tag + '-k3s1p1', dict(CONV_GEOMS[0][1], **a), 'conv direct')
        add('ConvBiasActFn', tag + '-k6', dict(CONV_GEOMS[7][1], **a), 'conv direct')
        add('RgbConvBiasActFn', tag, dict(N=2, H=4, W=4, K=64, k=3, a=2.0, b=-1.0, **a), 'RGB')
    add('ConvBiasActFn', 'a0-k4s2p1', dict(CONV_GEOMS[1][1], slope=ACTS[0][0], gain=ACTS[0][1]), 'conv direct')
    add('ConvBiasActFn', 'a0-logit', dict(CONV_GEOMS[5][1], slope=ACTS[0][0], gain=ACTS[0][1]), 'conv direct')
    add('ColSumFn', 'k12', dict(shape=(3, 5, 5, 12)), 'element-wise')
    for node in ('RgbConvFn', 'RgbDgradFn', 'RgbWgradFn'):
        for k in (1, 3):
            for (a, b) in ((2.0, -1.0), (1.0, 0.0)):
                add(node, 'k%d-a%g' % (k, a), dict(N=2, H=4, W=4, K=64, k=k, a=a, b=b), 'RGB')
        add(node, 'k3-4x6', dict(N=3, H=4, W=6, K=16, k=3, a=2.0, b=-1.0), 'RGB')
    fir = dict(taps=(1, 3, 3, 1))
    ufd = [('blur22', dict(shape=(3, 9, 9, 8), up=1, down=1, pad=(2, 2, 2, 2), g_pad=(1, 1, 1, 1), **fir)),
           ('blur11', dict(shape=(3, 9, 9, 8), up=1, down=1, pad=(1, 1, 1, 1), g_pad=(2, 2, 2, 2), **fir)),
           ('down2', dict(shape=(3, 8, 8, 8), up=1, down=2, pad=(1, 1, 1, 1), g_pad=(2, 1, 2, 1), **fir)),
           ('up2', dict(shape=(6, 4, 5, 1), up=2, down=1, pad=(2, 1, 2, 1), g_pad=(1, 1, 1, 1), kgain=4.0, **fir)),
           ('neg', dict(shape=(2, 9, 9, 8), up=1, down=1, pad=(-1, 1, -1, 1), g_pad=(4, 2, 4, 2), **fir))]
    for tag, c in ufd:
        add('UpFirDn2dFn', tag, c, 'element-wise')
        u, d = c['up'], c['down']
        B, H, W, C = c['shape']
        oh, ow = S.out_size(H, W, 4, 4, u, u, d, d, *c['pad'])
        add('UpFirDn2dBackwardFn', tag, dict(c, shape=(B, oh, ow, C), in_hw=(H, W)), 'element-wise')
    for B, splits in ((8, None), (12, (4, 8)), (3, None), (16, (16,))):
        tag = 'b%d%s' % (B, '-split' if splits and len(splits) > 1 else '')
        add('MinibatchStddevFn', tag, dict(shape=(B, 4, 4, 32), cpad=48, splits=splits), 'minibatch-stddev', seed=B)
        add('MinibatchStddevBwdFn', tag, dict(shape=(B, 4, 4, 32), cpad=48, splits=splits), 'minibatch-stddev', seed=B)
    add('SumSqMeanFn', 'img', dict(shape=(6, 3, 8, 8)), 'element-wise')
    for i, (a, b) in enumerate(((1.0, 1.0), (0.5, 0.5), (f32(2 ** -0.5), f32(0.3)))):
        add('LinCombFn', 'c%d' % i, dict(shape=(2, 5, 5, 12), a=a, b=b), 'element-wise')
    add('PackWeightsFn', '3in2', _PACK, 'pack / sn')
    add('UnpackWeightsFn', '3in2', _PACK, 'pack / sn')
    add('SnPackWeightsFn', 'train', dict(_SN, training=True), 'pack / sn')
    add('SnPackWeightsFn', 'eval', dict(_SN, training=False), 'pack / sn')
    add('NhwcScaleFn', 'n3', dict(shape=(3, 4, 5, 12)), 'element-wise')
    add('ModconvEpilogueFn', 'n3', dict(shape=(3, 4, 5, 12)), 'element-wise')
    return out


# a case whose default seed puts a pre-activation within GUARD of the kink gets another seed here (none needs one today:
# tests/test_nodes_ref64_cpu.py::test_every_activated_case_keeps_clear_of_the_kink asserts the condition for all of them)
SEEDS = {}
CASES = _cases()
for _c in CASES:
    _c['seed'] = SEEDS.get(_c['id'], _c['seed'])
BY_ID = {c['id']: c for c in CASES}


def conv_descs(case):
    """(N, H, W, C, K, k, s, p, ldw) of the conv-engine calls a conv case makes: the forward, dgrad and wgrad calls of its
    root, first and second backward all share one geometry."""
    c = case['cfg']
    return (c['N'], c['H'], c['W'], c['C'], c['K'], c['k'], c['s'], c['p'], _geo(c)[2])
