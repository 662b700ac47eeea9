"""Float64 parity of every any-order autograd node (contrad_amd/autograd_ops.py), node by node, to second order.

The kernels under the nodes have element-wise float64 parity of their own (test_conv_paths_gpu.py, test_dstep_kernels_gpu.py,
test_sg2_ops_kernels_gpu.py, test_gp_kernels_gpu.py); what can still be wrong is the wiring: which node a backward calls,
with which tensor in which slot, g_pad, (k, scale, 0) versus (k, a, b), packed cotangents wider than K, the
needs_input_grad / input_grad_only branches, non-dense tensors through _cont, the fused / unfused bias gradient, the
u / v snapshots.  The protocol (tests/nodes_ref64.py: protocol) runs the same steps on the HIP node and on its float64 twin --

    out = Node(a...);  g = grad(out, a, r, create_graph=True);  s = grad(g, (a..., r), h, allow_unused=True)

-- and every out, g_i and s_j is compared on the whole tensor (max-norm and rel-L2, conv_ref64.errors' definitions) with
the bound of its class and order (TOL: about 5x the worst observed on an MI355X, through ``margin``) and with the 1e-3
contract.  Where the twin gives None or zeros the node must give None or exact zeros.  Every call is made twice and must
repeat bitwise.  tests/test_nodes_ref64_cpu.py proves the twins, the guard condition of the activated cases, the planner
coverage of the conv cases and the sensitivity of this protocol without a GPU.
"""
import pytest
import torch

import nodes_ref64 as N
from contrad_amd import autograd_ops as A

pytestmark = pytest.mark.gpu

CONTRACT = 1e-3
DEV = 'cuda'

# class: {order: (max-norm, rel-L2)}, order 0 = value, 1 = first-order gradients, 2 = second-order gradients.
# 5x the worst observed against the float64 twin on an MI355X over this module (survey run: CONTRAD_MARGINS with
# CONTRAD_MARGINS_NOASSERT), and no bound below 3e-7 = 5 fp32 roundings (pack / sn order 2 is one scaling by a power of
# two: observed error 0).                                     # observed worst (max-norm, rel-L2)
TOL = {
    'conv direct': {0: (2.3e-06, 2e-06),                      # 4.6e-07, 3.9e-07
                    1: (3.4e-06, 2e-06),                      # 6.9e-07, 4.1e-07
                    2: (3.8e-06, 2.2e-06)},                   # 7.5e-07, 4.3e-07
    'conv Winograd': {0: (1.5e-05, 5.6e-06),                  # 2.9e-06, 1.1e-06
                      1: (1e-05, 4.3e-06),                    # 2.0e-06, 8.5e-07
                      2: (1.1e-05, 5.6e-06)},                 # 2.3e-06, 1.1e-06
    'conv F(4x4)': {0: (2.9e-05, 6.5e-06),                    # 5.8e-06, 1.3e-06
                    1: (3.3e-05, 6.5e-06),                    # 6.5e-06, 1.3e-06
                    2: (2.9e-05, 6.5e-06)},                   # 5.8e-06, 1.3e-06
    'RGB': {0: (2.2e-06, 1.7e-06),                            # 4.3e-07, 3.4e-07
            1: (3.5e-06, 2.1e-06),                            # 6.9e-07, 4.2e-07
            2: (4e-06, 2.3e-06)},                             # 7.9e-07, 4.5e-07
    'element-wise': {0: (9.1e-07, 4.4e-07),                   # 1.8e-07, 8.8e-08
                     1: (6.5e-06, 6.5e-06),                   # 1.3e-06, 1.3e-06
                     2: (8.1e-07, 5.7e-07)},                  # 1.6e-07, 1.1e-07
    'minibatch-stddev': {0: (3e-07, 3e-07),                   # 4.6e-08, 2.6e-08
                         1: (3.1e-05, 1.6e-05),               # 6.1e-06, 3.2e-06
                         2: (0.0001, 5.8e-05)},               # 2.1e-05, 1.2e-05
    'pack / sn': {0: (1.1e-06, 1.1e-06),                      # 2.3e-07, 2.2e-07
                  1: (2.2e-06, 2.4e-06),                      # 4.5e-07, 4.8e-07
                  2: (3e-07, 3e-07)},                         # 0.0e+00, 0.0e+00
}


# ---- the HIP side of every case: HIP[node](cfg, *fp32 device tensors) ------------------------------------------------
def _geom(c):
    return (c['K'], c['k'], c['k'], c['s'], c['p'])


def _wp_shape(c):
    return (c['k'] * c['k'] * c['C'], c.get('ldw', N.round4(c['K'])))


def _rgb(c):
    return (c['k'], c['a'], c['b'])


def _rgb_wp_shape(c):
    return (c['k'] * c['k'] * 3, N.round4(c['K']))


class _SnModule(object):
    """What SnPackWeightsFn reads of a spectral-normed module: its power-iteration buffers."""

    def __init__(self, u, v):
        self.weight_u, self.weight_v = u.clone(), v.clone()          # (training mode advances them in place)


def sn_modules(c, t):
    n = len(c['kcts'])
    mods = [_SnModule(u, v) for u, v in zip(t[n:2 * n], t[2 * n:])]
    return [m if len(s) == 4 else (m, kct) for m, s, kct in zip(mods, c['shapes'], c['kcts'])]      # (one view_kct entry)


def _sn_pack(c, *t):
    return A.SnPackWeightsFn.apply(sn_modules(c, t), c['training'], *t[:len(c['kcts'])])


HIP = {
    'Conv2dFn': lambda c, x, wp: A.Conv2dFn.apply(x, wp, _geom(c)),
    'ConvDgradFn': lambda c, gy, wp: A.ConvDgradFn.apply(gy, wp, (c['N'], c['H'], c['W'], c['C']), _geom(c)),
    'ConvWgradFn': lambda c, x, gy: A.ConvWgradFn.apply(x, gy, _geom(c), _wp_shape(c)),
    'ConvWgradBiasFn': lambda c, x, gy: A.ConvWgradBiasFn.apply(x, gy, _geom(c), _wp_shape(c)),
    'ActFn': lambda c, x: A.ActFn.apply(x, c['slope'], c['gain']),
    'ActBwdFn': lambda c, g, y: A.ActBwdFn.apply(g, y, c['slope'], c['gain']),
    'ColSumFn': lambda c, g: A.ColSumFn.apply(g),
    'ConvBiasActFn': lambda c, x, wp, b: A.ConvBiasActFn.apply(x, wp, b, _geom(c), c['slope'], c['gain']),
    'RgbConvFn': lambda c, img, wp: A.RgbConvFn.apply(img, wp, c['K'], _rgb(c)),
    'RgbDgradFn': lambda c, g, wp: A.RgbDgradFn.apply(g, wp, 3, (c['k'], c['a'])),
    'RgbWgradFn': lambda c, img, g: A.RgbWgradFn.apply(img, g, _rgb(c), _rgb_wp_shape(c)),
    'RgbConvBiasActFn': lambda c, img, wp, b: A.RgbConvBiasActFn.apply(img, wp, b, c['K'], _rgb(c), c['slope'], c['gain']),
    'UpFirDn2dFn': lambda c, x, k: A.UpFirDn2dFn.apply(x, k, c['up'], c['down'], c['pad']),
    'UpFirDn2dBackwardFn': lambda c, gy, k: A.UpFirDn2dBackwardFn.apply(gy, k, c['up'], c['down'], c['pad'], c['g_pad'],
                                                                         c['in_hw']),
    'MinibatchStddevFn': lambda c, x: A.MinibatchStddevFn.apply(x, c['cpad'], c['splits']),
    'MinibatchStddevBwdFn': lambda c, x, gy: A.MinibatchStddevBwdFn.apply(x, gy, c['splits']),
    'SumSqMeanFn': lambda c, g: A.SumSqMeanFn.apply(g),
    'LinCombFn': lambda c, x, z: A.LinCombFn.apply(x, z, c['a'], c['b']),
    'PackWeightsFn': lambda c, *ws: A.PackWeightsFn.apply(A.PackMeta(c['entries'], c['groups']), *ws),
    'UnpackWeightsFn': lambda c, *g: A.UnpackWeightsFn.apply(A.PackMeta(c['entries'], c['groups']), c['shapes'], *g),
    'SnPackWeightsFn': _sn_pack,
    'NhwcScaleFn': lambda c, x, s: A.NhwcScaleFn.apply(x, s),
    'ModconvEpilogueFn': lambda c, y, demod, noise, nw, b: A.ModconvEpilogueFn.apply(y, demod, noise, nw, b),
}
BEHAVIOUR_ONLY = ('ZeroGradFn',)          # no arithmetic of its own: test_zero_grad_node


def hip_fn(case):
    return lambda *t: HIP[case['node']](case['cfg'], *t)


def run_hip(case, fn=None, drop=None, draw=None):
    return N.protocol(fn or hip_fn(case), N.inputs(case), N.diff_flags(case), draw or N.drawer(case),
                      N.SPECS[case['node']][3], torch.float32, DEV, drop)


def bitwise(a, b):
    assert set(a) == set(b)
    for key in a:
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None:
            assert torch.equal(a[key], b[key]), key


def check(margin, case, got, ref):
    cls = case['cls']
    for key, order, emax, el2, exact in N.compare(got, ref):
        print('%-40s %-5s max-norm %.3e  rel-L2 %.3e%s' % (case['id'], key, emax, el2, '  (exact)' if exact else ''))
        assert emax < CONTRACT and el2 < CONTRACT, (case['id'], key, emax, el2)
        if not exact:
            margin('node %-17s order %d  max-norm' % (cls, order), emax, TOL[cls][order][0])
            margin('node %-17s order %d  rel-L2' % (cls, order), el2, TOL[cls][order][1])


def parity(margin, case, fn=None, drop=None):
    got = run_hip(case, fn, drop)
    bitwise(got, run_hip(case, fn, drop))                     # every call twice: the same bits
    ref, lo = N.reference(case, DEV, drop)
    assert lo >= N.GUARD
    check(margin, case, got, ref)
    return got, ref


@pytest.mark.parametrize('case', N.CASES, ids=lambda c: c['id'])
def test_node_matches_its_float64_twin(case, margin):
    got, ref = parity(margin, case)
    if case['node'] in ('MinibatchStddevFn', 'MinibatchStddevBwdFn'):
        C = case['cfg']['shape'][3]
        key = 'sr0' if case['node'] == 'MinibatchStddevFn' else 'g1'          # the gradient into gy: (B,H,W,Cp)
        assert got[key].shape[3] == case['cfg']['cpad'] and not bool(got[key][..., C + 1:].ne(0).any())
        if case['node'] == 'MinibatchStddevFn':
            assert not bool(got['out0'][..., C + 1:].ne(0).any())
    # piecewise linear in x, linear in the bias: the second-order gradient w.r.t. ActFn's input and w.r.t. the bias is
    # structurally zero (the twin gives None; compare() has already demanded None or exact zeros)
    for key in {'ActFn': ('s0',), 'ConvBiasActFn': ('s2',), 'RgbConvBiasActFn': ('s2',)}.get(case['node'], ()):
        assert ref[key] is None or not bool(ref[key].ne(0).any())
        assert got[key] is None or not bool(got[key].ne(0).any()), key


@pytest.mark.parametrize('cid,drop', [('ConvWgradBiasFn-k3s1p1', 0), ('ConvWgradBiasFn-k3s1p1', 1), ('PackWeightsFn-3in2', 1),
                                      ('UnpackWeightsFn-3in2', 2)])
def test_multi_output_node_with_one_cotangent_missing(cid, drop, margin):
    parity(margin, N.BY_ID[cid], drop=drop)


def test_unpack_with_a_none_group_gradient(margin):
    """UnpackWeightsFn reads a missing group gradient as zeros: the twin is given the zeros."""
    case = N.BY_ID['UnpackWeightsFn-3in2']
    c = case['cfg']
    ins = [t.to(DEV) for t in N.inputs(case)]
    outs = A.UnpackWeightsFn.apply(A.PackMeta(c['entries'], c['groups']), c['shapes'], ins[0], None)
    refs = N.unpack_groups(c['entries'], c['shapes'], [ins[0].double(), torch.zeros(c['groups'][1], dtype=N.f64, device=DEV)])
    for o, r, e in zip(outs, refs, c['entries']):
        if e[4] == 1:
            assert not bool(o.ne(0).any())
        else:
            check(margin, case, {'out0': o}, {'out0': r})


def test_packed_padding_columns_are_never_read():
    """K = 6 in ldw = 8: the results are bitwise those of the same cotangents with zeros in the padding columns."""
    for cid in ('ConvWgradFn-k6', 'Conv2dFn-k6', 'ConvDgradFn-k6', 'ConvBiasActFn-a0-k6'):
        case = N.BY_ID[cid]
        assert case['cfg']['padfill'] and N._geo(case['cfg'])[2] == 8
        filled, seen = N.drawer(case), []
        zeroed = N.drawer(dict(case, cfg=dict(case['cfg'], padfill=False)))

        def spy(shapes, what):
            ts = filled(shapes, what)
            seen.extend(bool((t == N.PAD_FILL).any()) for t in ts)
            return ts
        bitwise(run_hip(case, draw=spy), run_hip(case, draw=zeroed))
        assert any(seen), cid


def test_bias_gradient_branches():
    """C and K multiples of 4: one ConvWgradBiasFn launch; otherwise ConvWgradFn + ColSumFn, and the fused node's launcher
    rejects the shape."""
    for cid, fused in (('ConvBiasActFn-a0-k3s1p1', True), ('ConvBiasActFn-a0-k6', False)):
        case = N.BY_ID[cid]
        c = case['cfg']
        assert A._fused_bias_ok(torch.empty(c['N'], c['H'], c['W'], c['C']), c['K']) == fused
        x, wp, b = [t.to(DEV).requires_grad_() for t in N.inputs(case)]
        y = hip_fn(case)(x, wp, b)
        gw, gb = torch.autograd.grad(y, (wp, b), torch.ones_like(y), create_graph=True)
        names = (type(gw.grad_fn).__name__, type(gb.grad_fn).__name__)
        assert names == (('ConvWgradBiasFnBackward',) * 2 if fused else ('ConvWgradFnBackward', 'ColSumFnBackward')), names
    c = N.BY_ID['ConvWgradFn-k6']['cfg']
    x, gy = [t.to(DEV) for t in N.inputs(N.BY_ID['ConvWgradFn-k6'])]
    with pytest.raises(RuntimeError):
        A.ConvWgradBiasFn.apply(x, gy, _geom(c), _wp_shape(c))


@pytest.mark.parametrize('node', ['RgbConvFn', 'RgbDgradFn', 'RgbWgradFn'])
def test_rgb_launchers_reject_k_that_is_no_multiple_of_4(node):
    c = dict(N=2, H=4, W=4, K=6, k=3, a=2.0, b=-1.0)
    ins = [t.to(DEV) for t in N.SPECS[node][0](c, torch.Generator().manual_seed(0))]
    with pytest.raises(RuntimeError):
        HIP[node](c, *ins)
        torch.cuda.synchronize()


def test_upfirdn_backward_follows_an_in_place_change_of_the_fir_buffer(margin):
    """flipped_kernel is keyed on the buffer's version: a backward after ``kernel.mul_()`` uses the new flipped taps."""
    case = N.BY_ID['UpFirDn2dFn-blur22']
    c = case['cfg']
    x, k = [t.to(DEV) for t in N.inputs(case)]
    x.requires_grad_()
    r = torch.randn(3, 10, 10, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    torch.autograd.grad(HIP['UpFirDn2dFn'](c, x, k), x, r)                       # (fills the cache for this version)
    k.mul_(torch.arange(1.0, 17.0, device=DEV).view(4, 4))                      # asymmetric taps, same storage
    g, = torch.autograd.grad(HIP['UpFirDn2dFn'](c, x, k), x, r)
    x64 = x.detach().double().requires_grad_()
    ref, = torch.autograd.grad(N.t_upfirdn(c, x64, k.double()), x64, r.double())
    check(margin, case, {'g0': g}, {'g0': ref})


def test_minibatch_stddev_refuses_a_non_dense_input():
    t = torch.randn(8, 4, 4, 36, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        A.MinibatchStddevFn.apply(t[..., :32], 48, None)


def test_zero_grad_node():
    """ZeroGradFn: identity in value; exact zeros of the parameters' shapes; None for a frozen parameter and inside
    input_grad_only()."""
    out = torch.randn(4, 3, device=DEV, requires_grad=True)
    p1 = torch.randn(5, 2, device=DEV, requires_grad=True)
    p2 = torch.randn(7, device=DEV, requires_grad=False)
    p3 = torch.randn(2, 3, 1, 1, device=DEV, requires_grad=True)
    r = torch.randn(4, 3, device=DEV)
    y = A.ZeroGradFn.apply(out, p1, p2, p3)
    assert torch.equal(y, out)
    g = torch.autograd.grad(y, (out, p1, p3), r, retain_graph=True)
    assert torch.equal(g[0], r)
    for gi, p in zip(g[1:], (p1, p3)):
        assert gi.shape == p.shape and not bool(gi.ne(0).any())
    y.backward(r)
    assert p2.grad is None and torch.equal(out.grad, r)
    with A.input_grad_only():
        y = A.ZeroGradFn.apply(out, p1, p2, p3)
        g = torch.autograd.grad(y, (out, p1, p3), r, allow_unused=True)
    assert torch.equal(g[0], r) and g[1] is None and g[2] is None
    frozen = A.ZeroGradFn.apply(out, p1.detach(), p2)
    g = torch.autograd.grad(frozen, out, r)
    assert torch.equal(g[0], r)


def test_sn_snapshot_is_that_of_its_own_forward(margin):
    """A second forward advances weight_u / weight_v in place; the backward of the first still uses the first's u, v."""
    case = N.BY_ID['SnPackWeightsFn-train']
    c = case['cfg']
    n = len(c['kcts'])
    advanced = []

    def fn(*t):
        mods = sn_modules(c, t)
        outs = A.SnPackWeightsFn.apply(mods, True, *t[:n])
        first = [(m[0] if isinstance(m, tuple) else m).weight_u.clone() for m in mods]
        A.SnPackWeightsFn.apply(mods, True, *[torch.flip(w.detach(), [0]) * 1.5 for w in t[:n]])
        advanced.extend(not torch.equal(f, (m[0] if isinstance(m, tuple) else m).weight_u) for f, m in zip(first, mods))
        return outs
    parity(margin, case, fn)
    assert advanced and all(advanced)
    # the buffers a training forward leaves are the reference's u', v'
    t = [x.to(DEV) for x in N.inputs(case)]
    mods = sn_modules(c, t)
    A.SnPackWeightsFn.apply(mods, True, *t[:n])
    _, state = N.sn_pack([x.double() for x in t[:n]], [x.double() for x in t[n:2 * n]], [x.double() for x in t[2 * n:]],
                         c['kcts'], True)
    for m, (u, v, sigma) in zip(mods, state):
        m = m[0] if isinstance(m, tuple) else m
        check(margin, case, {'out0': m.weight_u, 'out1': m.weight_v}, {'out0': u, 'out1': v})


# ---- input_grad_only() -----------------------------------------------------------------------------------------------
FLAGGED = ['Conv2dFn-k3s1p1', 'ConvDgradFn-k3s1p1', 'ConvBiasActFn-a0-k3s1p1', 'ConvBiasActFn-a0-k6', 'RgbConvFn-k3-a2',
           'RgbDgradFn-k3-a2', 'RgbConvBiasActFn-a0']


@pytest.mark.parametrize('cid', FLAGGED)
def test_input_grad_only_returns_the_activation_gradient_alone(cid):
    case = N.BY_ID[cid]
    a = [t.to(DEV).requires_grad_() for t in N.inputs(case)]
    out = hip_fn(case)(*a)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    outside = torch.autograd.grad(out, a, r, retain_graph=True, create_graph=True)
    assert all(g is not None for g in outside)
    with A.input_grad_only():
        inside = torch.autograd.grad(out, a, r, retain_graph=True, create_graph=True, allow_unused=True)
    assert torch.equal(inside[0], outside[0])
    assert all(g is None for g in inside[1:])
    assert not A._INPUT_GRAD_ONLY


def test_input_grad_only_refuses_a_parameter_backward_and_restores_the_flag():
    case = N.BY_ID['PackWeightsFn-3in2']
    ws = [t.to(DEV).requires_grad_() for t in N.inputs(case)]
    outs = hip_fn(case)(*ws)
    with pytest.raises(RuntimeError, match='input_grad_only'):
        with A.input_grad_only():
            torch.autograd.grad(outs, ws, [torch.ones_like(o) for o in outs])
    assert A._INPUT_GRAD_ONLY is False
    with pytest.raises(KeyError):
        with A.input_grad_only():
            with A.input_grad_only():
                pass
            assert A._INPUT_GRAD_ONLY is True                  # (nested scopes restore what they found)
            raise KeyError('body')
    assert A._INPUT_GRAD_ONLY is False


def test_exchange_packed_reduces_at_the_production_site_unless_shared():
    class Comm(object):
        def __init__(self):
            self.seen = []

        def reduce_async(self, t):
            self.seen.append(t)

    gw = torch.ones(4, 4, device=DEV)
    comm, meta = Comm(), A.PackMeta([], [])
    A.exchange_packed((comm, meta, 1), gw)
    assert comm.seen == [gw] and meta.reduced == {1}
    meta.shared = True
    A.exchange_packed((comm, meta, 0), gw)
    assert len(comm.seen) == 1 and meta.reduced == {1}


# ---- non-dense tensors -----------------------------------------------------------------------------------------------
# (case, index of an input whose last dimension is its channel: a slice t[..., :C] of a wider tensor stands in for it)
SLICED = [('Conv2dFn-k3s1p1', 0), ('ConvDgradFn-k3s1p1', 0), ('ConvWgradFn-k3s1p1', 0), ('ConvWgradFn-k3s1p1', 1),
          ('ConvWgradBiasFn-k3s1p1', 1), ('ConvBiasActFn-a0-k3s1p1', 0), ('ActFn-a0', 0), ('ActBwdFn-a0', 0), ('ColSumFn-k12', 0),
          ('LinCombFn-c2', 0), ('LinCombFn-c2', 1), ('UpFirDn2dFn-blur22', 0), ('UpFirDn2dBackwardFn-down2', 0),
          ('RgbDgradFn-k3-a2', 0), ('RgbWgradFn-k3-a2', 1), ('MinibatchStddevBwdFn-b8', 1), ('NhwcScaleFn-n3', 0),
          ('ModconvEpilogueFn-n3', 0), ('SumSqMeanFn-img', 0)]


def _first(case, a, r_of):
    out = hip_fn(case)(*a)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    need = [t for t in a if t.requires_grad]
    g = torch.autograd.grad(outs, need, [r_of(o) for o in outs], allow_unused=True)
    return [o.detach() for o in outs] + list(g)


@pytest.mark.parametrize('cid,at', SLICED)
def test_a_channel_slice_gives_the_bits_of_its_dense_copy(cid, at):
    case = N.BY_ID[cid]
    diff = N.diff_flags(case)
    ins = [t.to(DEV) for t in N.inputs(case)]
    wide = torch.full(ins[at].shape[:-1] + (ins[at].shape[-1] + 4,), N.PAD_FILL, device=DEV)
    wide[..., :ins[at].shape[-1]] = ins[at]
    gen = torch.Generator().manual_seed(9)
    cots = {}

    def r_of(o):
        if tuple(o.shape) not in cots:
            cots[tuple(o.shape)] = torch.randn(o.shape, generator=gen).to(DEV) if o.dim() else torch.ones((), device=DEV)
        return cots[tuple(o.shape)]
    res = []
    for sliced in (False, True):
        src = wide.clone().requires_grad_(bool(diff[at]))
        a = [t.clone().requires_grad_(bool(d)) for t, d in zip(ins, diff)]
        a[at] = src[..., :ins[at].shape[-1]] if sliced else ins[at].clone().requires_grad_(bool(diff[at]))
        assert a[at].is_contiguous() != sliced
        out = _first(case, a, r_of)                # (the slice is no leaf; autograd.grad takes it all the same)
        res.append(out)
    for d, s in zip(*res):
        assert (d is None) == (s is None) and (d is None or torch.equal(d, s))


EXPANDED = ['Conv2dFn-k3s1p1', 'ConvDgradFn-k3s1p1', 'ConvWgradFn-k3s1p1', 'ConvBiasActFn-a0-k3s1p1', 'ConvBiasActFn-a0-k6',
            'ActFn-a0', 'ActBwdFn-a0', 'LinCombFn-c2', 'UpFirDn2dFn-blur22', 'UpFirDn2dBackwardFn-down2', 'RgbConvFn-k3-a2',
            'RgbDgradFn-k3-a2', 'RgbWgradFn-k3-a2', 'RgbConvBiasActFn-a0', 'MinibatchStddevFn-b8', 'MinibatchStddevBwdFn-b8',
            'NhwcScaleFn-n3', 'ModconvEpilogueFn-n3']


@pytest.mark.parametrize('cid', EXPANDED)
def test_an_expanded_cotangent_gives_the_bits_of_its_dense_copy(cid):
    """What ColSumFn.backward and the hb branch of ConvWgradBiasFn.backward hand on: one row expanded over the leading
    dimensions (all strides but the last are 0)."""
    case = N.BY_ID[cid]
    diff = N.diff_flags(case)
    ins = [t.to(DEV) for t in N.inputs(case)]
    gen = torch.Generator().manual_seed(11)
    rows = {}

    def expanded(o):
        if o.shape[-1] not in rows:
            rows[o.shape[-1]] = torch.randn(o.shape[-1], generator=gen).to(DEV)
        e = rows[o.shape[-1]].view((1,) * (o.dim() - 1) + (-1,)).expand(o.shape)
        assert not e.is_contiguous()
        return e
    res = [_first(case, [t.clone().requires_grad_(bool(d)) for t, d in zip(ins, diff)], r_of)
           for r_of in (expanded, lambda o: expanded(o).contiguous())]
    for e, d in zip(*res):
        assert (e is None) == (d is None) and (e is None or torch.equal(e, d))
