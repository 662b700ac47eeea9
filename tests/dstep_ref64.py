"""Float64 references of the non-conv kernels of the training steps (csrc/ntxent.hip, specnorm.hip, conv_small.hip,
elementwise.hip), in plain torch on whatever device the inputs live on, using none of this project's kernels.  Every
function takes the tensors the kernel under test read (fp32) and returns float64 results, so that the difference is the
kernel's own error.  tests/test_dstep_ref64_cpu.py checks each one against CPU float64 autograd / torch.optim.Adam."""
import torch
import torch.nn.functional as F

DIAG = -5e4          # the reference's fill_diagonal_ value (training/criterion.py)
f64 = torch.float64


def _d(t):
    return None if t is None else t.to(f64)


# ---- contrastive losses ----------------------------------------------------------------------------------------------
def contrast(z, N, mode, temperature):
    """z (R, D) rows as the kernel read them -> (loss, lse (R,), dZ (R, D)) of NT-Xent (mode 0, R = 2N) or the
    fake-anchored SupCon term (mode 1, R = 3N), in closed form: dZ = inv_temp * (G + G^T) Z,
    G_ij = c * (softmax_ij - T_ij) over the anchor rows i."""
    z = _d(z)
    R = z.shape[0]
    S = z @ z.t() / temperature
    S.fill_diagonal_(DIAG)
    lse = torch.logsumexp(S, 1)
    T = torch.zeros_like(S)
    idx = torch.arange(R, device=z.device)
    if mode == 0:
        T[idx, (idx + N) % (2 * N)] = 1.0
        anchor = torch.ones(R, dtype=torch.bool, device=z.device)
        c = 1.0 / (2 * N)
    else:
        T[2 * N:, 2 * N:] = 1.0 / (N - 1)
        T.fill_diagonal_(0.0)
        anchor = idx >= 2 * N
        c = 1.0 / N
    rowloss = torch.where(anchor, lse - (T * S).sum(1), torch.zeros_like(lse))
    G = c * (torch.exp(S - lse[:, None]) - T) * anchor[:, None]
    G.fill_diagonal_(0.0)
    dz = (G + G.t()) @ z / temperature
    return rowloss.sum() * c, lse, dz


def l2norm(u, eps=1e-12):
    """u (R, D) -> (z, 1 / max(|u|, eps)) of F.normalize."""
    u = _d(u)
    inv = 1.0 / u.norm(dim=1).clamp_min(eps)
    return u * inv[:, None], inv


def l2norm_bwd(dz, u, eps=1e-12):
    """d/du of F.normalize(u) against the upstream dz: (dz - z <z, dz>) / |u|."""
    z, inv = l2norm(u, eps)
    dz = _d(dz)
    return (dz - z * (z * dz).sum(1, keepdim=True)) * inv[:, None]


# ---- spectral norm / packed weights ----------------------------------------------------------------------------------
def pack(w2d, C, T):
    """W (K, C*T) with column c*T + tap -> the packed GEMM layout (T*C, K), row tap*C + c."""
    K = w2d.shape[0]
    return w2d.reshape(K, C, T).permute(2, 1, 0).reshape(T * C, K)


def unpack(wp, K, C, T):
    """(T*C, >= K) packed rows -> W (K, C*T)."""
    return wp[:, :K].reshape(T, C, K).permute(2, 1, 0).reshape(K, C * T)


def sn_prep(w2d, u, v, training, eps=1e-12, fixed_scale=0.0):
    """torch.nn.utils.spectral_norm's pre-forward hook (one power iteration in training mode), or the fixed runtime
    scale: -> (W_eff (K, IN), u', v', sigma)."""
    w, u, v = _d(w2d), _d(u), _d(v)
    if fixed_scale > 0:
        return w * fixed_scale, u, v, torch.tensor(1.0 / fixed_scale, dtype=f64, device=w.device)
    if training:
        v = F.normalize(w.t() @ u, dim=0, eps=eps)
        u = F.normalize(w @ v, dim=0, eps=eps)
    sigma = torch.dot(u, w @ v)
    return w / sigma, u, v, sigma


def sn_grad(g_eff, w2d, u, v, fixed_scale=0.0):
    """dL/dW_orig (K, IN) from dL/dW_eff with u, v constant in the graph: (G - <G, W/sigma> u v^T) / sigma."""
    g, w = _d(g_eff), _d(w2d)
    if fixed_scale > 0:
        return g * fixed_scale
    u, v = _d(u), _d(v)
    sigma = torch.dot(u, w @ v)
    return (g - (g * w).sum() / sigma * torch.outer(u, v)) / sigma


# ---- RGB-end convolutions --------------------------------------------------------------------------------------------
def rgb_fwd(img, w, bias, in_scale, in_shift, slope, gain):
    """img NCHW, w (K, C, k, k) -> NHWC gain * lrelu_slope(conv(img * in_scale + in_shift) + bias), 'same' padding."""
    k = w.shape[-1]
    y = F.conv2d(_d(img) * in_scale + in_shift, _d(w), _d(bias), padding=k // 2)
    y = torch.where(y > 0, y, y * slope) * gain
    return y.permute(0, 2, 3, 1)


def rgb_wgrad(img, gy, k, in_scale, in_shift):
    """img NCHW, gy NHWC (pre-activation gradient) -> (dw (K, C, k, k), dbias (K,))."""
    x = _d(img) * in_scale + in_shift
    N, C, H, W = x.shape
    K = gy.shape[3]
    cols = F.unfold(x, k, padding=k // 2)                              # (N, C*k*k, H*W)
    g = _d(gy).reshape(N, H * W, K)
    dw = torch.einsum('npk,ncp->kc', g, cols).reshape(K, C, k, k)
    return dw, g.sum((0, 1))


def rgb_dgrad(gy, w, bias, act=0, out_scale=1.0, out_shift=0.0, mod=None, residual=None):
    """gy NHWC (N,H,W,K), w (K, C, k, k) -> NCHW f(conv_transpose(gy * mod) + bias + residual) * out_scale + out_shift,
    f = tanh when act = 1."""
    k = w.shape[-1]
    g = _d(gy).permute(0, 3, 1, 2)
    if mod is not None:
        g = g * _d(mod)[:, :, None, None]
    y = F.conv_transpose2d(g, _d(w), _d(bias), padding=k // 2)
    if residual is not None:
        y = y + _d(residual)
    if act == 1:
        y = torch.tanh(y)
    return y * out_scale + out_shift


# ---- column statistics / BatchNorm -----------------------------------------------------------------------------------
def colstats(x2d):
    x = _d(x2d)
    return torch.stack([x.sum(0), (x * x).sum(0)])


def bn_relu(x2d, gamma, beta, eps, perm_hw=1):
    """BatchNorm (train: biased batch variance) + ReLU on (M, K) rows; perm_hw > 1 writes column c * perm_hw + hw to
    position hw * (K / perm_hw) + c."""
    x = _d(x2d)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    y = ((x - mean) / torch.sqrt(var + eps) * _d(gamma) + _d(beta)).clamp_min(0)
    if perm_hw > 1:
        M, K = y.shape
        y = y.reshape(M, K // perm_hw, perm_hw).transpose(1, 2).reshape(M, K)
    return y


def bn_relu_bwd(dy2d, x2d, gamma, beta, eps, mask=None):
    """-> (dx, dgamma, dbeta) of bn_relu (no permutation).  ``mask`` (bool, True where the ReLU passes) imposes the
    active set from outside instead of taking it from the sign of the float64 output: ReLU's derivative jumps at 0, and
    an fp32 forward whose output sits within its rounding of 0 must be judged on its own active set."""
    x, dy, gamma, beta = _d(x2d), _d(dy2d), _d(gamma), _d(beta)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    g = torch.where(xh * gamma + beta > 0 if mask is None else mask, dy, torch.zeros_like(dy))
    s1, s2 = g.sum(0), (g * xh).sum(0)
    M = x.shape[0]
    return gamma * rstd * (g - s1 / M - xh * s2 / M), s2, s1


def bn_relu_eval(x2d, conv_bias, running_mean, running_var, gamma, beta, eps, perm_hw=1):
    """Eval-mode BatchNorm + ReLU on (M, K) rows of a layer that ran without its bias ``conv_bias`` (None: no bias):
    relu(((x + cb) - rm) / sqrt(rv + eps) * gamma + beta); the output column permutation is that of bn_relu."""
    x = _d(x2d)
    if conv_bias is not None:
        x = x + _d(conv_bias)
    y = ((x - _d(running_mean)) / torch.sqrt(_d(running_var) + eps) * _d(gamma) + _d(beta)).clamp_min(0)
    if perm_hw > 1:
        M, K = y.shape
        y = y.reshape(M, K // perm_hw, perm_hw).transpose(1, 2).reshape(M, K)
    return y


# Regimes of eval-mode statistics: (scale of |running_mean - conv_bias|, scale of running_var, the max over 128 channels of
# mean^2 / var the draw below is meant to reach).  |mean| is scale * U(0.5, 1.5) with a random sign (A: 0.1 * randn, as
# O.det_fill draws it), var is scale * U(0.5, 2), so the largest ratio is about 2.8 scale_m^2 / scale_v.
BN_EVAL_REGIMES = {
    'A': (0.1, 1.0, 0.13),          # today's fixtures
    'B': (10.0, 1.0, 2.8e2),
    'C': (1.0, 1e-4, 2.8e4),
    'D': (10.0, 1e-4, 2.8e6),
    'E': (1.0, 1e-8, 2.8e8),        # var below one ulp of mean^2, and below eps
    'F': (1.0, None, 2.8e12),       # var exactly 0 / 1e-12 / 1e-4 by channel % 3; the ratio is over the channels with var > 0
    'G': (1.0, 1.0, 2.8),           # running_mean and conv_bias both near 100, their difference near 1
}
BN_EVAL_NEEDS_BIAS = ('G',)


def bn_eval_inputs(regime, M, K, seed, with_bias=True, device='cpu'):
    """-> dict(x (M, K), rm, rv, cb (or None), gamma, beta), all float32 on ``device``: x = (rm - cb) + sqrt(rv) * randn
    formed in float64 from the ROUNDED statistics and rounded once.  Drawn on the CPU generator: the same values on every
    device."""
    ms, vs, _ = BN_EVAL_REGIMES[regime]
    assert with_bias or regime not in BN_EVAL_NEEDS_BIAS
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=f64)
    n = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    sign = torch.where(r(K) < 0.5, -1.0, 1.0).to(f64)
    mean = 0.1 * n(K) if regime == 'A' else ms * (0.5 + r(K)) * sign
    if regime == 'F':
        rv = torch.tensor([0.0, 1e-12, 1e-4], dtype=f64)[torch.arange(K) % 3]
        r(K)
    else:
        rv = vs * (0.5 + 1.5 * r(K))
    cb = (100.0 + n(K)) if regime == 'G' else 0.1 * n(K)
    gamma, beta, z = r(K) + 0.5, 0.3 * n(K), n(M, K)
    cb = cb.float() if with_bias else None
    rm = (mean + (cb.double() if with_bias else 0)).float()
    rv = rv.float()
    x = (rm.double() - (cb.double() if with_bias else 0)) + torch.sqrt(rv.double()) * z
    out = dict(x=x.float(), rm=rm, rv=rv, cb=cb, gamma=gamma.float(), beta=beta.float())
    return {k: (None if v is None else v.to(device)) for k, v in out.items()}


def bn_eval_ratio(inp):
    """max over channels (with var > 0) of (rm - cb)^2 / rv."""
    mean = _d(inp['rm']) - (0 if inp['cb'] is None else _d(inp['cb']))
    rv = _d(inp['rv'])
    return float((mean * mean / rv)[rv > 0].max())


def bn_relu_eval_fp32(inp, eps, perm_hw=1):
    """Plain fp32 torch on the same tensors, on their device: F.relu(F.batch_norm(x + cb, rm, rv, gamma, beta)) -- the
    yardstick's own fp32 error sets the bound of the kernel (see bn_eval_bound)."""
    x = inp['x'].contiguous()
    if inp['cb'] is not None:
        x = x + inp['cb']
    y = F.relu(F.batch_norm(x, inp['rm'], inp['rv'], inp['gamma'], inp['beta'], False, 0.0, eps))
    if perm_hw > 1:
        M, K = y.shape
        y = y.reshape(M, K // perm_hw, perm_hw).transpose(1, 2).reshape(M, K)
    return y


def bn_eval_bound(family_tol, torch_errors, regime=None):
    """(max-norm, rel-L2) bounds of an eval BatchNorm output: max(the bn_fwd family bound, 2 x the error of plain fp32 torch
    on the same inputs).  The factor 2 covers the different rounding order (rsqrt against sqrt and divide; rm - cb rounded
    once per channel against x + cb rounded per element).  Regime A is held to the family bound alone."""
    if regime == 'A':
        return tuple(family_tol)
    return tuple(max(t, 2.0 * e) for t, e in zip(family_tol, torch_errors))


def bn_running(running_mean, running_var, x2d, conv_bias, momentum):
    """nn.BatchNorm's running update from the batch of the conv output WITHOUT its bias (folded in here)."""
    x = _d(x2d)
    m = x.mean(0) + (0 if conv_bias is None else _d(conv_bias))
    v = x.var(0, unbiased=x.shape[0] > 1)
    return (1 - momentum) * _d(running_mean) + momentum * m, (1 - momentum) * _d(running_var) + momentum * v


# ---- GAN logit losses ------------------------------------------------------------------------------------------------
def gan_d(d_real, d_gen, kind):
    """contrad.loss_D_fn -> (loss, d loss / d d_real, d loss / d d_gen)."""
    r, g = _d(d_real), _d(d_gen)
    N = r.numel()
    if kind == 'nonsat':
        return (F.softplus(g).mean() + F.softplus(-r).mean(), -torch.sigmoid(-r) / N, torch.sigmoid(g) / N)
    if kind == 'wgan':
        return g.mean() - r.mean(), -torch.ones_like(r) / N, torch.ones_like(g) / N
    if kind == 'hinge':
        return (F.relu(1 + g).mean() + F.relu(1 - r).mean(), -(1 - r > 0).to(f64) / N, (1 + g > 0).to(f64) / N)
    if kind == 'lsgan':
        return 0.5 * (((r - 1) ** 2).mean() + (g ** 2).mean()), (r - 1) / N, g / N
    raise ValueError(kind)


def gan_g(d, kind):
    """contrad.loss_G_fn -> (loss, d loss / d d)."""
    d = _d(d)
    N = d.numel()
    if kind == 'nonsat':
        return F.softplus(-d).mean(), -torch.sigmoid(-d) / N
    if kind == 'lsgan':
        return 0.5 * ((d - 1) ** 2).mean(), (d - 1) / N
    return -d.mean(), -torch.ones_like(d) / N


# ---- Adam ------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0):
    """One torch.optim.Adam step (no weight decay, no amsgrad) on float64 copies -> (p', m', v')."""
    p, g, m, v = _d(p), _d(g) * grad_scale, _d(m), _d(v)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - lr / bc1 * m / denom, m, v


def errors(out, ref):
    """(max-norm error max|e| / max|ref|, rel-L2 error ||e||_2 / ||ref||_2) of a float32 result against float64."""
    ref = ref.to(out.device, f64)
    e = out.to(f64) - ref
    return (e.abs().max() / ref.abs().max().clamp_min(1e-300)).item(), (e.norm() / ref.norm().clamp_min(1e-300)).item()
