"""Float64 restatements of the baseline-mode augmentations (HorizontalFlipRandomCrop, DiffAugment), their adjoints and the
consistency terms, in plain torch on the CPU -- none of this project's kernels, like aug_ref64.py.

Parameter blocks are those of include/contrad_hip.h: hfrt rows {sign, kx, ky, -}, DiffAugment rows {b, s, c, tx, ty, ox, oy,
-}.  The forward functions restate the reference's definitions stage by stage (DiffAugment's contrast stage takes the
true mean of its input, not the M = mean(u) + b shortcut of the kernel, so the shortcut is what gets tested); the adjoints
are written out by hand and compared with float64 autograd of the forward functions in test_baselines_ref64_cpu.py.
"""
import torch

STAGES = ('color', 'translation', 'cutout')


def _reflect(t, n):
    return torch.where(t < 0, -t - 1, torch.where(t >= n, 2 * n - 1 - t, t))


def hfrt_indices(p_row, H, W):
    """Source row of every output row, source column of every output column, for one parameter row."""
    sign, kx, ky = float(p_row[0]), int(p_row[1]), int(p_row[2])
    i, j = torch.arange(H), torch.arange(W)
    return _reflect(i + ky, H), _reflect((j if sign > 0 else W - 1 - j) + kx, W)


def hfrt_forward(x, P):
    """y[n, c, i, j] = x[n, c, rows[i], cols[j]] (augment/spatial.py:14-40 as an index map); dtype of x is kept."""
    out = torch.empty_like(x)
    for n in range(x.shape[0]):
        rows, cols = hfrt_indices(P[n], x.shape[2], x.shape[3])
        out[n] = x[n][:, rows][:, :, cols]
    return out


def hfrt_adjoint(g, P):
    """Transpose of hfrt_forward: every input pixel sums the outputs that read it."""
    g = g.double()
    out = torch.zeros_like(g)
    for n in range(g.shape[0]):
        H, W = g.shape[2], g.shape[3]
        rows, cols = hfrt_indices(P[n], H, W)
        tmp = torch.zeros_like(g[n]).index_add_(2, cols, g[n])
        out[n].index_add_(1, rows, tmp)
    return out


def policy_set(policy):
    names = [p for p in policy.split(',') if p]
    assert names == [s for s in STAGES if s in names], 'stages in the order color, translation, cutout'
    return set(names)


def cutout_mask(p_row, H, W):
    """1 where the pixel survives (third_party/diffaug.py:57-71)."""
    ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
    ox, oy = int(p_row[5]), int(p_row[6])
    rows = torch.clamp(torch.arange(ch) + ox - ch // 2, 0, H - 1)
    cols = torch.clamp(torch.arange(cw) + oy - cw // 2, 0, W - 1)
    m = torch.ones(H, W, dtype=torch.float64)
    m[rows[:, None], cols[None, :]] = 0
    return m


def _translate(u, tx, ty):
    """out[:, i, j] = u[:, i + tx, j + ty], zero outside."""
    C, H, W = u.shape
    out = torch.zeros_like(u)
    i0, i1 = max(0, -tx), min(H, H - tx)
    j0, j1 = max(0, -ty), min(W, W - ty)
    if i0 < i1 and j0 < j1:
        out[:, i0:i1, j0:j1] = u[:, i0 + tx:i1 + tx, j0 + ty:j1 + ty]
    return out


def diffaug_forward(x, P, policy):
    """DiffAugment (third_party/diffaug.py) in float64; differentiable in x."""
    pol = policy_set(policy)
    x = x.double()
    outs = []
    for n in range(x.shape[0]):
        p = P[n].double()
        u = 2.0 * x[n] - 1.0
        if 'color' in pol:
            u = u + p[0]
            m = u.mean(dim=0, keepdim=True)
            u = (u - m) * p[1] + m
            m = u.mean()
            u = (u - m) * p[2] + m
        if 'translation' in pol:
            u = _translate(u, int(p[3]), int(p[4]))
        if 'cutout' in pol:
            u = u * cutout_mask(p, u.shape[1], u.shape[2])
        outs.append(0.5 * u + 0.5)
    return torch.stack(outs)


def diffaug_dead_outputs(P, policy, H, W):
    """(B, H, W) bool: output pixels that are cut or read outside the image (exactly 0.5 in the forward)."""
    pol = policy_set(policy)
    dead = torch.zeros(P.shape[0], H, W, dtype=torch.bool)
    for n in range(P.shape[0]):
        if 'translation' in pol:
            live = _translate(torch.ones(1, H, W, dtype=torch.float64), int(P[n, 3]), int(P[n, 4]))[0]
            dead[n] |= live == 0
        if 'cutout' in pol:
            dead[n] |= cutout_mask(P[n], H, W) == 0
    return dead


def diffaug_backward(g, P, policy):
    """Transpose of diffaug_forward, written out: g3 = 0.5 g masked and un-translated; gu2 = c g3 + (1 - c) mean_chw(g3);
    gu1 = s gu2 + (1 - s) mean_c(gu2); gx = 2 gu1."""
    pol = policy_set(policy)
    g = g.double()
    outs = []
    for n in range(g.shape[0]):
        p = P[n].double()
        t = 0.5 * g[n]
        if 'cutout' in pol:
            t = t * cutout_mask(p, t.shape[1], t.shape[2])
        if 'translation' in pol:
            t = _translate(t, -int(p[3]), -int(p[4]))
        if 'color' in pol:
            t = p[2] * t + (1 - p[2]) * t.mean()
            t = p[1] * t + (1 - p[1]) * t.mean(dim=0, keepdim=True)
        outs.append(2.0 * t)
    return torch.stack(outs)


def consistency(a, b, n0, n1, lbd0, lbd1):
    """lbd0 mean_{[0,n0)} (a - b)^2 + lbd1 mean_{[n0, n0+n1)} (a - b)^2 (penalty.py:45-58) -> (value, d/da, d/db)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = a - b
    val = lbd0 * d[:n0].pow(2).mean()
    w = torch.full_like(d, 2.0 * lbd0 / n0)
    if n1 > 0:
        val = val + lbd1 * d[n0:n0 + n1].pow(2).mean()
        w[n0:] = 2.0 * lbd1 / n1
    ga = w * d
    return val, ga.reshape(-1, 1), (-ga).reshape(-1, 1)
